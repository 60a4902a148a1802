"""The host half of sentence pooling, no GPU: the fp64 oracle against independent fp32 NumPy expressions (within the bounds the GPU tests
use), the integer corpora's exactness claims against NumPy's own fp32 mean and std, load_frames on pickles, ResidentFrames' tables and
refusals on a CPU device, with_frames' refusals, the six widths, and the return codes of the two C entry points on arguments they must
refuse before any device work."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from multimodaltopicsegmentation_amd.frames import POOL_MODES, pooled_width
from tests import frame_pool_oracle as O
from tests.test_pca_cpu import corpus_of

# frames per sentence, per document: sizes 1 .. 5, round a wave's 64 lanes, 257 and 1025, and 32 | 33 (the last sentence held in registers
# alone, the first with a re-read row); a one-sentence document; the corpus' first and last sentences are a document's first and last
SENTENCE_FRAMES = [[3, 1025, 64, 1], [5], [2, 257, 65, 63, 4, 1], [33, 32]]
ROWS = [len(d) for d in SENTENCE_FRAMES]
TOTAL = sum(ROWS)


def test_the_oracle_agrees_with_fp32_numpy_within_the_bounds():
    """the reference's own expressions (mean, max, concatenate(mean | max, std), e[-1], next[0] - e[-1]) evaluated by NumPy in fp32: a
    pairwise order of summation, which the bounds cover like any other"""
    assert O.MODES == POOL_MODES                                                           # the oracle restates the product's six modes
    for wire in ('fp32', 'bf16'):
        docs = O.as_stored(O.real_frames(SENTENCE_FRAMES, 65), wire)
        e_m, e_s = O.bounds(docs)
        flat = [e for doc in docs for e in doc]
        mean = np.array([e.mean(axis=0) for e in flat])
        assert mean.dtype == np.float32
        want = O.pool(docs, 'mean_std')
        assert (np.abs(mean - want[:, :65]) <= e_m).all()
        assert (np.abs(np.array([np.std(e, axis=0) for e in flat]) - want[:, 65:]) <= e_s).all()
        assert np.array_equal(np.array([np.max(e, axis=0) for e in flat]), O.pool(docs, 'max'))
        assert np.array_equal(O.pool(docs, 'max_std'), np.concatenate([O.pool(docs, 'max'), want[:, 65:]], axis=1))
        assert np.array_equal(np.array([e[-1] for e in flat]), O.pool(docs, 'last'))
        gap = []
        for doc in docs:
            for i, e in enumerate(doc):
                gap.append(doc[i + 1][0].astype(np.float64) - e[-1] if i + 1 < len(doc) else e[-1].astype(np.float64))
        assert np.array_equal(np.array(gap), O.pool(docs, 'delta_gap'))
        assert (e_m > 0).all() and (e_s > 0).all()


def test_integer_corpora_are_exact_in_numpy_fp32_too():
    docs, centres = O.integer_frames(SENTENCE_FRAMES, 7)
    assert O.counts(docs).tolist() == [n for d in SENTENCE_FRAMES for n in d] and centres.shape == (TOTAL, 7)
    assert all(np.array_equal(e, np.rint(e)) and np.abs(e).max() <= 10 for doc in docs for e in doc)
    assert np.array_equal(O.as_stored(docs, 'bf16')[0][1], docs[0][1])                     # exact in bf16
    flat = [e for doc in docs for e in doc]
    want = O.integer_expected(docs, centres, 'mean_std')
    assert want.dtype == np.float32 and np.array_equal(want[:, :7], centres)
    assert np.array_equal(np.array([e.mean(axis=0) for e in flat]), want[:, :7])
    assert np.array_equal(np.array([np.std(e, axis=0) for e in flat]), want[:, 7:])
    assert np.abs(want[:, 7:] - O.pool(docs, 'mean_std')[:, 7:]).max() <= 4 * O.U32 * want[:, 7:].max()
    assert (want[O.counts(docs) == 1, 7:] == 0).all() and want[:, 7:].max() > 3
    for mode in O.MODES:
        assert O.integer_expected(docs, centres, mode).shape == (TOTAL, pooled_width(mode, 7))


def test_load_frames_reads_the_extractors_pickles(tmp_path):
    from multimodaltopicsegmentation_amd import load_frames
    g = np.random.default_rng(3)
    a = [g.standard_normal((n, 6)).astype(np.float32) for n in (3, 1, 4)]
    as_object = np.empty(3, dtype=object)
    for k, e in enumerate(a):
        as_object[k] = e
    single = [a[0], a[1][0], a[2]]                                                         # a 1-d entry: one frame
    for name, obj in (('object', as_object), ('list', list(a)), ('single', single)):
        with open(tmp_path / f'{name}.pkl', 'wb') as f:
            pickle.dump(obj, f)
    docs = load_frames(str(tmp_path), ['object', 'list', 'single'])
    assert len(docs) == 3
    for doc in docs:
        assert len(doc) == 3 and [e.shape for e in doc] == [(3, 6), (1, 6), (4, 6)]
        assert all(np.array_equal(x, y) for x, y in zip(doc, a))
    with pytest.raises(FileNotFoundError):
        load_frames(str(tmp_path), ['missing'])


def test_resident_frames_builds_its_tables_on_a_cpu_device_and_refuses_what_it_must():
    from multimodaltopicsegmentation_amd import ResidentFrames
    docs, _ = O.integer_frames(SENTENCE_FRAMES, 5)
    f = ResidentFrames(docs, 'cpu', wire_dtype='bf16')
    assert (len(f), f.n_docs, f.D, f.total_sentences, f.total_frames) == (4, 4, 5, TOTAL, sum(n for d in SENTENCE_FRAMES for n in d))
    assert f.sentences.tolist() == ROWS and f.frame_counts.tolist() == O.counts(docs).tolist()
    assert f._start_host.dtype == np.int64 and f._start_host.tolist() == np.concatenate([[0], np.cumsum(O.counts(docs))]).tolist()
    assert f._last_host.dtype == np.uint8 and np.flatnonzero(f._last_host).tolist() == (np.cumsum(ROWS) - 1).tolist()
    assert f.frames is None and f.frame_start is None and f.doc_last is None and f.nbytes == 0 and f.wire == torch.bfloat16
    assert [f.width(m) for m in POOL_MODES] == [5, 5, 10, 10, 5, 5]
    for mode in POOL_MODES:
        with pytest.raises(RuntimeError):
            f.pool(mode)                                                                   # valid: a CPU device has no fallback
    with pytest.raises(ValueError):
        f.pool('median')
    with pytest.raises(ValueError):
        ResidentFrames(docs, 'cpu', wire_dtype='fp16')
    with pytest.raises(ValueError):
        ResidentFrames([], 'cpu')
    with pytest.raises(ValueError, match='document 1'):
        ResidentFrames([docs[0], []], 'cpu')
    with pytest.raises(ValueError, match='sentence 2 of document 1 has no frames'):
        ResidentFrames([docs[0], [docs[2][0], docs[2][1], np.zeros((0, 5), dtype=np.float32)]], 'cpu')
    with pytest.raises(ValueError, match='sentence 1 of document 0 has width 4'):
        ResidentFrames([[docs[0][0], docs[0][1][:, :4]]], 'cpu')
    with pytest.raises(ValueError, match='sentence 0 of document 1 is 1-d'):
        ResidentFrames([docs[0], [docs[1][0][0]]], 'cpu')
    torch_docs = [[torch.from_numpy(np.array(e)) for e in doc] for doc in docs]           # tensors are taken like arrays
    assert ResidentFrames(torch_docs, 'cpu').frame_counts.tolist() == f.frame_counts.tolist()


def test_with_frames_refuses_mismatched_documents():
    from multimodaltopicsegmentation_amd import ResidentFrames
    docs, _ = O.integer_frames(SENTENCE_FRAMES, 5)
    text = np.zeros((TOTAL, 3), dtype=np.float32)
    corpus = corpus_of(text, ROWS, 'cpu')
    frames = ResidentFrames(docs, 'cpu')
    with pytest.raises(ValueError, match='documents'):
        corpus.with_frames(ResidentFrames(docs[:3], 'cpu'), 'mean')
    with pytest.raises(ValueError, match='document 2 has 6 sentences in the corpus but 5'):
        corpus.with_frames(ResidentFrames([docs[0], docs[1], docs[2][:5], docs[3]], 'cpu'), 'mean')
    with pytest.raises(ValueError, match='document 0'):
        corpus_of(text, [ROWS[1], ROWS[0]] + ROWS[2:], 'cpu').with_frames(frames, 'mean')  # the same sentences, other documents
    with pytest.raises(ValueError):
        corpus.with_frames(frames, 'median')
    with pytest.raises(ValueError):
        corpus.with_frames(frames, 'mean', field='targets')
    for field in ('embeddings', 'embeddings2', 'append'):
        with pytest.raises(RuntimeError):
            corpus.with_frames(frames, 'mean_std', field=field)                            # valid: a CPU device has no fallback


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    from multimodaltopicsegmentation_amd import _lib as L
    buf = (C.c_double * 16)()
    p = C.addressof(buf)                                             # a non-null HOST address: a refused call never reads it
    lib = L.lib

    def pool(in_dtype=L.F32, out_dtype=L.F32, n_sent=2, D=4, first=L.POOL_MEAN, with_std=1, frames=p, total=8, start=p, out=p, ld=8):
        return lib.mts_frame_pool(None, in_dtype, out_dtype, n_sent, D, first, with_std, frames, total, start, out, ld)

    def edges(in_dtype=L.F32, out_dtype=L.F32, n_sent=2, D=4, mode=L.EDGE_DELTA_GAP, frames=p, total=8, start=p, last=p, out=p, ld=4):
        return lib.mts_frame_edges(None, in_dtype, out_dtype, n_sent, D, mode, frames, total, start, last, out, ld)
    for call in (pool, edges):
        for hole in ('frames', 'start', 'out'):
            assert call(**{hole: None}) == 1, (call.__name__, hole)
        assert call(in_dtype=2) == 1 and call(in_dtype=-1) == 1 and call(out_dtype=7) == 1
        assert call(n_sent=0) == 1 and call(n_sent=-3) == 1 and call(D=0) == 1 and call(D=-1) == 1 and call(total=-1) == 1
    assert edges(last=None) == 1 and edges(mode=2) == 1 and edges(mode=-1) == 1
    assert edges(ld=3) == 1 and edges(mode=L.EDGE_LAST, ld=3) == 1
    assert pool(first=3) == 1 and pool(first=-1) == 1 and pool(with_std=2) == 1 and pool(first=L.POOL_NONE, with_std=0) == 1
    assert pool(ld=7) == 1 and pool(with_std=0, ld=3) == 1 and pool(first=L.POOL_NONE, ld=3) == 1 and pool(first=L.POOL_MAX, ld=7) == 1
    with pytest.raises(ValueError, match='ld_out'):
        L.check(pool(ld=7))
