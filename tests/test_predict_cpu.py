"""CPU tests of the prediction pass (multimodaltopicsegmentation_amd/predict.py, ResidentCorpus.from_documents) and of the host restatement
the GPU tests hold the kernel against (tests/segment_decode_oracle.py): the recurrence and walk back of mts_segment_decode against a
brute force over ALL admissible boundary sets, the segment-table rule, ``segment_audio`` against the reference's recorded spans (g23), the
rank merge, the spans, the saturated logits, and the unlabelled corpus' host half and refusals."""
import os

import numpy as np
import pytest
import torch

from tests import segment_decode_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
WEIGHTS = np.array([-3, -1, 0, 1, 2], dtype=np.int64)      # five values: ties between boundary sets are frequent


# ---- the oracle itself -----------------------------------------------------------------------------------------------------------
def test_recurrence_and_walk_back_equal_a_brute_force_over_all_admissible_sets():
    rng = np.random.default_rng(23)
    cases = tied = 0
    for n in range(0, 13):
        for m in range(1, 6):
            for _ in range(12):
                q = rng.choice(WEIGHTS, size=n)
                last = bool(rng.integers(2))
                tags = O.constrained_tags(q, m, last)
                assert tags.shape == (n,) and tags.dtype == np.uint8
                if n == 0:
                    continue
                assert tags[-1] == last and O.admissible(tags, m), (n, m, q, tags)
                want, tried = O.brute_force(q, m)
                got = int(q[:-1][tags[:-1] == 1].sum())
                assert got == want == O.dp_value(q, m), (n, m, q.tolist(), tags.tolist(), got, want)
                assert want >= 0 and tried >= 1                                     # the empty set is admissible
                if n < 2 * m:
                    assert tags[:-1].sum() == 0 and tried == 1                      # no interior position is eligible
                if m == 1:
                    assert (tags[:-1] == (q[:-1] > 0)).all()                        # the threshold rule
                tied += int(sum(1 for s in O.admissible_sets(n, m) if sum(int(q[t]) for t in s) == want) > 1)
                cases += 1
    assert cases >= 700 and tied >= 100, (cases, tied)


def test_fixed_point_is_the_threshold_rule_for_thresholds_from_2_to_the_minus_8():
    """for th in [2^-8, 1): q > 0 iff p > th (include/mts.h): T is exact, P is exact from 2^-8 up and at most 2^24 <= T below"""
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.random(4000).astype(np.float32), np.float32([0, 1, 2 ** -8, 2 ** -9, 2 ** -33, 3 * 2.0 ** -34, 0.5])])
    for th in [2.0 ** -8, 0.3, 0.5, float(np.nextafter(np.float32(1), np.float32(0))), float(p[17]), float(np.nextafter(p[17], np.float32(0)))]:
        th = float(np.float32(th))
        assert ((O.fixed_point(p, th) > 0) == (p > np.float32(th))).all(), th
    assert O.fixed_point(np.float32([2 ** -33, 3 * 2.0 ** -34, 2 ** -32]), 0.0).tolist() == [0, 1, 1]      # half to even: 0.5 -> 0, 0.75 -> 1


def test_segment_table_rule():
    tags = np.array([0, 1, 0, 0, 1, 0, 0, 0], dtype=np.uint8)
    ends, k = O.segment_table(tags, 7, True, 5)
    assert ends.tolist() == [2, 5, 7, -1, -1] and k == 3 and ends.dtype == np.int32        # the tail closes at the length
    ends, k = O.segment_table(tags, 7, False, 5)
    assert ends.tolist() == [2, 5, -1, -1, -1] and k == 2
    ends, k = O.segment_table(tags, 5, True, 5)                                            # ends on a boundary: no tail
    assert ends.tolist() == [2, 5, -1, -1, -1] and k == 2
    ends, k = O.segment_table(tags, 7, True, 2)                                            # clipped at Smax, the count is not
    assert ends.tolist() == [2, 5] and k == 3
    ends, k = O.segment_table(tags, 0, True, 3)                                            # an empty document
    assert ends.tolist() == [-1, -1, -1] and k == 0
    ends, k = O.segment_table(np.zeros(4, dtype=np.uint8), 4, True, 3)
    assert ends.tolist() == [4, -1, -1] and k == 1
    prob = np.float32([[0.9, 0.1, 0.9, 0.2, 0.7], [0.9, 0.9, 0.9, 0.9, 0.9]])
    tags, seg_end, n_seg = O.decode(prob, [5, 3], 0.5, 1, True, 4)
    assert tags.tolist() == [[1, 0, 1, 0, 1], [1, 1, 1, 0, 0]] and seg_end.tolist() == [[1, 3, 5, -1], [1, 2, 3, -1]] and n_seg.tolist() == [3, 3]
    tags, seg_end, n_seg = O.decode(prob, None, 0.5, 2, True, 4)                           # m = 2: interior positions 1 .. 2 only
    assert tags.tolist() == [[0, 0, 1, 0, 1], [0, 1, 0, 0, 1]] and n_seg.tolist() == [2, 2]


def test_entry_point_refuses_bad_arguments_before_any_device_work():
    """the checks of mts_segment_decode come before its launch, so they run without a GPU: 1 = MTS_ERR_INVALID, 2 = MTS_ERR_UNSUPPORTED"""
    from multimodaltopicsegmentation_amd import _lib as L

    def rc(B=1, Lq=8, n_out=1, th=0.5, m=1, Smax=4):
        return L.lib.mts_segment_decode(None, B, Lq, n_out, None, None, th, m, 1, Smax, None, None, None, None)
    assert rc(Lq=65537) == 2 and rc(m=1025) == 2 and rc(m=0) == 2
    assert rc(B=-1) == 1 and rc(Lq=0) == 1 and rc(Smax=0) == 1 and rc(n_out=0) == 1 and rc(n_out=5) == 1
    assert rc(m=2, th=float('nan')) == 1 and rc(m=2, th=2000.0) == 1
    assert rc() == 1                                                                       # null pointers with B > 0
    with pytest.raises(ValueError, match='null pointer'):
        L.check(rc())
    assert rc(B=0) == 0 and rc(B=0, m=1024, Lq=65536) == 0                                 # nothing to do: no launch
    with pytest.raises(NotImplementedError):
        L.check(rc(m=1025))


# ---- segment_audio against the reference's recorded spans -------------------------------------------------------------------------
def test_segment_audio_equals_the_reference_s_spans():
    from multimodaltopicsegmentation_amd import segment_audio
    g = np.load(os.path.join(GOLDEN, 'g23_segment_audio.npz'))
    raised = 0
    for i in range(int(g['cases'])):
        args = (int(g[f'n{i}']), g[f'flags{i}'].tolist())
        kw = dict(sr=int(g[f'sr{i}']), interval=float(g[f'interval{i}']), adaptive=bool(g[f'adaptive{i}']))
        if int(g[f'raises{i}']):
            with pytest.raises(IndexError):
                segment_audio(*args, **kw)
            raised += 1
            continue
        got = segment_audio(*args, **kw)
        assert got == [tuple(r) for r in g[f'spans{i}'].tolist()], i
        assert segment_audio(args[0], np.asarray(args[1], dtype=bool), **kw) == got           # an array of flags as well as a list
    assert raised == 2
    assert segment_audio(41, [0, 1, 0, 0, 1, 0, 0, 0, 0, 1], sr=4) == [(0, 8), (8, 20), (20, 40), (40, 41)]
    assert segment_audio(40, [0] * 9 + [1], sr=4)[-1] == (40, 40)                            # the uniform mode's empty tail, kept as upstream's
    assert segment_audio(1000, [0] * 99 + [1], adaptive=True) == [(0, 1000)] and segment_audio(1000, [0] * 100, adaptive=True) == []


# ---- Prediction -------------------------------------------------------------------------------------------------------------------
def _part(docs, ends, lengths, tags=None, names=None, **kw):
    from multimodaltopicsegmentation_amd import Prediction
    return Prediction(kw.get('threshold', 0.5), kw.get('min_segment', 1), kw.get('close_last', True), docs, names, lengths, ends, tags)


def test_merge_is_keyed_by_corpus_index_and_refuses_duplicates_and_gaps():
    from multimodaltopicsegmentation_amd import Prediction
    a = _part([0, 2, 4], [[2, 5], [3], [1, 4, 6]], [5, 3, 6], names=['a', 'c', 'e'], tags=[[0, 1, 0, 0, 0], [0, 0, 0], [1, 0, 0, 1, 0, 0]])
    b = _part([1, 3], [[7], [1, 2]], [7, 2], names=['b', 'd'], tags=[[0] * 7, [1, 0]])
    empty = _part([], [], [], names=[], tags=[])
    for parts in ([a, b], [b, a], [empty, b, a]):
        p = Prediction.merge(parts)
        assert p.documents.tolist() == [0, 1, 2, 3, 4] and p.documents.dtype == np.int64 and p.names == ['a', 'b', 'c', 'd', 'e']
        assert p.lengths.tolist() == [5, 7, 3, 2, 6] and p.n_segments.tolist() == [2, 1, 1, 2, 3]
        assert [e.tolist() for e in p.segment_ends] == [[2, 5], [7], [3], [1, 2], [1, 4, 6]] and all(e.dtype == np.int64 for e in p.segment_ends)
        assert [t.tolist() for t in p.tags] == [[0, 1, 0, 0, 0], [0] * 7, [0, 0, 0], [1, 0], [1, 0, 0, 1, 0, 0]] and p.probabilities is None
        assert (p.threshold, p.min_segment, p.close_last) == (0.5, 1, True)
    with pytest.raises(ValueError, match='more than once'):
        Prediction.merge([a, b, _part([3], [[2]], [2], names=['d'], tags=[[0, 0]])])
    with pytest.raises(ValueError, match='document 1 is missing'):
        Prediction.merge([a, _part([3], [[2]], [2], names=['d'], tags=[[0, 0]])])
    with pytest.raises(ValueError, match='settings'):
        Prediction.merge([a, _part([1, 3], [[7], [1, 2]], [7, 2], names=['b', 'd'], tags=[[0] * 7, [1, 0]], min_segment=3)])
    with pytest.raises(ValueError, match='tags'):
        Prediction.merge([a, _part([1, 3], [[7], [1, 2]], [7, 2], names=['b', 'd'])])
    with pytest.raises(ValueError):
        Prediction.merge([])
    with pytest.raises(ValueError):
        _part([0, 1], [[1]], [1, 1])


def test_spans_in_sentences_and_in_seconds():
    p = _part([0, 1, 2], [[2, 5], [], [3]], [5, 0, 4], close_last=False)
    assert p.spans() == [[(0, 2), (2, 5)], [], [(0, 3)]]
    times = [np.array([[0.0, 1.5], [1.5, 2.0], [2.5, 4.0], [4.0, 4.5], [5.0, 9.25]]), np.zeros((0, 2)), np.array([[1, 2], [2, 3], [3, 5], [5, 6]])]
    assert p.spans(times) == [[(0.0, 2.0), (2.5, 9.25)], [], [(1, 5)]]
    with pytest.raises(ValueError):
        p.spans([times[0][:4], times[1], times[2]])


def test_as_saturated_holds_the_tags_as_logits():
    p = _part([0, 1], [[2, 5], [1]], [5, 2], tags=[[0, 1, 0, 0, 0], [1, 0]])
    s = p.as_saturated('cpu')
    assert s.dtype == torch.float32 and tuple(s.shape) == (2, 5, 1)
    assert s[..., 0].tolist() == [[-30.0, 30.0, -30.0, -30.0, -30.0], [30.0, -30.0, -30.0, -30.0, -30.0]]
    with pytest.raises(ValueError, match='return_tags'):                                     # the tail hides the last sentence's tag
        _part([0], [[2, 5]], [5]).as_saturated('cpu')
    open_ended = _part([0, 1], [[2, 5], []], [5, 2], close_last=False).as_saturated('cpu')
    assert open_ended[..., 0].tolist() == [[-30.0, 30.0, -30.0, -30.0, 30.0], [-30.0] * 5]


# ---- the unlabelled corpus -----------------------------------------------------------------------------------------------------------
def test_from_documents_host_half_and_the_refusals():
    from multimodaltopicsegmentation_amd import ResidentCorpus, evaluate, fit
    g = torch.Generator().manual_seed(1)
    docs = [torch.randn(n, 6, generator=g) for n in (4, 1, 9, 2)]
    c = ResidentCorpus.from_documents(docs, 'cpu', names=['a.npy', 'b.npy', 'c.npy', 'd.npy'])
    assert c.labelled is False and c.names == ['a.npy', 'b.npy', 'c.npy', 'd.npy'] and len(c) == 4 and not c.truncate
    assert c.rows.tolist() == c.lengths.tolist() == [4, 1, 9, 2] and c.total_rows == 16
    assert torch.equal(c.corpus, torch.cat(docs)) and c.corpus2 is None and float(c.targets.abs().sum()) == 0 and c.targets.numel() == 16
    fields, Lmax = c.host_fields([2, 0, 3])
    assert Lmax == 9 and fields['id'].tolist() == [2, 0, 3] and fields['src_lengths'].tolist() == [9, 4, 2] and fields['domain'] is None
    assert fields['src_lengths'].dtype == torch.int64 and 'src_segments' not in fields
    assert c.host_fields([1], pad_to=5)[1] == 5
    two = ResidentCorpus.from_documents([d.numpy() for d in docs], 'cpu', wire_dtype='bf16', embeddings2=[d[:, :2] for d in docs], domain=[0, 1, 0, 1])
    assert two.names is None and two.corpus.dtype == torch.bfloat16 and tuple(two.corpus2.shape) == (16, 2)
    assert two.host_fields([3, 1])[0]['domain'] == [1, 1]
    assert ResidentCorpus.labelled is True                                                   # a corpus built the existing way
    for bad in (dict(names=['a']), dict(domain=[0]), dict(embeddings2=docs[:2])):
        with pytest.raises(ValueError):
            ResidentCorpus.from_documents(docs, 'cpu', **bad)
    with pytest.raises(ValueError):
        ResidentCorpus.from_documents([], 'cpu')
    with pytest.raises(ValueError):
        ResidentCorpus.from_documents([torch.zeros(6)], 'cpu')                               # a document that is no matrix
    with pytest.raises(ValueError, match='predict'):
        fit(None, c, batch_size=2, max_epochs=1)
    with pytest.raises(ValueError, match='predict'):
        evaluate(object(), c)
