"""resident.ResidentCorpus / DocumentShardSampler and the C ABI of mts_gather_pad, the part that needs no GPU: arity of header, ctypes
binding and ops wrapper; argument errors reported before any device work; the host half of a resident batch against the reference
collater (EncoderDataset.py:91-152); the sampler's sharding rules."""
import inspect
import itertools

import numpy as np
import pytest
import torch

LENGTHS = [1, 7, 13, 4, 9, 2]            # a length-1 document, and 13 > TV: one longer than truncate_value
TV = 8


def _lines(lengths=LENGTHS, D=6, seed=0, boundary_p=0.4):
    g = torch.Generator().manual_seed(seed)
    names = ['3fm_news.wav', 'show_a.wav', '9am.wav', 'talk.wav', 'evening.wav', '1live.wav']
    lines = []
    for k, n in enumerate(lengths):
        tgt = (torch.rand(n, generator=g) < boundary_p).float().tolist()
        lines.append((torch.randn(n, D, generator=g), tgt, names[k % len(names)]))
    return lines


def _dataset(truncate, crf=False, domain_adapt=False, segments=False, second=False, lengths=LENGTHS, **kw):
    from multimodaltopicsegmentation_amd import AudioPortionDataset
    second_input = _lines(lengths, D=4, seed=1) if second else None
    return AudioPortionDataset(_lines(lengths), {'O': 0, 'B': 1}, CRF=crf, truncate=truncate, truncate_value=TV, second_input=second_input,
                               domain_adapt=domain_adapt, segments=segments, **kw)


def test_header_binding_and_wrapper_agree_on_mts_gather_pad():
    from multimodaltopicsegmentation_amd import _lib as L, ops
    from tests.test_abi import _declared
    decl = _declared()
    assert decl['mts_gather_pad'] == 12 == len(L.SIGNATURES['mts_gather_pad'][1])
    assert L.lib.mts_gather_pad.argtypes == L.SIGNATURES['mts_gather_pad'][1]
    # the wrapper derives stream, dtypes, B, Lmax, D and n_docs from its tensors: five tensor-or-scalar arguments remain
    assert list(inspect.signature(ops.gather_pad).parameters) == ['corpus', 'row_start', 'doc_index', 'dst', 'pad_value']


def test_argument_errors_come_back_before_any_device_work():
    from multimodaltopicsegmentation_amd import _lib as L
    p = 4096                                                        # stands for a device address: never dereferenced by a refused call
    ok = dict(src=L.F32, dst=L.F32, B=2, Lmax=3, D=4, corpus=p, row_start=p, n_docs=1, doc_index=p, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.lib.mts_gather_pad(None, a['src'], a['dst'], a['B'], a['Lmax'], a['D'], a['corpus'], a['row_start'], a['n_docs'], a['doc_index'],
                                    a['out'], 0.0)
    for bad in (dict(corpus=None), dict(row_start=None), dict(doc_index=None), dict(out=None), dict(B=-1), dict(Lmax=0), dict(D=0),
                dict(n_docs=0), dict(src=2), dict(dst=-1), dict(src=7, dst=7)):
        assert call(**bad) == 1, bad                                   # MTS_ERR_INVALID
        assert b'mts_gather_pad' in L.lib.mts_last_error()
        with pytest.raises(ValueError):
            L.check(1)
    assert call(src=L.BF16, dst=L.F32) == 2                            # MTS_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        L.check(2)
    assert call(B=0) == 0                                              # nothing to gather: no launch
    assert call(B=0, corpus=None, row_start=None, doc_index=None, out=None) == 0


CASES = [[0, 1, 2, 3, 4, 5], [2], [0], [5, 5, 0, 2, 2], [4, 3]]


@pytest.mark.parametrize('truncate,crf,domain_adapt', list(itertools.product([True, False], repeat=3)))
def test_host_fields_equal_the_reference_collater(truncate, crf, domain_adapt):
    from multimodaltopicsegmentation_amd import ResidentCorpus
    ds = _dataset(truncate, crf=crf, domain_adapt=domain_adapt, segments=True, second=True)
    rc = ResidentCorpus(ds, 'cpu')
    assert len(rc) == len(LENGTHS) and rc.nbytes == sum(LENGTHS) * (6 + 4 + 1) * 4 + (len(LENGTHS) + 1) * 8
    for idx in CASES:
        ref = ds.collater([ds[i] for i in idx])
        got, Lmax = rc.host_fields(idx)
        assert Lmax == ref['src_tokens'].shape[1] == ref['tgt_tokens'].shape[1]
        assert got['src_lengths'].dtype == torch.int64 and torch.equal(got['src_lengths'], ref['src_lengths'])
        assert got['id'].dtype == ref['id'].dtype and torch.equal(got['id'], ref['id'])
        assert got['domain'] == ref['domain'] and (got['domain'] is None) == (not domain_adapt)
        assert got['src_segments'] == ref['src_segments']
        assert set(got) == {'id', 'src_lengths', 'domain', 'src_segments'}
    assert any(s for s in rc.host_fields(CASES[0])[0]['src_segments'])           # the fixture does have boundaries
    assert rc.host_fields([]) == ({}, 0) and rc.batch([]) == {} == ds.collater([])


def test_segments_follow_the_dataset_unless_overridden():
    from multimodaltopicsegmentation_amd import ResidentCorpus
    assert 'src_segments' not in ResidentCorpus(_dataset(False), 'cpu').host_fields([0, 1])[0]
    assert 'src_segments' in ResidentCorpus(_dataset(False), 'cpu', segments=True).host_fields([0, 1])[0]
    assert 'src_segments' not in ResidentCorpus(_dataset(False, segments=True), 'cpu', segments=False).host_fields([0, 1])[0]


def test_wire_dtype_defaults_to_the_datasets():
    from multimodaltopicsegmentation_amd import ResidentCorpus
    ds = _dataset(False)
    assert ResidentCorpus(ds, 'cpu').corpus.dtype == torch.float32
    assert ResidentCorpus(ds, 'cpu', wire_dtype='bf16').corpus.dtype == torch.bfloat16
    ds16 = _dataset(False, wire_dtype='bf16')
    rc16 = ResidentCorpus(ds16, 'cpu')
    assert rc16.corpus.dtype == torch.bfloat16 and rc16.targets.dtype == torch.float32
    assert torch.equal(rc16.corpus, torch.cat([line[0] for line in _lines()]).to(torch.bfloat16))
    with pytest.raises(ValueError):
        ResidentCorpus(ds, 'cpu', wire_dtype='fp16')


def test_pad_to_and_index_refusals():
    from multimodaltopicsegmentation_amd import AudioPortionDataset, ResidentCorpus
    rc = ResidentCorpus(_dataset(False), 'cpu')
    assert rc.host_fields([0, 1], pad_to=7)[1] == 7 and rc.host_fields([0, 1], pad_to=20)[1] == 20 and rc.host_fields([0, 1])[1] == 7
    with pytest.raises(ValueError):
        rc.host_fields([0, 1], pad_to=6)                               # below the longest listed document
    with pytest.raises(ValueError):
        rc.batch([0, 2], pad_to=12)
    rt = ResidentCorpus(_dataset(True), 'cpu')
    assert rt.host_fields([0, 2])[1] == TV
    with pytest.raises(ValueError):
        rt.host_fields([0, 2], pad_to=TV)                              # truncate=True fixes the length
    for bad in ([6], [-1], [0, 99]):
        with pytest.raises(IndexError):
            rc.host_fields(bad)
        with pytest.raises(IndexError):
            rc.batch(bad)
    lines = _lines()
    lines[3] = (torch.randn(4, 5), lines[3][1], lines[3][2])           # one document of another width
    with pytest.raises(ValueError):
        ResidentCorpus(AudioPortionDataset(lines, {}, truncate=False), 'cpu')


# ---- the sampler ------------------------------------------------------------------------------------------------------------

def _ranks(lengths, batch, world, **kw):
    from multimodaltopicsegmentation_amd import DocumentShardSampler
    return [DocumentShardSampler(lengths, batch, rank=r, world=world, **kw) for r in range(world)]


def test_ranks_partition_every_global_batch_and_pad_alike():
    lengths = np.array([5, 9, 2, 14, 7, 3, 11, 8, 6, 4, 10])
    for world in (1, 2, 3):
        ss = _ranks(lengths, 4, world, seed=3)
        assert len({len(s) for s in ss}) == 1 and len(ss[0]) == 3
        steps = [list(s) for s in ss]
        assert all(len(st) == len(ss[0]) for st in steps)
        seen = []
        for k, g in enumerate(ss[0].global_batches()):
            local = [steps[r][k][0] for r in range(world)]
            assert all(local[r] == g[r::world].tolist() for r in range(world))           # the rule of trainer.shard_batch
            flat = [i for part in local for i in part]
            assert sorted(flat) == sorted(g.tolist()) and len(set(flat)) == len(flat)    # union = the global batch, ranks disjoint
            assert all(len(part) >= 1 for part in local)
            assert {steps[r][k][1] for r in range(world)} == {int(lengths[g].max())}     # one pad_to, the global batch's longest
            seen += flat
        assert sorted(seen) == list(range(11)) and ss[0].dropped_documents == 0


def test_seed_and_epoch_change_the_permutation_and_ranks_agree():
    from multimodaltopicsegmentation_amd import DocumentShardSampler
    n = 40
    a, b = DocumentShardSampler(n, 8, rank=0, world=2, seed=1), DocumentShardSampler(n, 8, rank=1, world=2, seed=1)
    assert np.array_equal(a.permutation(), b.permutation()) and sorted(a.permutation().tolist()) == list(range(n))
    p0 = a.permutation()
    assert np.array_equal(p0, a.permutation())                                           # iterating twice in one epoch: the same order
    a.set_epoch(1)
    assert not np.array_equal(p0, a.permutation())
    b.set_epoch(1)
    assert np.array_equal(a.permutation(), b.permutation())
    assert not np.array_equal(p0, DocumentShardSampler(n, 8, seed=2).permutation())
    assert DocumentShardSampler(n, 8, shuffle=False).permutation().tolist() == list(range(n))
    assert all(pad is None for _, pad in a)                                              # built from a document count: no pad_to


def test_remainder_policy_and_dropped_documents():
    # 11 documents, global batch 4, three ranks: 4 + 4 + 3 -- the remainder still gives every rank a document and is kept
    ss = _ranks(np.arange(1, 12), 4, 3)
    assert [len(s) for s in ss] == [3, 3, 3] and all(s.dropped_documents == 0 for s in ss)
    assert [[len(ix) for ix, _ in s] for s in ss] == [[2, 2, 1], [1, 1, 1], [1, 1, 1]]
    ss = _ranks(np.arange(1, 12), 4, 3, drop_last=True)
    assert [len(s) for s in ss] == [2, 2, 2] and all(len(list(s)) == 2 for s in ss) and all(s.dropped_documents == 0 for s in ss)
    # 10 documents: the remainder of 2 cannot feed three ranks -- dropped on every rank, and counted
    ss = _ranks(np.arange(1, 11), 4, 3)
    assert [len(s) for s in ss] == [2, 2, 2] and all(len(list(s)) == 2 for s in ss) and all(s.dropped_documents == 2 for s in ss)
    # a global batch smaller than the world leaves nothing to step on
    ss = _ranks(np.arange(1, 12), 2, 3)
    assert all(len(s) == 0 and list(s) == [] and s.dropped_documents == 11 for s in ss)
    from multimodaltopicsegmentation_amd import DocumentShardSampler
    for bad in (dict(rank=3, world=3), dict(rank=-1, world=2), dict(world=0)):
        with pytest.raises(ValueError):
            DocumentShardSampler(11, 4, **bad)
    with pytest.raises(ValueError):
        DocumentShardSampler(11, 0)


def test_world_one_is_a_plain_batch_sampler():
    from multimodaltopicsegmentation_amd import DocumentShardSampler
    lengths = np.array([5, 9, 2, 14, 7, 3, 11])
    s = DocumentShardSampler(lengths, 3, shuffle=False)
    assert list(s) == [([0, 1, 2], 9), ([3, 4, 5], 14), ([6], 11)] and len(s) == 3 and s.dropped_documents == 0
    assert list(DocumentShardSampler(lengths, 3, shuffle=False, drop_last=True)) == [([0, 1, 2], 9), ([3, 4, 5], 14)]


def test_corpus_makes_its_own_sampler():
    from multimodaltopicsegmentation_amd import ResidentCorpus
    rc = ResidentCorpus(_dataset(False), 'cpu')
    for ix, pad in rc.sampler(4, rank=1, world=2, seed=5):
        assert rc.host_fields(ix, pad)[1] == pad >= max(LENGTHS[i] for i in ix)
    rt = ResidentCorpus(_dataset(True), 'cpu')
    assert all(pad is None and rt.host_fields(ix, pad)[1] == TV for ix, pad in rt.sampler(4, rank=0, world=2))
