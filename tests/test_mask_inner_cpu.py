"""Negative-sentence masking, the part that needs no GPU: the host half of MaskedCorpus (lengths, host_fields, src_segments, the epoch's
plan, the sampler's pad_to on two ranks) against the host oracle (tests/mask_oracle.py: the rule of include/mts.h mts_mask_plan, row by
row); draws that are SEEN to drop a document's first and last row and to trigger the empty-draw rule; the kept share of 100 000 negatives;
the refusals of mts_mask_plan and mts_gather_rows before any device work; arity of header, ctypes binding and ops wrappers."""
import inspect

import numpy as np
import pytest
import torch

from tests import mask_oracle as O
from tests.test_segment_augment_cpu import LABELS as SEGMENT_LABELS, TV, _dataset

# the documents of the segment-order tests (1, 7, 5, 4, 37 and 300 rows), a 5-row one without a boundary and one whose first and last
# rows are negatives
LABELS = SEGMENT_LABELS + [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 1, 0]]
N = len(LABELS)
ALL_NEGATIVE, EDGES = N - 2, N - 1
PS = [0.0, 0.25, 0.5, 0.9, 1.0]


def _seen(seed):
    """the two draws the tests must see at this view seed, epoch 0: p = 0.5 drops the first and the last row of EDGES; p = 0.25 drops every
    row of ALL_NEGATIVE (so that the empty-draw rule is what keeps its row 0)"""
    edges = O.kept_rows(LABELS[EDGES], O.doc_seed(seed, 0, N, EDGES), 0.5)
    T = O.threshold(0.25)
    h = O.hash32(O.doc_seed(seed, 0, N, ALL_NEGATIVE), list(range(5)))
    return 0 not in edges and 6 not in edges and all(int(v) >= T for v in h)


SEED = next(s for s in range(1000) if _seen(s))                      # deterministic: the smallest seed that shows both


def _corpus(truncate=False, labels=LABELS, **kw):
    from multimodaltopicsegmentation_amd import ResidentCorpus
    return ResidentCorpus(_dataset(truncate, labels=labels, **kw), 'cpu')


def _want(p, epoch, truncate, seed=SEED, labels=LABELS):
    """per document: (kept rows, reported length, src_segments) from the oracle"""
    out = []
    for d, y in enumerate(labels):
        rows = O.kept_rows(y, O.doc_seed(seed, epoch, len(labels), d), p)
        length = min(len(rows), TV) if truncate else len(rows)
        out.append((rows, length, O.segments([y[r] for r in rows], length)))
    return out


def test_the_searched_seed_shows_both_draws():
    assert _seen(SEED)
    edges = O.kept_rows(LABELS[EDGES], O.doc_seed(SEED, 0, N, EDGES), 0.5)
    assert edges[0] > 0 and edges[-1] < 6 and {2, 5} <= set(edges)     # the boundaries stay, the first and the last row went
    assert O.kept_rows(LABELS[ALL_NEGATIVE], O.doc_seed(SEED, 0, N, ALL_NEGATIVE), 0.25) == [0]      # kept by the empty-draw rule alone
    view = _corpus().masked(0.5, seed=SEED)
    assert view.kept_rows(EDGES).tolist() == edges
    view = _corpus().masked(0.25, seed=SEED)
    assert view.kept_rows(ALL_NEGATIVE).tolist() == [0] and int(view.rows[ALL_NEGATIVE]) == 1


@pytest.mark.parametrize('truncate', [False, True])
@pytest.mark.parametrize('p', PS)
def test_lengths_host_fields_and_segments_equal_the_oracle(p, truncate):
    from multimodaltopicsegmentation_amd import MaskedCorpus
    rc = _corpus(truncate, second=True, domain_adapt=True, segments=True)
    view = rc.masked(p, seed=SEED)
    assert isinstance(view, MaskedCorpus) and len(view) == N == len(rc)
    for epoch in (0, 1):
        view.set_epoch(epoch)
        want = _want(p, epoch, truncate)
        assert view.rows.tolist() == [len(w[0]) for w in want] and view.lengths.tolist() == [w[1] for w in want]
        assert [view.kept_rows(d).tolist() for d in range(N)] == [w[0] for w in want]
        seeds = [O.doc_seed(SEED, epoch, N, d) for d in range(N)]
        assert [int(v) for v in view.doc_seeds] == seeds
        for idx in (list(range(N)), [5, 5, 0, 7], [6], [4, 1, 7, 2]):
            got, Lmax = view.host_fields(idx)
            assert Lmax == (TV if truncate else max(len(want[d][0]) for d in idx))
            assert got['id'].tolist() == idx and got['id'].dtype == torch.int64
            assert got['src_lengths'].dtype == torch.int64 and got['src_lengths'].tolist() == [want[d][1] for d in idx]
            assert got['src_segments'] == [want[d][2] for d in idx]
            assert got['domain'] == [rc.domain[d] for d in idx]
            assert set(got) == {'id', 'src_lengths', 'domain', 'src_segments'}
    assert view.host_fields([]) == ({}, 0) and view.batch([]) == {}
    if truncate:
        with pytest.raises(ValueError):
            view.host_fields([1, 2], pad_to=TV)
    else:
        longest = max(int(view.rows[1]), int(view.rows[2]))
        assert view.host_fields([1, 2], pad_to=longest + 3)[1] == longest + 3
        with pytest.raises(ValueError):
            view.host_fields([1, 5], pad_to=int(view.rows[5]) - 1)
    for bad in ([N], [-1]):
        with pytest.raises(IndexError):
            view.host_fields(bad)
    with pytest.raises(RuntimeError):
        view.batch([1, 2])                                             # valid: only now does the missing GPU matter


@pytest.mark.parametrize('truncate', [False, True])
def test_probability_one_is_the_corpus_and_zero_keeps_the_boundaries(truncate):
    rc = _corpus(truncate, domain_adapt=True, segments=True)
    everything, nothing = rc.masked(1.0, seed=SEED), rc.masked(0.0, seed=SEED)
    for epoch in (0, 1):
        everything.set_epoch(epoch)
        nothing.set_epoch(epoch)
        for idx in (list(range(N)), [7, 0, 5, 5]):
            a, b = everything.host_fields(idx), rc.host_fields(idx)
            assert a[1] == b[1] and set(a[0]) == set(b[0])
            assert torch.equal(a[0]['id'], b[0]['id']) and torch.equal(a[0]['src_lengths'], b[0]['src_lengths'])
            assert a[0]['src_segments'] == b[0]['src_segments'] and a[0]['domain'] == b[0]['domain']
        assert everything.lengths.tolist() == rc.lengths.tolist() and everything.rows.tolist() == rc.rows.tolist()
        for d, y in enumerate(LABELS):
            ones = [r for r, v in enumerate(y) if v == 1]
            assert nothing.kept_rows(d).tolist() == (ones or [0])       # the boundary rows; row 0 of a document without one
    assert nothing.kept_rows(ALL_NEGATIVE).tolist() == [0] and nothing.kept_rows(3).tolist() == [0] and nothing.kept_rows(0).tolist() == [0]


def test_epochs_differ_and_the_plan_is_kept_until_the_epoch_changes():
    view = _corpus().masked(0.5, seed=SEED)
    first = [view.kept_rows(d).tolist() for d in range(N)]
    held = view._kept_rel
    view.set_epoch(0)
    assert view._kept_rel is held                                        # the same epoch: the cached plan, not a new pass
    view.set_epoch(1)
    second = [view.kept_rows(d).tolist() for d in range(N)]
    assert first != second and first[5] != second[5]
    assert second == [w[0] for w in _want(0.5, 1, False)]
    view.set_epoch(0)
    assert [view.kept_rows(d).tolist() for d in range(N)] == first       # a draw hangs on (seed, epoch, document) alone
    other = _corpus().masked(0.5, seed=SEED + 1)
    assert [other.kept_rows(d).tolist() for d in range(N)] != first


def test_two_ranks_make_the_same_plan_and_pad_alike():
    from multimodaltopicsegmentation_amd import DocumentShardSampler
    views = [_corpus().masked(0.5, seed=SEED) for _ in range(2)]
    samplers = [v.sampler(4, rank=r, world=2, seed=SEED) for r, v in enumerate(views)]
    assert all(isinstance(s, DocumentShardSampler) and len(s) == 2 for s in samplers)
    pads = []
    for epoch in (0, 1, 2):
        for s in samplers:
            s.set_epoch(epoch)
        assert [v.epoch for v in views] == [epoch, epoch]
        assert np.array_equal(views[0]._kept_rel, views[1]._kept_rel) and np.array_equal(views[0].rows, views[1].rows)
        assert np.array_equal(views[0].doc_seeds, views[1].doc_seeds)
        want = _want(0.5, epoch, False)
        seen = 0
        for (ix0, pad0), (ix1, pad1), g in zip(samplers[0], samplers[1], samplers[0].global_batches()):
            assert sorted(ix0 + ix1) == sorted(g.tolist()) and ix0 == g[0::2].tolist() and ix1 == g[1::2].tolist()
            assert pad0 == pad1 == max(len(want[d][0]) for d in g.tolist())       # the longest MASKED document of the global batch
            assert views[0].host_fields(ix0, pad0)[1] == views[1].host_fields(ix1, pad1)[1] == pad0
            pads.append(pad0)
            seen += 1
        assert seen == 2
    assert max(pads) < 300                                               # the 300-row document never went through unmasked
    # with truncate=True every batch is truncate_value long: the sampler hands out no pad_to
    assert all(pad is None for _, pad in _corpus(True).masked(0.5).sampler(4))


def test_kept_share_of_100000_negatives():
    """p = 0.9: the kept share lies within 4 sigma of 0.9, sigma = sqrt(p (1 - p) / n) = 0.00095"""
    n, p = 100000, 0.9
    labels = [[0] * n]
    rc = _corpus(labels=labels, D=1)
    view = rc.masked(p, seed=0)
    kept = view.kept_rows(0).tolist()
    assert kept == O.kept_rows(labels[0], O.doc_seed(0, 0, 1, 0), p)
    share = len(kept) / n
    sigma = (p * (1 - p) / n) ** 0.5
    print(f'kept share {share:.5f}, {abs(share - p) / sigma:.2f} sigma from {p}')
    assert abs(share - p) < 4 * sigma


def test_header_binding_and_wrappers_agree_on_the_two_symbols():
    from multimodaltopicsegmentation_amd import _lib as L, ops
    from tests.test_abi import _declared
    decl = _declared()
    assert decl['mts_mask_plan'] == 11 == len(L.SIGNATURES['mts_mask_plan'][1])
    assert decl['mts_gather_rows'] == 13 == len(L.SIGNATURES['mts_gather_rows'][1]) == decl['mts_gather_pad'] + 1
    assert L.lib.mts_mask_plan.argtypes == L.SIGNATURES['mts_mask_plan'][1] and L.lib.mts_gather_rows.argtypes == L.SIGNATURES['mts_gather_rows'][1]
    assert list(inspect.signature(ops.mask_plan).parameters) == ['targets', 'row_start', 'doc_index', 'doc_seed', 'keep_probability', 'src_row', 'kept']
    assert list(inspect.signature(ops.gather_rows).parameters) == ['corpus', 'row_start', 'doc_index', 'src_row', 'dst', 'pad_value']


def test_argument_errors_come_back_before_any_device_work():
    from multimodaltopicsegmentation_amd import _lib as L
    p = 4096                                                        # stands for a device address: never dereferenced by a refused call
    ok = dict(B=2, Lmax=3, targets=p, row_start=p, n_docs=1, doc_index=p, doc_seed=p, keep=0.5, src_row=p, kept=p)

    def plan(**kw):
        a = dict(ok, **kw)
        return L.lib.mts_mask_plan(None, a['B'], a['Lmax'], a['targets'], a['row_start'], a['n_docs'], a['doc_index'], a['doc_seed'], a['keep'],
                                   a['src_row'], a['kept'])
    for bad in (dict(B=-1), dict(Lmax=0), dict(n_docs=0), dict(keep=-0.001), dict(keep=1.001), dict(keep=float('nan')), dict(keep=float('inf')),
                dict(targets=None), dict(row_start=None), dict(doc_index=None), dict(doc_seed=None), dict(src_row=None), dict(kept=None)):
        assert plan(**bad) == 1, bad                                   # MTS_ERR_INVALID
        assert b'mts_mask_plan' in L.lib.mts_last_error()
    assert plan(B=0) == 0 and plan(B=0, targets=None, row_start=None, doc_index=None, doc_seed=None, src_row=None, kept=None) == 0
    assert plan(B=0, keep=2.0) == 1 and plan(B=0, Lmax=0) == 1        # the checks come before the early return

    ok = dict(src=L.F32, dst=L.F32, B=2, Lmax=3, D=4, corpus=p, row_start=p, n_docs=1, doc_index=p, src_row=p, out=p)

    def rows(**kw):
        a = dict(ok, **kw)
        return L.lib.mts_gather_rows(None, a['src'], a['dst'], a['B'], a['Lmax'], a['D'], a['corpus'], a['row_start'], a['n_docs'], a['doc_index'],
                                     a['src_row'], a['out'], 0.0)
    for bad in (dict(corpus=None), dict(row_start=None), dict(doc_index=None), dict(src_row=None), dict(out=None), dict(B=-1), dict(Lmax=0),
                dict(D=0), dict(n_docs=0), dict(src=2), dict(dst=-1), dict(corpus=p + 2)):
        assert rows(**bad) == 1, bad
        assert b'mts_gather_rows' in L.lib.mts_last_error()
    assert rows(src=L.BF16, dst=L.F32) == 2                            # MTS_ERR_UNSUPPORTED, as mts_gather_pad
    assert rows(B=0) == 0 and rows(B=0, corpus=None, row_start=None, doc_index=None, src_row=None, out=None) == 0


def test_refusals_of_the_python_layer():
    from multimodaltopicsegmentation_amd import fit
    rc = _corpus()
    for bad in (1.5, -0.1, float('nan')):
        with pytest.raises(ValueError):
            rc.masked(bad)
        with pytest.raises(ValueError):
            rc.batch_masked([1], [7], bad)
    with pytest.raises(ValueError):
        fit(None, rc, batch_size=4, max_epochs=1, mask_inner=0.5, augment='shuffle')      # refused before the trainer is looked at
    with pytest.raises(ValueError):
        rc.batch_masked([1, 2], [7], 0.5)                              # one seed per listed document
    with pytest.raises(ValueError):
        rc.batch_masked([1, 2], [7, 8], 1.0, pad_to=6)                 # below the longest masked document (7 rows at p = 1)
    with pytest.raises(IndexError):
        rc.batch_masked([N], [7], 0.5)
    with pytest.raises(RuntimeError):
        rc.batch_masked([1, 2], [7, 2 ** 64 - 1], 0.5)                 # valid: only now does the missing GPU matter
    assert rc.batch_masked([], [], 0.5) == {}
