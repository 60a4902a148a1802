"""Segment-order augmentation, the part that needs no GPU: the host oracle (tests/segment_augment_oracle.py) against the reference's own
twins (tests/golden/g22_segment_augment.npz: cross_validation_split(inverse_augmentation=True), utils/load_datasets_precomputed.py:71-96);
ResidentCorpus.n_segments, the host half of AugmentedCorpus (lengths, host_fields, the orders of both modes, the sampler's epoch) against
the oracle; the refusals of batch_segments; arity of header, ctypes binding and ops wrapper of mts_gather_segments."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import segment_augment_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g22_segment_augment.npz')

# one row; two boundaries and a tail; every row but the last a boundary; no boundary; segments of 1, 2, 3, 5, 9 rows and a tail of 17 (their
# edges fall in every phase of a group of four rows); boundaries on rows 0 and 298 of 300 (segments of 1, 298 and 1 rows)
LABELS = [[0], [0, 0, 1, 0, 1, 0, 0], [1, 1, 1, 1, 0], [0, 0, 0, 0],
          [1 if t in (0, 2, 5, 10, 19) else 0 for t in range(37)], [1 if t in (0, 298) else 0 for t in range(300)]]
NAMES = ['3fm_news.wav', 'show_a.wav', '9am.wav', 'talk.wav', 'evening.wav', '1live.wav']
TV = 6                                                     # truncate_value: below most augmented lengths
SEED = 3


def _lines(D, seed, labels=LABELS):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(len(y), D, generator=g), [float(v) for v in y], NAMES[k % len(NAMES)]) for k, y in enumerate(labels)]


def _dataset(truncate, D=6, second=False, labels=LABELS, **kw):
    from multimodaltopicsegmentation_amd import AudioPortionDataset
    return AudioPortionDataset(_lines(D, 0, labels), {'O': 0, 'B': 1}, CRF=False, truncate=truncate, truncate_value=TV,
                               second_input=_lines(4, 1, labels) if second else None, **kw)


def test_the_oracle_reproduces_the_references_twins():
    z = np.load(GOLDEN)
    n = sum(1 for k in z.files if k.startswith('emb'))
    assert n == 6 and int(z['train_len']) == n + 11                 # the upstream loop ran on into its own twins; not reproduced here
    empty = 0
    for i in range(n):
        emb, lab = torch.from_numpy(z[f'emb{i}']), z[f'lab{i}'].tolist()
        order, close_last = O.reverse_rule(lab)
        got_emb, got_lab = O.augment_document(emb, lab, order, close_last)
        if 1 in lab:
            assert torch.equal(got_emb, torch.from_numpy(z[f'twin_emb{i}'])), i
            assert got_lab.tolist() == z[f'twin_lab{i}'].tolist() and close_last, i
        else:
            # deviation: upstream makes an EMPTY twin of a document without a boundary; the product's rule keeps the document
            empty += 1
            assert z[f'twin_emb{i}'].size == 0 and z[f'twin_lab{i}'].size == 0
            assert (order, close_last) == ([0], False)
            assert torch.equal(got_emb, emb) and got_lab.tolist() == lab
        # every segment in place is the document itself
        same_emb, same_lab = O.augment_document(emb, lab, *O.identity_rule(lab))
        assert torch.equal(same_emb, emb) and same_lab.tolist() == lab
    assert empty == 2                                                # the one-row and the no-boundary document


def test_n_segments_counts_the_labels():
    from multimodaltopicsegmentation_amd import ResidentCorpus
    labels = LABELS + [[0, 1, 0, 1]]                                 # one without a tail
    rc = ResidentCorpus(_dataset(False, labels=labels), 'cpu')
    want = [sum(y) + (0 if y[-1] == 1 else 1) for y in labels]
    assert isinstance(rc.n_segments, np.ndarray) and rc.n_segments.tolist() == want == [len(O.segment_ends(y)) for y in labels]
    assert want == [1, 3, 5, 1, 6, 3, 2]


def test_header_binding_and_wrapper_agree_on_mts_gather_segments():
    from multimodaltopicsegmentation_amd import _lib as L, ops
    from tests.test_abi import _declared
    decl = _declared()
    assert decl['mts_gather_segments'] == 18 == len(L.SIGNATURES['mts_gather_segments'][1]) == decl['mts_gather_pad'] + 6
    assert L.lib.mts_gather_segments.argtypes == L.SIGNATURES['mts_gather_segments'][1]
    assert list(inspect.signature(ops.gather_segments).parameters) == ['corpus', 'row_start', 'doc_index', 'seg_ptr', 'seg_dst', 'seg_src',
                                                                       'dst_len', 'dst', 'pad_value', 'close_last']


def test_argument_errors_come_back_before_any_device_work():
    from multimodaltopicsegmentation_amd import _lib as L
    p = 4096                                                        # stands for a device address: never dereferenced by a refused call
    ok = dict(src=L.F32, dst=L.F32, B=2, Lmax=3, D=1, corpus=p, row_start=p, n_docs=1, doc_index=p, seg_ptr=p, seg_dst=p, seg_src=p,
              n_listed=2, dst_len=p, close_last=p, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.lib.mts_gather_segments(None, a['src'], a['dst'], a['B'], a['Lmax'], a['D'], a['corpus'], a['row_start'], a['n_docs'],
                                         a['doc_index'], a['seg_ptr'], a['seg_dst'], a['seg_src'], a['n_listed'], a['dst_len'], a['close_last'],
                                         a['out'], 0.0)
    for bad in (dict(corpus=None), dict(row_start=None), dict(doc_index=None), dict(out=None), dict(seg_ptr=None), dict(seg_dst=None),
                dict(seg_src=None), dict(dst_len=None), dict(B=-1), dict(Lmax=0), dict(D=0), dict(n_docs=0), dict(n_listed=-1), dict(src=2),
                dict(dst=-1), dict(D=2), dict(src=L.BF16, dst=L.BF16), dict(src=L.F32, dst=L.BF16)):      # the label rule: D = 1 in fp32
        assert call(**bad) == 1, bad                                   # MTS_ERR_INVALID
        assert b'mts_gather_segments' in L.lib.mts_last_error()
    assert call(src=L.BF16, dst=L.F32, close_last=None) == 2           # MTS_ERR_UNSUPPORTED, as mts_gather_pad
    assert call(B=0) == 0 and call(B=0, corpus=None, row_start=None, doc_index=None, seg_ptr=None, dst_len=None, out=None) == 0


@pytest.mark.parametrize('truncate', [True, False])
@pytest.mark.parametrize('mode', ['reverse', 'shuffle'])
def test_host_fields_and_lengths_equal_the_oracle(mode, truncate):
    from multimodaltopicsegmentation_amd import AugmentedCorpus, ResidentCorpus
    rc = ResidentCorpus(_dataset(truncate, second=True, domain_adapt=True, segments=True), 'cpu')
    view = rc.augmented(mode, seed=SEED)
    n = len(LABELS)
    assert isinstance(view, AugmentedCorpus) and len(view) == 2 * n and len(rc) == n
    view.set_epoch(4)
    want_len, want_seg = [], []
    for v in range(2 * n):
        d = v % n
        y = LABELS[d]
        rule = O.identity_rule(y) if v < n else O.reverse_rule(y) if mode == 'reverse' else O.shuffle_rule(y, SEED, 4, d)
        _, lab = O.augment_document(torch.zeros(len(y), 1), y, *rule)
        length = min(len(lab), TV) if truncate else len(lab)
        want_len.append(length)
        want_seg.append(O.augmented_segments(lab, length))
    assert view.lengths.tolist() == want_len                          # known without drawing an order
    if mode == 'shuffle':
        assert view.lengths[n:].tolist() == view.lengths[:n].tolist()
    else:
        assert [int(r) for r in view.rows[n:]] == [1, 5, 4, 4, 20, 299]
    for idx in ([0, 1, 2, 3, 4, 5], list(range(n, 2 * n)), [7, 1, 10, 10, 4], [11], [6, 9, 0]):
        got, Lmax = view.host_fields(idx)
        assert Lmax == (TV if truncate else max(int(view.rows[v]) for v in idx))
        assert got['id'].tolist() == idx and got['id'].dtype == torch.int64
        assert got['src_lengths'].dtype == torch.int64 and got['src_lengths'].tolist() == [want_len[v] for v in idx]
        assert got['src_segments'] == [want_seg[v] for v in idx]
        assert got['domain'] == [rc.domain[v % n] for v in idx] and set(got['domain']) <= {0, 1}
        assert set(got) == {'id', 'src_lengths', 'domain', 'src_segments'}
    # stored documents alone: the corpus' own host fields
    a, b = view.host_fields([2, 0, 5]), rc.host_fields([2, 0, 5])
    assert a[1] == b[1] and a[0]['src_segments'] == b[0]['src_segments'] and torch.equal(a[0]['src_lengths'], b[0]['src_lengths'])
    assert view.host_fields([]) == ({}, 0) and view.batch([]) == {}
    if not truncate:
        assert view.host_fields([7, 1], pad_to=9)[1] == 9
        with pytest.raises(ValueError):
            view.host_fields([1, 10], pad_to=19 if mode == 'reverse' else 36)
    else:
        with pytest.raises(ValueError):
            view.host_fields([7, 1], pad_to=TV)
    for bad in ([2 * n], [-1]):
        with pytest.raises(IndexError):
            view.host_fields(bad)


def test_shuffle_orders_agree_between_ranks_and_change_with_the_epoch():
    from multimodaltopicsegmentation_amd import DocumentShardSampler, ResidentCorpus
    n = len(LABELS)
    views = [ResidentCorpus(_dataset(False), 'cpu').augmented('shuffle', seed=SEED) for _ in range(2)]
    samplers = [v.sampler(4, rank=r, world=2, seed=SEED) for r, v in enumerate(views)]
    assert all(isinstance(s, DocumentShardSampler) and len(s) == 3 for s in samplers)
    per_epoch = []
    for epoch in (0, 1, 2):
        for s in samplers:
            s.set_epoch(epoch)
        assert [v.epoch for v in views] == [epoch, epoch]
        assert np.array_equal(samplers[0].permutation(), samplers[1].permutation())
        orders = [[v.order(k)[0].tolist() for k in range(n, 2 * n)] for v in views]
        assert orders[0] == orders[1]                                  # the same twin on every rank, no collective
        assert orders[0] == [O.shuffle_rule(LABELS[d], SEED, epoch, d)[0] for d in range(n)]
        assert all(sorted(o) == list(range(len(O.segment_ends(LABELS[d])))) and not views[0].order(n + d)[1] for d, o in enumerate(orders[0]))
        # the ranks' shares of one global batch are disjoint and pad alike, to the longest VIRTUAL document of the global batch
        for (ix0, pad0), (ix1, pad1), g in zip(samplers[0], samplers[1], samplers[0].global_batches()):
            assert sorted(ix0 + ix1) == sorted(g.tolist()) and pad0 == pad1 == int(views[0].lengths[g].max())
        per_epoch.append(orders[0])
    assert per_epoch[0] != per_epoch[1] and per_epoch[1] != per_epoch[2]
    # 'reverse' is fixed per document, whatever the epoch
    rv = ResidentCorpus(_dataset(False), 'cpu').augmented('reverse')
    fixed = [rv.order(n + d) for d in range(n)]
    rv.sampler(4).set_epoch(5)
    assert all(a[0].tolist() == b[0].tolist() and a[1] == b[1] for a, b in zip(fixed, [rv.order(n + d) for d in range(n)]))
    assert [(o.tolist(), c) for o, c in fixed] == [tuple(O.reverse_rule(y)) for y in LABELS]
    # with truncate=True every batch is truncate_value long: the sampler hands out no pad_to
    assert all(pad is None for _, pad in ResidentCorpus(_dataset(True), 'cpu').augmented('shuffle').sampler(4))


def test_bad_orders_and_other_refusals():
    from multimodaltopicsegmentation_amd import ResidentCorpus, load_dataset_from_precomputed
    rc = ResidentCorpus(_dataset(False), 'cpu')
    for orders in ([[], [0]], [[0, 0], [0]], [[0, 1, 0], [0]], [[3], [0]], [[-1], [0]], [[0], [1]], [[0]]):
        with pytest.raises(ValueError):
            rc.batch_segments([1, 3], orders, False)                   # document 1 has segments 0 .. 2, document 3 only segment 0
    with pytest.raises(ValueError):
        rc.batch_segments([1, 3], [[0], [0]], [True, False, True])
    with pytest.raises(ValueError):
        rc.batch_segments([1, 3], [[2, 0, 1], [0]], False, pad_to=6)   # below the longest augmented document (7)
    with pytest.raises(ValueError):
        ResidentCorpus(_dataset(True), 'cpu').batch_segments([1], [[0]], False, pad_to=TV)
    for bad in ([6], [-1]):
        with pytest.raises(IndexError):
            rc.batch_segments(bad, [[0]], False)
    with pytest.raises(RuntimeError):
        rc.batch_segments([1, 3], [[2, 0, 1], [0]], False)             # valid: only now does the missing GPU matter
    assert rc.batch_segments([], [], False) == {}
    with pytest.raises(ValueError):
        rc.augmented('mirror')
    # labels that are not 0 / 1: the corpus is still a corpus (batch() never looked), but it has no segments to reorder
    labels = [list(y) for y in LABELS]
    labels[1][3] = 2
    odd = ResidentCorpus(_dataset(False, labels=labels), 'cpu')
    assert odd.host_fields([1])[1] == 7
    with pytest.raises(ValueError):
        odd.batch_segments([0], [[0]], False)
    with pytest.raises(ValueError):
        odd.augmented('reverse')
    # the loader still refuses the load-time flag
    with pytest.raises(NotImplementedError, match='augmented'):
        load_dataset_from_precomputed('nowhere', 'nothing.pkl', inverse_augmentation=True)
