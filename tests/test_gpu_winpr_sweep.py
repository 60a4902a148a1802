"""GPU tests of the WinPR threshold sweep (mts_winpr_sweep, ops.winpr_sweep, ThresholdSweep(metric='scaiano')).  Every comparison of integers
and float64 values is `==`: the expected three floats per document x threshold come from metrics.WinPR on integer lists over the tags
ops.greedy_decode produces at that threshold, the expected three integers from the closed form of tests/winpr_oracle.py, and the two are
asserted to agree before the kernel is looked at."""
import numpy as np
import pytest
import torch

from tests import winpr_oracle as W

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LENGTHS = [300, 257, 256, 65, 64, 63, 12, 10, 9, 5, 2, 1, 0]


def _batch(n_out, B=13, L=300, Lt=303, lengths=LENGTHS, seed=0, rate=0.15):
    """scores = 2 randn with a few entries at +-30 (saturated probabilities), targets 0 / 1 inside each length and -1 behind it."""
    g = torch.Generator().manual_seed(4321 + 10 * n_out + seed)
    scores = 2 * torch.randn(B, L, n_out, generator=g)
    flat = scores.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:12]
    flat[idx[:6]], flat[idx[6:]] = 30.0, -30.0
    targets = (torch.rand(B, Lt, generator=g) < rate).float()
    if lengths is not None:
        for b, n in enumerate(lengths):
            targets[b, n:] = -1.0
    return scores, targets


def _expected(scores_d, targets, lengths, device_values, end_boundary, k=10):
    """Per threshold: decode on the device, then per document metrics.WinPR on integer lists and the closed form ->
    counts [B, T, 3] int64, floats [B][T] of (P, R, F), and the number of (document, threshold) pairs with a wrap-around `prev`."""
    from multimodaltopicsegmentation_amd import ops
    B, L, _ = scores_d.shape
    lens = [L] * B if lengths is None else list(lengths)
    li32 = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    tags = torch.empty(B, L, dtype=torch.uint8, device=DEV)
    counts = np.zeros((B, len(device_values), 3), dtype=np.int64)
    fl = [[None] * len(device_values) for _ in range(B)]
    tgt = targets.numpy()
    wraps = 0
    for j, th in enumerate(device_values):
        ops.greedy_decode(scores_d, li32, float(th), tags)
        tags_h = tags.cpu().numpy()
        for b, n in enumerate(lens):
            h, t = W.operands(tags_h[b, :n], tgt[b, :n], end_boundary)
            fl[b][j] = W.via_metrics(h, t, k)
            counts[b, j] = W.counts_closed(h, t, k)
            assert W.floats(counts[b, j]) == fl[b][j], (b, j)
            wraps += (W.wrap_prevs(h, k) + W.wrap_prevs(t, k)) > 0
    return counts, fl, wraps


def _sweep(scores_d, targets_d, lengths, thresholds, end_boundary, invert=False, **kw):
    from multimodaltopicsegmentation_amd import ThresholdSweep
    s = ThresholdSweep(thresholds=thresholds, end_boundary=end_boundary, invert=invert, metric='scaiano', **kw)
    s.add(scores_d, targets_d, None if lengths is None else torch.tensor(lengths))
    return s


def _check(s, want_counts, want_floats):
    got = s.counts()
    assert got.dtype == np.int64 and got.shape == want_counts.shape
    assert np.array_equal(got, want_counts), np.argwhere(got != want_counts)[:10]
    per = s._per_document()
    for b in range(got.shape[0]):
        for j in range(got.shape[1]):
            assert tuple(per[b, j]) == want_floats[b][j], (b, j)
    tab = s.table()
    want = W.mean_table(want_floats, s.thresholds)
    for k in ('b_precision', 'b_recall', 'b_f1'):
        assert list(tab[k]) == want[k], k
    assert s.best('scaiano') == W.select(want)


@pytest.mark.parametrize('end_boundary', [False, True])
@pytest.mark.parametrize('T', [19, 1])
@pytest.mark.parametrize('n_out', [1, 2, 3])
def test_counts_equal_the_decode_kernel_and_metrics_winpr(n_out, T, end_boundary):
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS
    scores, targets = _batch(n_out)
    ths = DEFAULT_THRESHOLDS if T == 19 else np.array([0.5])
    want_counts, want_floats, _ = _expected(scores.to(DEV), targets, LENGTHS, ths, end_boundary)
    s = _sweep(scores.to(DEV), targets.to(DEV), LENGTHS, ths, end_boundary)
    _check(s, want_counts, want_floats)
    c = s.counts()
    assert c[..., 0].max() > 0 and c[..., 1].max() > 0 and c[..., 2].max() > 0        # the case is not vacuous
    assert (c[12] == 0).all()                                                          # n = 0: three zeros
    # the rows with n < 10 (9, 5, 2, 1 sentences) do exercise python's wrap-around of the previous window
    short = [8, 9, 10, 11]
    _, _, wraps = _expected(scores[short].contiguous().to(DEV), targets[short], [LENGTHS[b] for b in short], ths, end_boundary)
    assert wraps > 0
    assert c[short].max() > 0


def test_degenerate_classes_give_exact_counts_and_zero_floats():
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS
    lengths = [50, 45, 30, 60]
    scores, targets = _batch(1, B=4, L=60, Lt=60, lengths=lengths, seed=2, rate=0.2)
    targets[0, :50] = 0.0                                      # a target without boundaries: TP + FP == 0
    scores[1] = -30.0                                          # a hypothesis without boundaries against a target with some: TP + FN == 0
    assert targets[1, :45].sum() > 0
    scores[2], targets[2, :30] = 30.0, 1.0                     # all boundaries on both sides
    scores[3], targets[3, :60] = -30.0, 0.0                    # TP == 0 with FP, FN > 0: the windows of sentence 0 and of sentence 40 are disjoint
    scores[3, 0], targets[3, 40] = 30.0, 1.0
    want_counts, want_floats, _ = _expected(scores.to(DEV), targets, lengths, DEFAULT_THRESHOLDS, False)
    s = _sweep(scores.to(DEV), targets.to(DEV), lengths, DEFAULT_THRESHOLDS, False)
    _check(s, want_counts, want_floats)
    c, per = s.counts(), s._per_document()
    assert (c[0, :, 0] + c[0, :, 1] == 0).all() and (c[0, :, 2] > 0).any() and (per[0] == 0).all()
    assert (c[1, :, 0] + c[1, :, 2] == 0).all() and (c[1, :, 1] > 0).all() and (per[1] == 0).all()
    assert (c[2, :, 0] > 0).all() and (c[2, :, 1:] == 0).all() and (per[2] == 1.0).all()
    assert (c[3, :, 0] == 0).all() and (c[3, :, 1] > 0).all() and (c[3, :, 2] > 0).all() and (per[3] == 0).all()


@pytest.mark.parametrize('k', [1, 3, 10, 64])
def test_window_sizes_through_the_ops_wrapper(k):
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS, ops
    scores, targets = _batch(2, seed=4)
    want_counts, _, wraps = _expected(scores.to(DEV), targets, LENGTHS, DEFAULT_THRESHOLDS, False, k=k)
    out = torch.full((13, 19, 3), -7, dtype=torch.int32, device=DEV)
    ths = torch.from_numpy(DEFAULT_THRESHOLDS.astype(np.float32)).to(DEV)
    ops.winpr_sweep(scores.to(DEV), targets.to(DEV), torch.tensor(LENGTHS, dtype=torch.int32, device=DEV), ths, out, False, k)
    assert np.array_equal(out.cpu().numpy().astype(np.int64), want_counts)
    assert wraps == 0 if k == 1 else (wraps > 0 or k < 10)                             # no document is shorter than 1; four are shorter than 10
    s = _sweep(scores.to(DEV), targets.to(DEV), LENGTHS, None, False, winpr_k=k)
    assert np.array_equal(s.counts(), want_counts)


def test_long_documents():
    """9 000 and 4 097 sentences: more 64-sentence words than one pass of the workgroup, prefixes across every wave."""
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS
    lengths = [9000, 4097]
    scores, targets = _batch(1, B=2, L=9000, Lt=9000, lengths=lengths, seed=7, rate=0.01)
    ths = DEFAULT_THRESHOLDS[[0, 6, 12, 18]]
    want = _expected(scores.to(DEV), targets, lengths, ths, False)
    _check(_sweep(scores.to(DEV), targets.to(DEV), lengths, ths, False), *want[:2])


def test_the_longest_document_the_kernel_covers():
    """65 536 sentences, a multiple of 64: the count of the whole document is read from the one word behind the masks."""
    scores, targets = _batch(1, B=1, L=65536, Lt=65536, lengths=[65536], seed=8, rate=0.01)
    want = _expected(scores.to(DEV), targets, [65536], np.array([0.9]), False)
    _check(_sweep(scores.to(DEV), targets.to(DEV), [65536], np.array([0.9]), False), *want[:2])
    assert want[0][0, 0].min() > 0


def test_inverted_rule_equals_decode_at_one_minus_threshold():
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS
    scores, targets = _batch(1, seed=9)
    want = _expected(scores.to(DEV), targets, LENGTHS, [1.0 - float(th) for th in DEFAULT_THRESHOLDS], False)     # rnn_taggers: 1.0 - threshold
    _check(_sweep(scores.to(DEV), targets.to(DEV), LENGTHS, None, False, invert=True), *want[:2])


def test_lengths_none_and_descending_thresholds():
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS
    scores, targets = _batch(2, B=3, L=130, Lt=130, lengths=None, seed=3)
    want = _expected(scores.to(DEV), targets, None, DEFAULT_THRESHOLDS, False)
    _check(_sweep(scores.to(DEV), targets.to(DEV), None, DEFAULT_THRESHOLDS, False), *want[:2])
    desc = DEFAULT_THRESHOLDS[::-1].copy()
    s = _sweep(scores.to(DEV), targets.to(DEV), None, desc, False)
    assert np.array_equal(s.counts(), want[0][:, ::-1])
    assert list(s.table()['thresholds']) == list(desc)


def test_accumulation_over_batches_and_reproducibility():
    from multimodaltopicsegmentation_amd import ThresholdSweep
    s1, t1 = _batch(1, seed=11)
    s2, t2 = _batch(1, B=3, L=70, Lt=70, lengths=[70, 33, 1], seed=12)
    one = _sweep(s1.to(DEV), t1.to(DEV), LENGTHS, None, False).counts()
    two = _sweep(s2.to(DEV), t2.to(DEV), [70, 33, 1], None, False).counts()

    def run():
        s = ThresholdSweep(metric='scaiano')
        s.add(s1.to(DEV), t1.to(DEV), torch.tensor(LENGTHS), keys=list(range(13)))
        s.add(s2.to(DEV), t2.to(DEV), torch.tensor([70, 33, 1], device=DEV), keys=[13, 14, 15])
        return s
    a, b = run(), run()
    assert np.array_equal(a.counts(), np.concatenate([one, two], axis=0))
    assert np.array_equal(a.counts(), b.counts())
    ta, tb = a.table(), b.table()
    assert all(ta[k].tobytes() == tb[k].tobytes() for k in ta)
    assert a.gather() is a and np.array_equal(a.counts(), b.counts())                  # no process group: the identity
    a.reset()
    assert a.counts().shape == (0, 19, 3)


def test_wrapper_refuses_what_the_kernel_does_not_cover():
    from multimodaltopicsegmentation_amd import ops
    sc, tg = torch.zeros(1, 8, 1, device=DEV), torch.zeros(1, 8, device=DEV)
    out = torch.zeros(1, 65, 3, dtype=torch.int32, device=DEV)
    one = torch.zeros(1, device=DEV)
    for k in (0, 65):
        with pytest.raises(ValueError):
            ops.winpr_sweep(sc, tg, None, one, out[:, :1].contiguous(), False, k)
    with pytest.raises(ValueError):
        ops.winpr_sweep(sc, tg, None, torch.zeros(65, device=DEV), out)
    with pytest.raises(NotImplementedError):
        ops.winpr_sweep(torch.zeros(1, 65537, 1, device=DEV), torch.zeros(1, 65537, device=DEV), None, one, out[:, :1].contiguous())
    assert (out == 0).all()                                                            # refused before any device work


def test_relation_to_test_step_in_float32():
    """TextSegmenter.test_step calls metrics.WinPR(list(tag), tgt) with tgt a float32 array, so its sums, and with them its three results,
    are numpy.float32.  Each result is reached by at most six float32 roundings of values <= 1 (two quotients, a product, a sum, a quotient
    and the doubling), so the float64 values of the sweep lie within 8 * 2**-24 of it.  Non-degenerate documents only: there test_step
    raises ZeroDivisionError (or warns and returns nan) where the sweep reports zeros."""
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS, metrics, ops
    scores, targets = _batch(1, seed=13)
    sd = scores.to(DEV)
    s = _sweep(sd, targets.to(DEV), LENGTHS, None, False)
    per, c = s._per_document(), s.counts()
    tags = torch.empty(13, 300, dtype=torch.uint8, device=DEV)
    li32 = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    checked = single = 0
    for j, th in enumerate(DEFAULT_THRESHOLDS):
        ops.greedy_decode(sd, li32, float(th), tags)
        tags_h = tags.cpu().numpy().astype(bool)
        for b, n in enumerate(LENGTHS):
            if n == 0 or W.degenerate(c[b, j]):
                continue
            tgt = targets[b, :n].numpy()
            assert tgt.dtype == np.float32
            got = metrics.WinPR(list(tags_h[b, :n].tolist()), tgt)
            single += all(isinstance(v, np.float32) for v in got)
            for x, y in zip(per[b, j], got):
                assert abs(float(x) - float(y)) <= 8 * 2.0 ** -24, (b, j, x, y)
            checked += 1
    assert checked > 100 and single > checked // 2             # the comparison is against float32 results, as said
