"""CPU-only checks of the decision-threshold search: the two forms of tests/sweep_oracle.py agree exactly (so the integer definition the
kernel implements IS metrics.py's Pk / WindowDiff / F1), ThresholdSweep's host side (table, selection rules, fallback, metric names)
through its add_counts seam, and the C entry point's argument validation, which happens before any device work."""
import ctypes as C

import numpy as np
import pytest

from tests import sweep_oracle as O


def _documents():
    """(name, hypothesis, target) triples: random documents, the smallest ones, n = k and n = k + 1, and the special targets."""
    rng = np.random.default_rng(20240611)
    docs = []
    for n in (1, 2, 3, 4, 5, 7, 16, 63, 64, 65, 130, 257, 300):
        for rate in (0.0, 0.1, 0.5, 1.0):
            docs.append((f'rand{n}@{rate}', rng.random(n) < 0.3, (rng.random(n) < rate).astype(np.float32)))
    for name, t in O.special_targets().items():
        docs.append((name, rng.random(len(t)) < 0.3, t))
        docs.append((name + '/same', t.copy(), t))
        docs.append((name + '/empty', np.zeros(len(t)), t))
    return docs


DOCS = _documents()


def test_window_k_is_metrics_default_k():
    from multimodaltopicsegmentation_amd import metrics
    for n in range(1, 400):
        for nseg in range(1, n + 1):
            masses = [1] * (nseg - 1) + [n - (nseg - 1)]
            assert O.window_k(n, nseg) == metrics._default_k(masses), (n, nseg)
    assert [O.window_k(n, 4) for n in (12, 20, 28, 36)] == [2, 2, 4, 4]


@pytest.mark.parametrize('end_boundary', [False, True])
def test_counts_and_metrics_agree_exactly(end_boundary):
    for name, h, t in DOCS:
        c = O.counts(h, t, end_boundary)
        assert O.floats(c) == O.via_metrics(h, t, end_boundary), (name, c)
        n = len(t)
        assert c[2] == max(n - O.window_k(n, 1 + int((np.asarray(t)[:n - 1] == 1).sum())), 0)
    assert O.counts([], [], end_boundary).tolist() == [0] * 6


def test_edge_lengths_are_covered():
    """n in {1, 2, 3, k, k + 1}: no window at all up to n = k, exactly one at n = k + 1."""
    windows = {}
    for name, h, t in DOCS:
        n = len(t)
        k = O.window_k(n, 1 + int((np.asarray(t)[:n - 1] == 1).sum()))
        windows.setdefault(n - k, []).append(name)
        assert O.counts(h, t)[2] == max(n - k, 0)
    assert {-1, 0, 1} <= set(windows), sorted(windows)          # n < k (n = 1), n = k, n = k + 1
    sp = O.special_targets()
    assert [len(sp[f'tie{n}']) - int(O.counts(sp[f'tie{n}'], sp[f'tie{n}'])[2]) for n in (12, 20, 28, 36)] == [2, 2, 4, 4]
    assert 50 - int(O.counts(sp['none'], sp['none'])[2]) == 25 and 50 - int(O.counts(sp['all'], sp['all'])[2]) == 2


def test_end_boundary_only_touches_the_hypothesis_last_sentence():
    t = np.array([0, 1, 0, 0, 1, 0, 0, 1], dtype=np.float32)
    h = np.array([0, 1, 0, 1, 0, 0, 0, 1])
    off, on = O.counts(h, t, False), O.counts(h, t, True)
    assert off[:3].tolist() == on[:3].tolist()
    assert off[3:].tolist() == [1, 2, 1] and on[3:].tolist() == [1, 1, 1]     # the target's last 1 never counts; the hypothesis' only without end_boundary


# ---- ThresholdSweep's host side --------------------------------------------------------------------------------------------
def _sweep_with(counts, **kw):
    from multimodaltopicsegmentation_amd import ThresholdSweep
    s = ThresholdSweep(**kw)
    s.add_counts(np.asarray(counts))
    return s


def _random_counts(rng, docs, T):
    c = np.zeros((docs, T, 6), dtype=np.int64)
    w = rng.integers(0, 40, size=docs)
    w[0] = 0                                                   # a document without windows
    for d in range(docs):
        c[d, :, 2] = w[d]
        c[d, :, 0] = rng.integers(0, w[d] + 1, size=T)
        c[d, :, 1] = np.minimum(c[d, :, 0] + rng.integers(0, 3, size=T), w[d])
        c[d, :, 3:] = rng.integers(0, 6, size=(T, 3))
    c[1, :, 3] = 0                                             # ... and one without a true positive
    return c


def test_table_equals_the_sequential_host_sums():
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS
    assert len(DEFAULT_THRESHOLDS) == 19 and DEFAULT_THRESHOLDS.dtype == np.float64
    assert np.array_equal(DEFAULT_THRESHOLDS, np.arange(0.05, 1, 0.05))
    rng = np.random.default_rng(5)
    c = _random_counts(rng, 11, 19)
    s = _sweep_with(c[:4])
    s.add_counts(c[4:])                                        # two batches of different size
    assert np.array_equal(s.counts(), c) and s.counts().dtype == np.int64
    want = O.mean_table([[O.floats(c[d, j]) for j in range(19)] for d in range(11)], DEFAULT_THRESHOLDS)
    got = s.table()
    assert set(got) == {'thresholds', 'Pk_loss', 'WD_loss', 'F1_loss'}
    for k in want:
        assert list(got[k]) == list(want[k]), k                # equal, not close
    for metric in ('Pk', 'WD', 'F1', 'pk'):
        assert s.best(metric) == O.select(want, metric), metric
    s.reset()
    assert s.counts().shape == (0, 19, 6)
    with pytest.raises(ValueError):
        s.table()


def _counts_for(pk, wd, f1_tp):
    """One document, T thresholds: 10 windows with the given error counts; tp as given with fp = fn = 1."""
    T = len(pk)
    c = np.zeros((1, T, 6), dtype=np.int64)
    c[0, :, 0], c[0, :, 1], c[0, :, 2] = pk, wd, 10
    c[0, :, 3], c[0, :, 4], c[0, :, 5] = f1_tp, 1, 1
    return c


def test_selection_rules_ties_and_names():
    ths = [0.2, 0.4, 0.6, 0.8]
    s = _sweep_with(_counts_for([5, 3, 3, 4], [6, 6, 2, 2], [1, 4, 4, 0]), thresholds=ths)
    pk, wd, f1 = s.best('Pk'), s.best('WD'), s.best('F1')
    assert pk == {'valid_loss': 0.3, 'WD_loss': 0.6, 'F1_loss': 0.8, 'threshold': 0.4}        # the first of the two 3s wins
    assert wd == {'valid_loss': 0.2, 'Pk_loss': 0.3, 'F1_loss': 0.8, 'threshold': 0.6}        # the first of the two 2s
    assert f1 == {'valid_loss': 0.8, 'Pk_loss': 0.3, 'WD_loss': 0.6, 'threshold': 0.4}        # 2*4 / (2*4 + 2), the first of the two
    assert s.best('anything else') == pk


def test_fallback_threshold_when_nothing_beats_the_start_value():
    ths = [0.3, 0.7]
    s = _sweep_with(_counts_for([10, 10], [10, 10], [0, 0]), thresholds=ths)                  # Pk = WD = 1 (not < 1); F1 = 0 > -1
    assert s.best('Pk') == {'valid_loss': 1.0, 'WD_loss': 1.0, 'F1_loss': 0.0, 'threshold': 0.4}
    assert s.best('WD') == {'valid_loss': 1.0, 'Pk_loss': 1.0, 'F1_loss': 0.0, 'threshold': 0.4}
    assert s.best('F1') == {'valid_loss': 0.0, 'Pk_loss': 1.0, 'WD_loss': 1.0, 'threshold': 0.3}


def test_inverted_thresholds_are_the_sheikh_decode_arguments():
    from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS, ThresholdSweep
    s = ThresholdSweep(invert=True)
    assert s._device_values.dtype == np.float32
    assert s._device_values.tolist() == [C.c_float(1.0 - float(th)).value for th in DEFAULT_THRESHOLDS]
    assert ThresholdSweep()._device_values.tolist() == [C.c_float(float(th)).value for th in DEFAULT_THRESHOLDS]
    with pytest.raises(ValueError):
        ThresholdSweep(thresholds=[])
    with pytest.raises(ValueError):
        ThresholdSweep(thresholds=np.linspace(0.01, 0.99, 65))


# ---- C entry point: argument validation before any device work -------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_device():
    from multimodaltopicsegmentation_amd import _lib as L
    buf = (C.c_float * 64)()
    p = C.addressof(buf)                                       # never dereferenced: every call below is refused on its arguments
    f = L.lib.mts_threshold_sweep

    def call(B=1, Lq=4, Lt=4, n_out=1, scores=p, targets=p, lengths=None, T=3, ths=p, eb=0, out=p):
        return f(None, B, Lq, Lt, n_out, scores, targets, lengths, T, ths, eb, out)

    assert call(T=0) == 1 and call(T=65) == 1 and call(T=-1) == 1
    assert call(n_out=5) == 1 and call(n_out=0) == 1
    assert call(Lt=3) == 1
    assert call(scores=None) == 1 and call(targets=None) == 1 and call(ths=None) == 1 and call(out=None) == 1
    assert call(B=0) == 1 and call(Lq=0, Lt=0) == 1
    with pytest.raises(ValueError):
        L.check(call(T=65))
    assert call(Lq=65537, Lt=65537) == 2                        # MTS_ERR_UNSUPPORTED: documents above 65 536 sentences
    with pytest.raises(NotImplementedError):
        L.check(call(Lq=65537, Lt=65537))


def test_hook_is_inert_without_the_flag_and_refuses_what_the_kernel_does_not_cover():
    """TextSegmenter.on_validation_epoch_end on the host: None without search_threshold; no sweep for the CRF tagger or for 'b' / 'scaiano'."""
    from multimodaltopicsegmentation_amd import TextSegmenter
    assert TextSegmenter(2, 64, 32, architecture='BiLSTM', loss_fn='FocalLoss').on_validation_epoch_end() is None
    for kw in (dict(architecture='biLSTMCRF'), dict(architecture='BiLSTM', loss_fn='FocalLoss', metric='scaiano'),
               dict(architecture='BiLSTM', loss_fn='FocalLoss', metric='B')):
        ts = TextSegmenter(2, 64, 32, search_threshold=True, **kw)
        assert ts._sweep is None
        with pytest.raises(NotImplementedError, match='search_threshold'):
            ts.on_validation_epoch_end()
    ts = TextSegmenter(2, 64, 32, architecture='SheikhBiLSTM', search_threshold=True, end_boundary=True)
    assert ts._sweep.invert and ts._sweep.end_boundary
    ts = TextSegmenter(2, 64, 32, architecture='BiLSTM', loss_fn='FocalLoss', search_threshold=True)
    assert not ts._sweep.invert and not ts._sweep.end_boundary
