"""CPU-only checks of the fit loop's two rules (fit.PlateauLR, fit.BestTracker -- the objects fit() itself steps once per epoch) on scripted
monitor sequences, and of the argument checks that need no device."""
import pytest
import torch

MIN_SEQ = [5.0, 4.0, 4.0, 3.0, 3.5, 3.0, 3.2, 3.1, 2.0, 2.0, 2.5, 2.0, 2.0, 2.0]
MAX_SEQ = [-v for v in MIN_SEQ]


def _reference_trace(seq, lr, mode, factor, patience):
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode, factor=factor, patience=patience)
    out = []
    for v in seq:
        sched.step(v)
        out.append(opt.param_groups[0]['lr'])
    return out


@pytest.mark.parametrize('mode,seq', [('min', MIN_SEQ), ('max', MAX_SEQ)])
@pytest.mark.parametrize('factor,patience', [(0.8, 10), (0.8, 1), (0.5, 0), (0.1, 2)])
def test_lr_trace_is_torch_reduce_on_plateau(mode, seq, factor, patience):
    from multimodaltopicsegmentation_amd.fit import PlateauLR
    rule = PlateauLR(0.01, mode, factor, patience)
    got = [rule.step(v) for v in seq * 2]
    assert got == _reference_trace(seq * 2, 0.01, mode, factor, patience)
    if patience < 10:
        assert got[-1] < 0.01                                  # the sequence does reach a plateau


def _run(seq, mode, patience):
    """the loop's use of BestTracker -> (stop epoch or None, best epoch, best value, epochs at which the state would be cloned)"""
    from multimodaltopicsegmentation_amd.fit import BestTracker
    tr = BestTracker(mode, patience)
    cloned = []
    for epoch, v in enumerate(seq):
        improved, stop = tr.step(epoch, v)
        if improved:
            cloned.append(epoch)
        if stop:
            return epoch, tr.best_epoch, tr.best, cloned
    return None, tr.best_epoch, tr.best, cloned


@pytest.mark.parametrize('mode,seq,sign', [('min', MIN_SEQ, 1.0), ('max', MAX_SEQ, -1.0)])
def test_early_stopping_is_lightnings_with_min_delta_zero(mode, seq, sign):
    """strict improvement only: the repeated 4.0 at epoch 2 does not count as one.  Consecutive epochs without improvement: epoch 2 (one),
    4-7 (four), 9-13 (five)."""
    improving = [0, 1, 3, 8]
    assert _run(seq, mode, None) == (None, 8, sign * 2.0, improving)
    assert _run(seq, mode, 0) == (2, 1, sign * 4.0, [0, 1])     # Lightning: wait_count 1 >= 0 at the first epoch that is no better
    assert _run(seq, mode, 1) == (2, 1, sign * 4.0, [0, 1])
    assert _run(seq, mode, 3) == (6, 3, sign * 3.0, [0, 1, 3])  # epochs 4, 5, 6; epoch 2 alone was forgiven by the improvement at 3
    assert _run(seq, mode, 5) == (13, 8, sign * 2.0, improving)
    assert _run(seq[:1], mode, 0) == (None, 0, sign * 5.0, [0])  # a first epoch always improves


def test_monitor_mode_follows_the_reference():
    from multimodaltopicsegmentation_amd.fit import BestTracker, monitor_mode
    assert [monitor_mode(True, m) for m in ('Pk', 'pk', 'WD', 'F1', 'scaiano', 'B')] == ['min', 'min', 'min', 'max', 'max', 'max']
    assert [monitor_mode(False, m) for m in ('Pk', 'F1', 'scaiano')] == ['min'] * 3
    with pytest.raises(ValueError):
        BestTracker('best')


def test_fit_is_exported_and_forwarded():
    import inspect
    import multimodaltopicsegmentation_amd as M
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    sig = inspect.signature(M.fit)
    assert list(sig.parameters)[:3] == ['trainer', 'train', 'val']
    want = dict(search_threshold=False, metric='Pk', thresholds=None, end_boundary=False, patience=None, lr_factor=0.8, lr_patience=10, seed=0,
                shuffle=True, restore_best=True, on_epoch_end=None)
    for k, v in want.items():
        assert sig.parameters[k].default == v and sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert sig.parameters['batch_size'].default is inspect.Parameter.empty and sig.parameters['max_epochs'].default is inspect.Parameter.empty
    calls = []

    class Probe(NativeTrainer):
        def __init__(self):
            pass
    import sys
    F = sys.modules['multimodaltopicsegmentation_amd.fit']   # the module: the package attribute of that name is the function
    old = F.fit
    F.fit = lambda *a, **k: calls.append((a, k)) or 'record'
    try:
        p = Probe()
        assert p.fit('train', 'val', batch_size=3, max_epochs=2) == 'record'
        assert calls == [((p, 'train', 'val'), dict(batch_size=3, max_epochs=2))]
    finally:
        F.fit = old
