"""CPU-only: the gradient-clipping entry points (include/mts.h: mts_grad_norm, mts_adam_step_clipped, mts_sgd_step_clipped) are declared,
exported and bound, validate their arguments before any device work, and trainer.NativeTrainer takes Lightning's gradient_clip_val /
gradient_clip_algorithm / error_if_nonfinite (train_fit.py:288,295,779)."""
import ctypes as C

import pytest

NEW = ('mts_grad_norm_workspace', 'mts_grad_norm', 'mts_adam_step_clipped', 'mts_sgd_step_clipped')
# addresses that are never dereferenced: validation fails (or n == 0 returns) before any device work
A16, A16B, ODD = 0x10000, 0x20000, 0x10004


def _spans(*spans):
    return (C.c_size_t * len(spans))(*[a for a, _ in spans]), (C.c_size_t * len(spans))(*[b for _, b in spans])


def test_new_symbols_are_declared_exported_and_bound():
    from multimodaltopicsegmentation_amd import _lib as L, ops
    from tests.test_abi import _declared
    decl = _declared()
    for name in NEW:
        assert name in decl, f'{name} not declared in include/mts.h'
        assert hasattr(L.lib, name) and name in L.SIGNATURES
        assert len(L.SIGNATURES[name][1]) == decl[name]
    assert L.lib.mts_grad_norm_workspace() >= 4
    for fn in ('grad_norm', 'grad_norm_workspace', 'adam_step_clipped', 'sgd_step_clipped'):
        assert callable(getattr(ops, fn))


def test_grad_norm_validates_before_any_device_work():
    from multimodaltopicsegmentation_amd import _lib as L
    b, e = _spans((0, 8))
    assert L.lib.mts_grad_norm(None, None, 1, b, e, 1.0, A16B, A16B + 0x8000) == 1            # null gradient
    with pytest.raises(ValueError):
        L.check(1)
    assert b'null' in L.lib.mts_last_error()
    assert L.lib.mts_grad_norm(None, A16, 1, b, e, 1.0, None, A16B) == 1                      # null workspace
    assert L.lib.mts_grad_norm(None, A16, 1, b, e, 1.0, A16B, None) == 1                      # null result
    assert L.lib.mts_grad_norm(None, A16, 0, b, e, 1.0, A16B, A16B + 0x8000) == 1             # no spans
    assert L.lib.mts_grad_norm(None, A16, 5, b, e, 1.0, A16B, A16B + 0x8000) == 1             # more spans than the kernel takes
    assert L.lib.mts_grad_norm(None, ODD, 1, b, e, 1.0, A16B, A16B + 0x8000) == 1             # base not 16-byte aligned
    assert b'16-byte' in L.lib.mts_last_error()
    b, e = _spans((0, 8), (9, 17))                                                            # second span begins at element 9
    assert L.lib.mts_grad_norm(None, A16, 2, b, e, 1.0, A16B, A16B + 0x8000) == 1
    assert b'span 1' in L.lib.mts_last_error()
    b, e = _spans((8, 4))
    assert L.lib.mts_grad_norm(None, A16, 1, b, e, 1.0, A16B, A16B + 0x8000) == 1             # ends before it begins
    b, e = _spans((0, 0), (16, 16))
    assert L.lib.mts_grad_norm(None, A16, 2, b, e, 1.0, A16B, A16B + 0x8000) == 0             # nothing to sum: OK, no launch


@pytest.mark.parametrize('which', ['adam', 'sgd'])
def test_clipped_steps_validate_before_any_device_work(which):
    from multimodaltopicsegmentation_amd import _lib as L
    p, g, m, v, norm = A16, A16 + 0x1000, A16 + 0x2000, A16 + 0x3000, A16B

    def call(n=8, param=p, grad=g, total_norm=norm, max_norm=1.0, clip_value=0.0, mom=m):
        if which == 'adam':
            return L.lib.mts_adam_step_clipped(None, n, param, grad, mom, v, 1e-3, 0.9, 0.999, 1e-7, 1, 1.0, None, total_norm, max_norm,
                                               clip_value, None)
        return L.lib.mts_sgd_step_clipped(None, n, param, grad, mom, 1e-2, 0.9, 1e-4, 1, 1.0, None, total_norm, max_norm, clip_value, None)

    assert call(grad=None) == 1                                   # null gradient
    assert call(param=None) == 1 and call(mom=None) == 1
    assert call(max_norm=-1.0) == 1                               # negative max_norm
    assert b'max_norm' in L.lib.mts_last_error()
    assert call(max_norm=float('nan')) == 1
    assert call(clip_value=-0.5, total_norm=None) == 1
    assert call(total_norm=None, clip_value=0.0) == 1             # neither mode
    assert call(total_norm=norm, clip_value=0.5) == 1             # both modes
    if which == 'adam':
        assert call(grad=ODD) == 1 and call(param=ODD) == 1       # the kernel's 16-byte accesses
        assert b'aligned' in L.lib.mts_last_error()
    assert call(grad=A16 + 1) == 1                                # not even a float boundary
    assert call(n=0) == 0                                         # norm mode, nothing to step
    assert call(n=0, total_norm=None, clip_value=0.5) == 0        # value mode


class _Flat:
    """what NativeTrainer's constructor reads of a tagger"""
    flat = None


def test_native_trainer_takes_lightnings_clipping_arguments():
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    with pytest.raises(ValueError):
        NativeTrainer(_Flat(), gradient_clip_val=1.0, gradient_clip_algorithm='l1')
    with pytest.raises(ValueError):
        NativeTrainer(_Flat(), gradient_clip_algorithm='l1')      # refused even while clipping is off
    with pytest.raises(ValueError):
        NativeTrainer(_Flat(), gradient_clip_val=-1.0)
    for off in (None, 0.0, 0):
        tr = NativeTrainer(_Flat(), gradient_clip_val=off)
        assert tr.clip_mode is None and tr.last_grad_norm is None and tr.last_clip_coef is None
    assert NativeTrainer(_Flat()).clip_mode is None               # the reference CLI's default
    tr = NativeTrainer(_Flat(), gradient_clip_val=0.5)
    assert tr.clip_mode == 'norm' and tr.gradient_clip_val == 0.5 and tr.error_if_nonfinite is False
    assert tr.last_grad_norm is None                              # nothing stepped yet
    tr = NativeTrainer(_Flat(), gradient_clip_val=2, gradient_clip_algorithm='value', error_if_nonfinite=True)
    assert tr.clip_mode == 'value' and tr.gradient_clip_val == 2.0 and tr.error_if_nonfinite is True
