"""CPU tests of the gated late-fusion merge: constructor validation, parameter layout and padding, that the default (concat) is untouched,
the argument checks of mts_gate_merge_fwd / _bwd (no device work), the fp64 oracle (tests/gated_fusion_oracle.py) against gradcheck, and
the condition on the GPU tests' inputs that makes the gate matter."""
import ctypes

import pytest
import torch

from tests import gated_fusion_oracle as O


def _ctor(H=32, **kw):
    from multimodaltopicsegmentation_amd import BiLSTMLateFusion
    return BiLSTMLateFusion(2, [40, 24], H, num_layers=2, loss_fn='FocalLoss', compute_dtype='fp32', **kw)


def test_constructor_validation():
    from multimodaltopicsegmentation_amd import BiLSTMLateFusion, TextSegmenter
    for bad in ('Gate', 'sum', None, 1):
        with pytest.raises(ValueError):
            _ctor(merge=bad)
    assert _ctor().merge == 'concat' and _ctor(merge='gate').merge == 'gate'
    for arch in ('BiLSTM', 'biLSTMCRF', 'Transformer', 'SwitchBiLSTM', 'SheikhBiLSTM', 'RecurrentLongT5'):
        with pytest.raises(ValueError):
            TextSegmenter(2, 40, 32, architecture=arch, fusion_merge='gate')
    with pytest.raises(ValueError):
        TextSegmenter(2, [40, 24], 32, architecture='BiLSTMLateFusion', fusion_merge='mean')
    ts = TextSegmenter(2, [40, 24], 32, architecture='BiLSTMLateFusion', fusion_merge='gate', loss_fn='FocalLoss')
    assert isinstance(ts.model, BiLSTMLateFusion) and ts.model.merge == 'gate' and ts.double_input
    assert TextSegmenter(2, [40, 24], 32, architecture='BiLSTMLateFusion').model.merge == 'concat'
    assert TextSegmenter(2, 40, 32, architecture='BiLSTM', fusion_merge='concat').model is not None      # the default passes everywhere


@pytest.mark.parametrize('H', [32, 25])
def test_state_dict_keys_and_unpadded_shapes(H):
    gate, cat = _ctor(H, merge='gate'), _ctor(H)
    sd, sc = gate.state_dict(), cat.state_dict()
    assert set(sd) == set(sc) | {'gate.weight', 'gate.bias'}
    assert {n: tuple(t.shape) for n, t in sd.items()} == O.param_shapes((40, 24), H, 2, 1)
    assert tuple(sc['classification.weight'].shape) == (1, 4 * H)
    Hp = (H + 7) // 8 * 8
    assert tuple(gate.gate.weight.shape) == (2 * Hp, 4 * Hp) and tuple(gate.gate.bias.shape) == (2 * Hp,)
    assert tuple(gate.classification.weight.shape) == (1, 2 * Hp)
    assert gate._layout.pads.get('gate.weight') == ([(0, 2, H, Hp), (1, 4, H, Hp)] if Hp != H else None)
    assert gate._layout.pads.get('gate.bias') == ([(0, 2, H, Hp)] if Hp != H else None)
    # load_state_dict takes the unpadded shapes back, bit for bit
    other = _ctor(H, merge='gate', seed=99)
    other.load_state_dict(sd)
    assert torch.equal(other.flat, gate.flat)
    assert not sd['gate.bias'].any() and float(sd['gate.weight'].abs().max()) <= 1.0 / (4 * H) ** 0.5      # init: zero bias, nn.Linear's weight


def _real_mask(m):
    """1 where the flat vector holds a real (reference-shaped) parameter entry, 0 at pad entries and alignment gaps"""
    from multimodaltopicsegmentation_amd.flat import pad_blocks
    mask = torch.zeros(m._layout.numel)
    for name, (off, shape) in m._layout.entries.items():
        ones = torch.ones(tuple(m.state_dict()[name].shape))
        m._layout.view(mask, name).copy_(pad_blocks(ones, m._layout.pads[name]) if name in m._layout.pads else ones)
    return mask


@pytest.mark.parametrize('H', [32, 25])
def test_pad_entries_are_zero_after_init(H):
    m = _ctor(H, merge='gate', seed=3)
    mask = _real_mask(m)
    assert int(mask.sum()) == sum(t.numel() for t in m.state_dict().values())
    assert not m.flat[mask == 0].any()
    if H == 25:
        assert int((mask == 0).sum()) > 64 * 128 - 50 * 100                   # the gate's pad rows and columns are among them
        assert float(m.flat[mask == 1].abs().sum()) > 0


def test_concat_default_is_untouched_and_the_encoders_draw_the_same_weights():
    a, b, g = _ctor(seed=5), _ctor(seed=5, merge='concat'), _ctor(seed=5, merge='gate')
    assert list(a._layout.entries.items()) == list(b._layout.entries.items()) and torch.equal(a.flat, b.flat)
    assert 'gate.weight' not in a._layout.entries and not hasattr(a, 'gate')
    sa, sg = a.state_dict(), g.state_dict()
    for n in sa:
        if n.startswith('model'):
            assert torch.equal(sa[n], sg[n]), n                                 # the gate and the narrower head are drawn after the encoders


def _fake(n=1 << 20, off=0):
    """an aligned non-null address that is never dereferenced: every call below must be refused before any device work"""
    return ctypes.c_void_p(n + off)


def _fwd(L, dtype, rows, W, ptrs=None, lds=None):
    ptrs = ptrs or [_fake()] * 4
    lds = lds or [W] * 4
    return L.lib.mts_gate_merge_fwd(None, dtype, rows, W, *[v for pair in zip(ptrs, lds) for v in pair])


def _bwd(L, dtype, rows, W, ptrs=None, lds=None):
    ptrs = ptrs or [_fake()] * 7
    lds = lds or [W] * 7
    return L.lib.mts_gate_merge_bwd(None, dtype, rows, W, *[v for pair in zip(ptrs, lds) for v in pair])


@pytest.mark.parametrize('call,n', [(_fwd, 4), (_bwd, 7)], ids=['fwd', 'bwd'])
def test_entry_points_refuse_bad_arguments_before_any_device_work(call, n):
    from multimodaltopicsegmentation_amd import _lib as L
    INVALID = 1
    assert call(L, 7, 4, 16) == INVALID and call(L, -1, 4, 16) == INVALID                  # unknown dtype
    with pytest.raises(ValueError):
        L.check(call(L, 7, 4, 16))
    for dt in (L.F32, L.BF16):
        es = 4 if dt == L.F32 else 2
        assert call(L, dt, 4, 0) == INVALID and call(L, dt, 4, -8) == INVALID              # W < 1
        assert call(L, dt, 4, 18) == INVALID and call(L, dt, 4, 2) == INVALID              # W no multiple of 4
        for k in range(n):                                                                 # every operand in turn
            lds = [16] * n
            lds[k] = 12
            assert call(L, dt, 4, 16, lds=lds) == INVALID, k                               # a leading dimension below W
            lds[k] = 18
            assert call(L, dt, 4, 16, lds=lds) == INVALID, k                               # ... no multiple of 4
            ptrs = [_fake()] * n
            ptrs[k] = _fake(off=es)                                                        # one element past a vector boundary
            assert call(L, dt, 4, 16, ptrs=ptrs) == INVALID, k
            ptrs[k] = _fake(off=2 * es)
            assert call(L, dt, 4, 16, ptrs=ptrs) == INVALID, k
            ptrs[k] = None                                                                 # a null operand with rows > 0
            assert call(L, dt, 4, 16, ptrs=ptrs) == INVALID, k
            assert b'NULL' in L.lib.mts_last_error()
        # rows == 0: MTS_OK without a launch, null operands included
        assert call(L, dt, 0, 16) == 0 and call(L, dt, 0, 16, ptrs=[None] * n) == 0
        assert call(L, dt, 0, 18) == INVALID                                               # ... but the shape is still checked


def test_oracle_gradient_against_gradcheck():
    """B = 2, L = 5, H = 4: autograd through the oracle against finite differences, and the backward as the definition writes it out (what
    the kernels and GEMMs compute) against autograd."""
    torch.manual_seed(0)
    B, L, H, D = 2, 5, 4, (6, 3)
    lengths = torch.tensor([5, 3])
    x1, x2 = torch.randn(B, L, D[0], dtype=torch.float64), torch.randn(B, L, D[1], dtype=torch.float64)
    tags = (torch.rand(B, L) < 0.4).double()
    names, shapes = zip(*O.param_shapes(D, H, 1, 1).items())
    vals = [(torch.randn(s, dtype=torch.float64) * (2.0 if n == 'gate.weight' else 0.5)).requires_grad_(True) for n, s in zip(names, shapes)]

    for loss_fn, segments in (('FocalLoss', None), ('BinaryCrossEntropy', None), ('FocalLoss', [[2, 5], [1]])):
        def f(*ts):
            return O.loss(x1, x2, lengths, tags, dict(zip(names, ts)), loss_fn, segments=segments, batched=False)[0]
        assert torch.autograd.gradcheck(f, vals, eps=1e-6, atol=1e-7, rtol=1e-5)

    h1, h2 = (torch.randn(7, 2 * H, dtype=torch.float64, requires_grad=True) for _ in range(2))
    wg = (torch.randn(2 * H, 4 * H, dtype=torch.float64) * 2).requires_grad_(True)
    bg = torch.randn(2 * H, dtype=torch.float64, requires_grad=True)
    m, z, _ = O.gate(h1, h2, wg, bg)
    dm = torch.randn_like(m)
    auto = torch.autograd.grad(m, (h1, h2, wg, bg), dm)
    dh1, dh2, _, dwg, dbg = O.gate_backward(h1.detach(), h2.detach(), wg.detach(), z.detach(), dm)
    for got, want in zip((dh1, dh2, dwg, dbg), auto):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-13)
    assert torch.allclose(m, z * h1 + (1 - z) * h2, rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize('H', [32, 25])
def test_the_gpu_cases_spread_their_gates(H):
    """tests/test_gpu_gated_fusion.py scales gate.weight (O.GATE_SCALE) so that the gate matters: at least a fifth of the oracle's gates over
    valid rows lie outside [0.25, 0.75].  A condition on the inputs, established here."""
    cs = O.small_case(H)
    p = {n: t.double() for n, t in cs['p'].items()}
    _, z = O.scores(cs['x1'].double(), cs['x2'].double(), cs['lengths'], p, return_gate=True)
    frac = O.decided_fraction(z, cs['lengths'].tolist())
    print(f'gated fusion H={H}: {frac:.3f} of the valid gates outside [0.25, 0.75]')
    assert frac >= 0.2
