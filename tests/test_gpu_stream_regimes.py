"""The flat streaming kernels of csrc/optim.hip and csrc/dropout.hip in every launch regime, against the references of tests/stream_oracle.py (which
also holds the size ladders; tests/test_stream_oracle_cpu.py pins both on the CPU):

  * mts_adam_step / mts_sgd_step and their clipped forms BIT FOR BIT against the float32 replicas over every size of their ladders (the scalar
    tail alone, one grid pass exactly, one element into the second trip, three trips with a tail), with and without the bf16 mirror, and
    against torch's optimizers in fp64 at two sizes each; the one narrowing to bf16 on crafted values;
  * mts_scale bit for bit; mts_grad_norm in the three- and four-trip cases of its two-loads-in-flight loop and over four spans, against fp64;
  * mts_dropout_fwd / mts_dropout_bwd in fp32 and bf16, with and without mask and residual, out of place and in place, bit for bit;
  * the refusals: bad arguments and every pointer off its vector boundary are ValueErrors before any launch.
Every output is a window inside a buffer prefilled with a NaN bit pattern: an element a kernel skips fails the comparison, and the guard elements
on either side must come back bit-identical.  No misaligned pointer reaches a kernel here: those calls are refused on the host.
"""
import numpy as np
import pytest
import torch

from tests import stream_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
ACTS = [F32, BF16]
ACT_IDS = ['fp32', 'bf16']
NAN_BITS = {BF16: (torch.int16, 0x7FC1), F32: (torch.int32, 0x7FC00DEA), U8: (torch.uint8, 0xA5)}
GUARD = 64                     # elements on either side: a multiple of 16 bytes in every dtype, so the window keeps the vector alignment
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-7
SEED = 123456789


@pytest.fixture(scope='module')
def ops():
    from multimodaltopicsegmentation_amd import ops as o
    return o


@pytest.fixture(scope='module')
def L():
    from multimodaltopicsegmentation_amd import _lib
    return _lib


class Win:
    """n elements inside a larger buffer of NaN bit patterns (0xA5 bytes for a mask), optionally filled with `init`"""

    def __init__(self, n, dtype=F32, init=None):
        it, self.bits = NAN_BITS[dtype]
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), self.bits, dtype=it, device=DEV)
        self.t = self.buf.view(dtype)[GUARD:GUARD + n]
        if init is not None:
            self.t.copy_(torch.as_tensor(init))

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.bits).all()) and bool((self.buf[GUARD + self.n:] == self.bits).all())

    def untouched(self):
        return bool((self.buf == self.bits).all())


def _off_by_one(n, dtype):
    """(buffer of NaN bit patterns, its window [1, 1 + n)): one element off the allocation's boundary"""
    it, bits = NAN_BITS[dtype]
    buf = torch.full((n + 8,), bits, dtype=it, device=DEV)
    return buf, buf.view(dtype)[1:1 + n]


def _t(ref):
    return ref if torch.is_tensor(ref) else torch.from_numpy(np.ascontiguousarray(ref))


def _ulps(a, b):
    """distance in float32 ulps between two finite float32 tensors, via the ordered-integer map"""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


def _same(win, ref, what):
    """the window holds exactly the bits of `ref`, and nothing was written outside it"""
    assert win.guards_intact(), f'{what}: written outside the output'
    got_t, ref_t = win.t.cpu(), _t(ref)
    assert got_t.dtype == ref_t.dtype and got_t.shape == ref_t.shape, (what, got_t.dtype, ref_t.dtype)
    got, want = O.bits(got_t), O.bits(ref_t)
    if not torch.equal(got, want):
        bad = (got != want).nonzero().flatten()
        i = int(bad[0])
        extra = f', worst {int(_ulps(got_t, ref_t).max())} ulp' if got_t.dtype == F32 else ''
        raise AssertionError(f'{what}: {bad.numel()} of {got.numel()} elements differ, first at {i}: got {float(got_t[i])!r} '
                             f'({int(got[i]) & 0xFFFFFFFF:#x}), want {float(ref_t[i])!r} ({int(want[i]) & 0xFFFFFFFF:#x}){extra}')


def _scalar_bits(t):
    return int(t.detach().cpu().view(torch.int32))


def _scalar_f32(t):
    return np.float32(t.detach().cpu().numpy())


# ================================================================================================================ Adam
def _pg(n):
    """test_adam_and_sgd_match_torch's inputs at any n"""
    return O.rnd(n, seed=41), O.rnd(n, seed=42, scale=0.1)


class AdamState:
    """device windows and the replica's arrays, stepped together"""

    def __init__(self, n, p0, mirror=True, m0=None, v0=None):
        z = np.zeros(n, np.float32)
        self.n = n
        self.rp, self.rm, self.rv = p0.numpy().copy(), (z if m0 is None else m0.numpy()), (z if v0 is None else v0.numpy())
        self.p, self.m, self.v = Win(n, F32, self.rp), Win(n, F32, self.rm), Win(n, F32, self.rv)
        self.mir = Win(n, BF16) if mirror else None

    def args(self, g_dev, step, lr=LR):
        return (self.p.t, g_dev, self.m.t, self.v.t, lr, B1, B2, EPS, step, 0.25, self.mir.t if self.mir else None)

    def replica(self, g_dev_host, step, clip=None, lr=LR):
        self.rp, self.rm, self.rv = O.adam_f32(self.rp, g_dev_host, self.rm, self.rv, lr, B1, B2, EPS, step, grad_scale=0.25, clip=clip)

    def check(self, what):
        torch.cuda.synchronize()
        _same(self.m, self.rm, f'{what} exp_avg')
        _same(self.v, self.rv, f'{what} exp_avg_sq')
        _same(self.p, self.rp, f'{what} param')
        if self.mir is not None:
            _same(self.mir, O.to_bf16(self.rp), f'{what} bf16 mirror')


@pytest.mark.parametrize('mirror', [True, False], ids=['mirror', 'no mirror'])
@pytest.mark.parametrize('n', O.ADAM_NS)
def test_adam_bitwise_at_every_size(ops, n, mirror):
    """steps 1, 2, 3 (non-zero moments from the second on), gradient g * step summed over 4 ranks with grad_scale 1/4"""
    p0, g = _pg(n)
    st = AdamState(n, p0, mirror)
    for step in (1, 2, 3):
        gh = g * (4 * step)
        st.replica(gh, step)
        ops.adam_step(*st.args(gh.to(DEV), step))
        st.check(f'adam n={n} step {step}')
    assert not np.array_equal(st.rp, p0.numpy())


def test_adam_late_step_bitwise(ops):
    """step 100000: both bias corrections have reached 1 in float32; moments of a run in progress"""
    n = O.P_ADAM + 7
    p0, g = _pg(n)
    st = AdamState(n, p0, True, m0=O.rnd(n, seed=43, scale=0.05), v0=O.rnd(n, seed=44, scale=0.05).square())
    gh = g * 4
    st.replica(gh, 100000)
    ops.adam_step(*st.args(gh.to(DEV), 100000))
    st.check(f'adam n={n} step 100000')


@pytest.mark.parametrize('mode', ['norm active', 'norm clamped', 'value'])
@pytest.mark.parametrize('n', O.ADAM_CLIP_NS)
def test_adam_clipped_bitwise(ops, n, mode):
    """norm mode reads the norm mts_grad_norm wrote on the device; the replica gets the coefficient formed from that norm's bits"""
    p0, g = _pg(n)
    st = AdamState(n, p0, True)
    ws, norm, coef = ops.grad_norm_workspace(DEV), torch.zeros((), device=DEV), torch.full((), -1.0, device=DEV)
    max_norm = {'norm active': 0.25 * float(g.double().norm()), 'norm clamped': 1e30, 'value': 0.0}[mode]
    for step in (1, 2, 3):
        gh = g * (4 * step)
        gd = gh.to(DEV)
        if mode == 'value':
            clip, kw = ('value', 0.1), dict(clip_value=0.1)
        else:
            ops.grad_norm(gd, [(0, n)], 0.25, ws, norm)
            c = O.clip_coef(_scalar_f32(norm), max_norm)
            assert (c == 1.0) if mode == 'norm clamped' else (0.0 < c < 0.26), c
            clip, kw = ('norm', c), dict(total_norm=norm, max_norm=max_norm, clip_coef_out=coef)
        st.replica(gh, step, clip)
        ops.adam_step_clipped(*st.args(gd, step), **kw)
        st.check(f'adam {mode} n={n} step {step}')
        if mode != 'value':
            assert _scalar_bits(coef) == int(np.float32(clip[1]).view(np.int32)), (float(coef), clip[1])
    if mode == 'value':
        assert float(coef) == -1.0                                      # no coefficient in value mode


@pytest.mark.parametrize('n', O.ADAM_F64_NS)
def test_adam_against_fp64(ops, n):
    """torch.optim.Adam on float64 copies, the bar of test_adam_and_sgd_match_torch: the bitwise replica and this reference cannot both drift"""
    p0, g = _pg(n)
    st = AdamState(n, p0, False)
    grads = [g * step for step in (1, 2, 3)]
    for step, gs in enumerate(grads, 1):
        ops.adam_step(*st.args((gs * 4).to(DEV), step))
    worst = O.within_bar(st.p.t.cpu(), O.adam_f64(p0, grads, LR))
    print(f'adam n={n}: {worst:.3f} of atol 1e-7 + rtol 1e-6')
    assert st.p.guards_intact() and worst <= 1.0, worst


# ================================================================================================================ SGD
SGD_LR = 0.01
SGD_FORMS = [('plain', True), ('plain', False), ('norm', True), ('value', True)]          # (entry point / clip mode, bf16 mirror)


@pytest.mark.parametrize('mom,wd', [(0.9, 1e-4), (0.0, 0.0)], ids=['momentum', 'bare'])
@pytest.mark.parametrize('n', O.SGD_NS)
def test_sgd_bitwise_at_every_size(ops, n, mom, wd):
    p0, g = _pg(n)
    ws, norm, coef = ops.grad_norm_workspace(DEV), torch.zeros((), device=DEV), torch.full((), -1.0, device=DEV)
    max_norm = 0.25 * float(g.double().norm())
    for form, mirror in SGD_FORMS:
        rp, rb = p0.numpy().copy(), np.zeros(n, np.float32)
        p, buf, mir = Win(n, F32, rp), Win(n, F32, rb), (Win(n, BF16) if mirror else None)
        for step in (1, 2, 3):
            gh = g * (4 * step)
            gd = gh.to(DEV)
            args = (p.t, gd, buf.t, SGD_LR, mom, wd, step == 1, 0.25, mir.t if mirror else None)
            clip = None
            if form == 'plain':
                ops.sgd_step(*args)
            elif form == 'value':
                clip = ('value', 0.1)
                ops.sgd_step_clipped(*args, clip_value=0.1)
            else:
                ops.grad_norm(gd, [(0, n)], 0.25, ws, norm)
                clip = ('norm', O.clip_coef(_scalar_f32(norm), max_norm))
                assert 0.0 < clip[1] < 0.26
                ops.sgd_step_clipped(*args, total_norm=norm, max_norm=max_norm, clip_coef_out=coef)
            rp, rb = O.sgd_f32(rp, gh, rb, SGD_LR, mom, wd, step == 1, grad_scale=0.25, clip=clip)
            what = f'sgd {form} n={n} momentum {mom} step {step}'
            torch.cuda.synchronize()
            _same(buf, rb, f'{what} momentum_buf')
            _same(p, rp, f'{what} param')
            if mirror:
                _same(mir, O.to_bf16(rp), f'{what} bf16 mirror')
            if form == 'norm':
                assert _scalar_bits(coef) == int(np.float32(clip[1]).view(np.int32))
        assert not np.array_equal(rp, p0.numpy())


@pytest.mark.parametrize('mom,wd', [(0.9, 1e-4), (0.0, 0.0)], ids=['momentum', 'bare'])
@pytest.mark.parametrize('n', O.SGD_F64_NS)
def test_sgd_against_fp64(ops, n, mom, wd):
    p0, g = _pg(n)
    p, buf = Win(n, F32, p0), Win(n, F32, torch.zeros(n))
    grads = [g * step for step in (1, 2, 3)]
    for step, gs in enumerate(grads, 1):
        ops.sgd_step(p.t, (gs * 4).to(DEV), buf.t, SGD_LR, mom, wd, step == 1, 0.25, None)
    worst = O.within_bar(p.t.cpu(), O.sgd_f64(p0, grads, SGD_LR, mom, wd))
    print(f'sgd n={n} momentum {mom}: {worst:.3f} of atol 1e-7 + rtol 1e-6')
    assert p.guards_intact() and worst <= 1.0, worst


# ================================================================================================================ the narrowing
@pytest.mark.parametrize('opt', ['adam', 'sgd'])
def test_bf16_mirror_is_one_round_to_nearest_even(ops, opt):
    """lr = 0 and a positive gradient: the update is +0 and p stays as it is (-0.0 included), so the mirror is bf16(p) of crafted values in the vector
    body and in the scalar tail: ties up and down to even, FLT_MAX -> inf, subnormals, -0.0"""
    n = O.NARROW_N
    vals = O.narrowing_values(n)
    g = O.rnd(n, seed=42, scale=0.1).abs() + 0.01
    p, mir = Win(n, F32, vals), Win(n, BF16)
    a, b = Win(n, F32, torch.zeros(n)), Win(n, F32, torch.zeros(n))
    if opt == 'adam':
        ops.adam_step(p.t, g.to(DEV), a.t, b.t, 0.0, B1, B2, EPS, 1, 1.0, mir.t)
    else:
        ops.sgd_step(p.t, g.to(DEV), a.t, 0.0, 0.9, 0.0, True, 1.0, mir.t)
    torch.cuda.synchronize()
    _same(p, vals, f'{opt} lr=0 param')
    _same(mir, O.to_bf16(vals), f'{opt} bf16 mirror of crafted values')
    assert a.guards_intact() and float(a.t.abs().max()) > 0             # the step ran


# ================================================================================================================ mts_scale
@pytest.mark.parametrize('n', O.SCALE_NS)
def test_scale_bitwise_at_every_size(ops, n):
    x = O.rnd(n, seed=n).numpy()
    for s in (0.5, 1.0 / 3.0, 3.0):
        w = Win(n, F32, x)
        ops.scale_(w.t, s)
        torch.cuda.synchronize()
        _same(w, x * np.float32(s), f'scale n={n} by {s}')


def test_scale_by_one_and_of_nothing_touch_nothing(ops, L):
    n = O.P_SCALE + 1
    w = Win(n, F32)                                                     # NaN patterns: x * 1.0f would quieten nothing, but a launch is not made at all
    L.check(L.lib.mts_scale(L.stream_ptr(), n, L.ptr(w.t), 1.0))
    ops.scale_(w.t, 1.0)
    L.check(L.lib.mts_scale(L.stream_ptr(), 0, L.ptr(w.t), 0.5))
    L.check(L.lib.mts_scale(L.stream_ptr(), 0, None, 0.5))
    ops.scale_(w.t[:0], 0.5)
    torch.cuda.synchronize()
    assert w.untouched()
    with pytest.raises(ValueError):
        L.check(L.lib.mts_scale(L.stream_ptr(), 4, None, 0.5))


# ================================================================================================================ mts_grad_norm
def _norm_twice(ops, g_dev, spans, scale):
    """two calls into a NaN-filled workspace: the result, after checking that the second call gave the same bits"""
    ws = ops.grad_norm_workspace(DEV).fill_(float('nan'))              # partials the launch does not write are never read
    a, b = torch.full((), -1.0, device=DEV), torch.full((), -2.0, device=DEV)
    ops.grad_norm(g_dev, spans, scale, ws, a)
    ops.grad_norm(g_dev, spans, scale, ws, b)
    assert _scalar_bits(a) == _scalar_bits(b)
    return float(a)


# the bar of tests/test_gpu_grad_clip.py: a lane adds at most a few tens of non-negative terms in sequence (here: up to 16 per running sum), the
# trees add about 20 levels: ~4e-6 on the sum, half on the root
NORM_REL = 1e-5


@pytest.mark.parametrize('scale', [1.0, 0.125])
@pytest.mark.parametrize('n', O.NORM_NS)
def test_grad_norm_three_and_four_trips(ops, n, scale):
    g = O.rnd(n, seed=n)
    ref = float(g.double().mul(scale).square().sum().sqrt())
    got = _norm_twice(ops, g.to(DEV), [(0, n)], scale)
    rel = abs(got - ref) / ref
    print(f'n {n} scale {scale}: got {got!r} ref {ref!r} rel {rel:.3e}')
    assert rel <= NORM_REL, (got, ref, rel)


@pytest.mark.parametrize('scale', [1.0, 0.125])
def test_grad_norm_four_spans_one_empty(ops, scale):
    spans, total = O.span_layout(O.NORM_SPAN_LENGTHS)
    g = O.rnd(total, seed=7)
    live = torch.cat([g[a:b] for a, b in spans])
    ref = float(live.double().mul(scale).square().sum().sqrt())
    edges = [0] + [x for ab in spans for x in ab] + [total]
    for k in range(0, len(edges), 2):                                   # what lies between and around the spans must not be read
        g[edges[k]:edges[k + 1]] = float('nan') if k % 4 == 0 else float('inf')
    assert torch.isfinite(torch.cat([g[a:b] for a, b in spans])).all() and not torch.isfinite(g[spans[0][1]])
    got = _norm_twice(ops, g.to(DEV), spans, scale)
    rel = abs(got - ref) / ref
    print(f'four spans scale {scale}: got {got!r} ref {ref!r} rel {rel:.3e}')
    assert rel <= NORM_REL, (got, ref, rel)


def test_grad_norm_refusals_come_before_any_launch(ops):
    g = torch.ones(64, device=DEV)
    ws = ops.grad_norm_workspace(DEV).fill_(float('nan'))
    out = torch.full((), 5.0, device=DEV)
    for spans in ([(0, 4), (4, 8), (8, 12), (12, 16), (16, 20)],        # n_spans = 5
                  [(0, 8), (9, 16)],                                    # a begin 4 bytes off a 16-byte boundary
                  [(2, 8)]):
        with pytest.raises(ValueError):
            ops.grad_norm(g, spans, 1.0, ws, out)
    torch.cuda.synchronize()
    assert float(out) == 5.0 and bool(torch.isnan(ws).all())


# ================================================================================================================ dropout
def _act(n, seed, dtype):
    return O.rnd(n, seed=seed).to(dtype)


def _mask_ref(kept):
    return torch.from_numpy(kept.astype(np.uint8))


@pytest.mark.parametrize('dtype', ACTS, ids=ACT_IDS)
@pytest.mark.parametrize('n', O.DROPOUT_NS)
def test_dropout_bitwise_at_every_size(ops, n, dtype):
    """p = 0.3, out of place: mask x residual, then the backward out of place and in place"""
    p = 0.3
    x, r, dy = _act(n, 1, dtype), _act(n, 2, dtype), _act(n, 3, dtype)
    xd, rd = x.to(DEV), r.to(DEV)
    kept = O.keep(n, p, SEED)
    for with_mask in (True, False):
        for with_res in (True, False):
            y, mask = Win(n, dtype), Win(n, U8)
            ops.dropout_fwd(xd, y.t, p, SEED, mask=mask.t if with_mask else None, residual=rd if with_res else None)
            torch.cuda.synchronize()
            what = f'dropout {dtype} n={n} mask={with_mask} residual={with_res}'
            _same(y, O.dropout_fwd_f32(x, kept, p, r if with_res else None), f'{what} y')
            if with_mask:
                _same(mask, _mask_ref(kept), f'{what} mask')
            else:
                assert mask.untouched()
    assert torch.equal(xd.cpu(), x) and torch.equal(rd.cpu(), r)      # the inputs are read only
    ref = O.dropout_bwd_f32(dy, kept, p)
    mask = Win(n, U8, _mask_ref(kept))
    dx = Win(n, dtype)
    ops.dropout_bwd(dy.to(DEV), dx.t, mask.t, p)
    inplace = Win(n, dtype, dy)
    ops.dropout_bwd(inplace.t, inplace.t, mask.t, p)
    torch.cuda.synchronize()
    _same(dx, ref, f'dropout_bwd {dtype} n={n}')
    _same(inplace, ref, f'dropout_bwd {dtype} n={n} in place')
    _same(mask, _mask_ref(kept), 'the mask after the backward')


@pytest.mark.parametrize('p', [0.3] + O.DROPOUT_EDGE_PS)
@pytest.mark.parametrize('dtype', ACTS, ids=ACT_IDS)
@pytest.mark.parametrize('n', O.DROPOUT_EDGE_NS)
def test_dropout_in_place_and_every_p(ops, n, dtype, p):
    """the forms the models call: y is x with and without a residual; and every p out of place (p = 0.3 out of place is the test above)"""
    x, r = _act(n, 1, dtype), _act(n, 2, dtype)
    x[5], x[n - 2] = -0.0, -0.0                                         # vector body and last vector
    rd = r.to(DEV)
    kept = O.keep(n, p, SEED)
    if p == 0.0:
        assert kept.all()
    for with_res in (True, False):
        ref = O.dropout_fwd_f32(x, kept, p, r if with_res else None)
        what = f'dropout {dtype} n={n} p={p} residual={with_res}'
        xy, mask = Win(n, dtype, x), Win(n, U8)
        ops.dropout_fwd(xy.t, xy.t, p, SEED, mask=mask.t, residual=rd if with_res else None)
        torch.cuda.synchronize()
        _same(xy, ref, f'{what} in place')
        _same(mask, _mask_ref(kept), f'{what} in place, mask')
        if p != 0.3:
            y = Win(n, dtype)
            ops.dropout_fwd(x.to(DEV), y.t, p, SEED, mask=None if with_res else mask.t, residual=rd if with_res else None)
            torch.cuda.synchronize()
            _same(y, ref, f'{what} out of place')
        if p == 0.0 and not with_res:
            # nothing is dropped and the scale is 1: y is x bit for bit, except that (-0.0 * 1) + 0 is +0.0 -- the replica decides that one
            neg0 = O.bits(x) == O.bits(torch.tensor(-0.0, dtype=dtype))
            assert neg0.sum() == 2 and torch.equal(O.bits(ref)[~neg0], O.bits(x)[~neg0]) and not bool(O.bits(ref)[neg0].any())
    dy = _act(n, 3, dtype)
    dd = Win(n, dtype, dy)
    mask = Win(n, U8, _mask_ref(kept))
    ops.dropout_bwd(dd.t, dd.t, mask.t, p)
    torch.cuda.synchronize()
    _same(dd, O.dropout_bwd_f32(dy, kept, p), f'dropout_bwd {dtype} n={n} p={p} in place')


@pytest.mark.parametrize('n', [1028, O.P_DROPOUT + 4])
def test_dropout_seeds(ops, n):
    """seed 0, a seed above 2^62 and the largest one; the same seed gives the same bits, another seed another mask"""
    x = _act(n, 1, F32)
    xd = x.to(DEV)
    masks = []
    for seed in (0, (1 << 62) + 987654321, (1 << 64) - 1):
        kept = O.keep(n, 0.3, seed)
        runs = []
        for _ in range(2):
            y, mask = Win(n, F32), Win(n, U8)
            ops.dropout_fwd(xd, y.t, 0.3, seed, mask=mask.t)
            torch.cuda.synchronize()
            _same(y, O.dropout_fwd_f32(x, kept, 0.3), f'dropout n={n} seed {seed} y')
            _same(mask, _mask_ref(kept), f'dropout n={n} seed {seed} mask')
            runs.append((y, mask))
        assert torch.equal(runs[0][0].buf, runs[1][0].buf) and torch.equal(runs[0][1].buf, runs[1][1].buf)
        masks.append(runs[0][1].t.clone())
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2]) and not torch.equal(masks[0], masks[2])


@pytest.mark.parametrize('dtype', ACTS, ids=ACT_IDS)
def test_dropout_refusals_come_before_any_launch(ops, dtype):
    n = 1028
    x = _act(n, 1, dtype).to(DEV)
    y, mask, dx = Win(n, dtype), Win(n, U8), Win(n, dtype)
    for p in (1.0, 1.5, -0.1, float('nan')):
        with pytest.raises(ValueError):
            ops.dropout_fwd(x, y.t, p, SEED, mask=mask.t)
        with pytest.raises(ValueError):
            ops.dropout_bwd(x, dx.t, mask.t, p)
    with pytest.raises(ValueError):                                      # n % 4 != 0
        ops.dropout_fwd(x[:n - 2], y.t[:n - 2], 0.3, SEED, mask=mask.t[:n - 2])
    with pytest.raises(ValueError):
        ops.dropout_bwd(x[:n - 2], dx.t[:n - 2], mask.t[:n - 2], 0.3)
    with pytest.raises(ValueError):                                      # the backward needs its mask
        ops.dropout_bwd(x, dx.t, None, 0.3)
    torch.cuda.synchronize()
    assert y.untouched() and mask.untouched() and dx.untouched()


# ================================================================================================================ alignment
ALIGN_N = 1028


@pytest.mark.parametrize('entry', ['plain', 'clipped'])
@pytest.mark.parametrize('which', ['param', 'grad', 'exp_avg', 'exp_avg_sq', 'bf16_copy'])
def test_adam_refuses_a_pointer_off_its_vector_boundary(ops, which, entry):
    """a slice flat[1 : 1 + n] of an aligned buffer: 4 bytes off the 16-byte boundary (2 bytes off the mirror's 8)"""
    n = ALIGN_N
    wins = {k: Win(n, BF16 if k == 'bf16_copy' else F32) for k in ('param', 'grad', 'exp_avg', 'exp_avg_sq', 'bf16_copy')}
    t = {k: w.t for k, w in wins.items()}
    assert all(v.data_ptr() % 16 == 0 for v in t.values())
    buf, t[which] = _off_by_one(n, BF16 if which == 'bf16_copy' else F32)
    assert t[which].data_ptr() % (8 if which == 'bf16_copy' else 16) != 0
    args = (t['param'], t['grad'], t['exp_avg'], t['exp_avg_sq'], LR, B1, B2, EPS, 1, 1.0, t['bf16_copy'])
    with pytest.raises(ValueError, match='aligned'):
        ops.adam_step(*args) if entry == 'plain' else ops.adam_step_clipped(*args, clip_value=0.1)
    torch.cuda.synchronize()
    assert all(w.untouched() for w in wins.values()) and bool((buf == buf[0]).all())


@pytest.mark.parametrize('entry', ['plain', 'clipped'])
@pytest.mark.parametrize('which', ['param', 'grad', 'momentum_buf', 'bf16_copy'])
def test_sgd_refuses_a_pointer_off_its_element_size(L, which, entry):
    """SGD works element by element, so only an address that is no multiple of the element size is refused: no tensor slice has one, the raw
    pointer is moved by half an element (and stays inside its window; the call never reaches a launch)"""
    n = ALIGN_N
    wins = {k: Win(n, BF16 if k == 'bf16_copy' else F32) for k in ('param', 'grad', 'momentum_buf', 'bf16_copy')}
    a = {k: w.t.data_ptr() for k, w in wins.items()}
    a[which] += 1 if which == 'bf16_copy' else 2
    head = (L.stream_ptr(), n - 4, a['param'], a['grad'], a['momentum_buf'], 0.01, 0.9, 1e-4, 1, 1.0, a['bf16_copy'])
    rc = L.lib.mts_sgd_step(*head) if entry == 'plain' else L.lib.mts_sgd_step_clipped(*head, None, 0.0, 0.1, None)
    with pytest.raises(ValueError, match='aligned'):
        L.check(rc)
    torch.cuda.synchronize()
    assert all(w.untouched() for w in wins.values())


@pytest.mark.parametrize('dtype', ACTS, ids=ACT_IDS)
@pytest.mark.parametrize('which', ['x', 'residual', 'y', 'mask', 'dy', 'dx', 'bwd mask'])
def test_dropout_refuses_a_pointer_off_its_vector_boundary(ops, which, dtype):
    """one element off: 4 (fp32) or 2 (bf16) bytes off the 4-element boundary of the data, 1 byte off the mask's word"""
    n = ALIGN_N
    wins = {k: Win(n, U8 if 'mask' in k else dtype) for k in ('x', 'residual', 'y', 'mask', 'dy', 'dx', 'bwd mask')}
    t = {k: w.t for k, w in wins.items()}
    buf, t[which] = _off_by_one(n, U8 if 'mask' in which else dtype)
    assert t[which].data_ptr() % (4 if 'mask' in which else 4 * t[which].element_size()) != 0
    with pytest.raises(ValueError, match='aligned'):
        if which in ('x', 'residual', 'y', 'mask'):
            ops.dropout_fwd(t['x'], t['y'], 0.3, SEED, mask=t['mask'], residual=t['residual'])
        else:
            ops.dropout_bwd(t['dy'], t['dx'], t['bwd mask'], 0.3)
    torch.cuda.synchronize()
    assert all(w.untouched() for w in wins.values()) and bool((buf == buf[0]).all())
