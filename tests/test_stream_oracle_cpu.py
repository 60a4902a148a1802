"""CPU pins of tests/stream_oracle.py, the bitwise float32 replicas that tests/test_gpu_stream_regimes.py compares the kernels of csrc/optim.hip and
csrc/dropout.hip with: the replicas against torch's own optimizers in fp64 (so that a replica cannot copy a kernel's bug), the hash against plain
Python integers, and the size ladders against the regimes they are there for, asserted from the launch constants."""
import numpy as np
import pytest
import torch

from tests import stream_oracle as O

N = 10007
STEPS = 20
LR_ADAM, LR_SGD, MOM, WD = 1e-3, 0.01, 0.9, 1e-4


def _inputs():
    """test_adam_and_sgd_match_torch's: seeds 41 / 42; the device gradient is a SUM over 4 ranks, grad_scale 1/4 restores g exactly"""
    return O.rnd(N, seed=41), O.rnd(N, seed=42, scale=0.1)


def _norm_clip(g_dev, scale, max_norm):
    """the float32 norm a device reduction would hand over (here: the fp64 norm narrowed) -> the replica's clip argument"""
    norm = np.float32(float(g_dev.double().mul(scale).norm()))
    return ('norm', O.clip_coef(norm, max_norm))


def _run_adam(p0, grads, clip32):
    p, m, v, coefs = p0.numpy(), np.zeros(N, np.float32), np.zeros(N, np.float32), []
    for step, gs in enumerate(grads, 1):
        gd = gs * 4
        c = clip32(gd)
        coefs.append(float(c[1]) if c else None)
        p, m, v = O.adam_f32(p, gd, m, v, LR_ADAM, 0.9, 0.999, 1e-7, step, grad_scale=0.25, clip=c)
    return p, coefs


def _adam_case(name, clip64, clip32):
    """Adam as in test_adam_and_sgd_match_torch (gradient g * step), over 20 steps"""
    p0, g = _inputs()
    grads = [g * step for step in range(1, STEPS + 1)]
    ref = O.adam_f64(p0, grads, LR_ADAM, clip64)
    p, coefs = _run_adam(p0, grads, clip32)
    worst = O.within_bar(p, ref)
    print(f'adam {name}: {worst:.3f} of atol 1e-7 + rtol 1e-6 after {STEPS} steps')
    assert float((torch.from_numpy(p).double() - p0.double()).abs().max()) > 1e-3      # the steps moved the parameters
    assert worst <= 1.0, worst
    return coefs


def test_adam_f32_against_torch_adam_in_fp64():
    _adam_case('plain', None, lambda gd: None)


def test_adam_f32_norm_mode_against_clip_grad_norm():
    """max_norm = 5.5 ||g||: the gradient g * step is left alone for five steps (coefficient clamped to 1) and clipped from the sixth on.
    A max_norm below ||g|| would clip EVERY step to one and the same gradient; Adam's update of such a gradient is lr exactly, and subtracting the
    same 0.001 from a float32 near 1 is off by the same 0.4 ulp every step: a drift of float32 itself (torch's float32 Adam has it too) that
    uses up the whole bar in 20 steps and says nothing about the replica."""
    _, g = _inputs()
    max_norm = 5.5 * float(g.double().norm())
    coefs = _adam_case('norm', ('norm', max_norm), lambda gd: _norm_clip(gd, 0.25, max_norm))
    assert coefs[:5] == [1.0] * 5 and all(c < 1.0 for c in coefs[5:]) and abs(coefs[-1] - 5.5 / 20) < 1e-4


def test_adam_f32_value_mode_against_clip_grad_value():
    _, g = _inputs()
    assert 0.1 < float((g.abs() * STEPS > 0.1).float().mean()) and float((g.abs() > 0.1).float().mean()) < 0.9
    _adam_case('value', ('value', 0.1), lambda gd: ('value', 0.1))


@pytest.mark.parametrize('mode', ['plain', 'norm', 'value'])
def test_sgd_f32_against_torch_sgd_in_fp64(mode, mom=MOM, wd=WD):
    """SGD as in test_adam_and_sgd_match_torch (the same gradient g every step, momentum 0.9, weight decay 1e-4), over 20 steps; the clip settings
    of tests/test_gpu_grad_clip.py.  (Without momentum the same gradient gives the same update 20 times, and float32 rounds p - lr g the same way
    each time: up to 20 half-ulps, 1.2e-6 |p|, past the bar by float32's own doing.  The GPU file compares that form with fp64 over 3 steps.)"""
    p0, g = _inputs()
    max_norm = 0.25 * float(g.double().norm())
    clip64 = {'plain': None, 'norm': ('norm', max_norm), 'value': ('value', 0.1)}[mode]
    clip32 = {'plain': lambda gd: None, 'norm': lambda gd: _norm_clip(gd, 0.25, max_norm), 'value': lambda gd: ('value', 0.1)}[mode]
    grads = [g] * STEPS
    ref = O.sgd_f64(p0, grads, LR_SGD, mom, wd, clip64)
    p, buf = p0.numpy(), np.zeros(N, np.float32)
    for step, gs in enumerate(grads, 1):
        gd = gs * 4
        c = clip32(gd)
        if mode == 'norm':
            assert abs(float(c[1]) - 0.25) < 1e-4            # clipping acts
        p, buf = O.sgd_f32(p, gd, buf, LR_SGD, mom, wd, step == 1, grad_scale=0.25, clip=c)
    worst = O.within_bar(p, ref)
    print(f'sgd {mode} momentum {mom}: {worst:.3f} of atol 1e-7 + rtol 1e-6 after {STEPS} steps')
    assert float((torch.from_numpy(p).double() - p0.double()).abs().max()) > 1e-3
    assert worst <= 1.0, worst


def test_clip_coef_clamps_at_one_and_keeps_nan():
    assert O.clip_coef(2.0, 1.0) == np.float32(1.0) / (np.float32(2.0) + np.float32(1e-6))
    assert O.clip_coef(0.5, 1.0) == np.float32(1.0) and O.clip_coef(0.0, 0.0) == np.float32(0.0)
    assert np.isnan(O.clip_coef(float('nan'), 1.0))
    assert O.clip_coef(float('inf'), 1.0) == 0.0
    g = np.array([0.5, -0.5, 0.05, float('nan'), -0.0], np.float32)
    got = O._clip(g, ('value', 0.1))
    assert np.array_equal(got[:3], np.array([0.1, -0.1, 0.05], np.float32)) and np.isnan(got[3]) and np.signbit(got[4])


def test_adam_bias_corrections_come_from_the_float32_betas():
    bc1, bc2s = O.adam_bias(0.9, 0.999, 1)
    assert bc1 == np.float32(1.0 - float(np.float32(0.9))) and bc1 != np.float32(1.0 - 0.9)
    assert bc2s == np.float32(np.sqrt(1.0 - float(np.float32(0.999))))
    assert O.adam_bias(0.9, 0.999, 100000) == (np.float32(1.0), np.float32(1.0))


# ---------------------------------------------------------------------------------------------------------------- the hash
def _hash_int(seed, idx):
    M = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z = z ^ (z >> 31)
    return z >> 32


@pytest.mark.parametrize('seed,first', [(123456789, 0), (0, 0), ((1 << 62) + 12345, (1 << 32) - 40), ((1 << 64) - 1, 7), (99, (1 << 32) - 1)])
def test_hash_against_python_integers(seed, first):
    got = O.hash32(64, seed, first)
    want = [_hash_int(seed, first + i) for i in range(64)]
    assert got.dtype == np.uint32 and got.tolist() == want
    thr = O.threshold(0.3)
    assert O.keep(64, 0.3, seed, first).tolist() == [w >= thr for w in want]


def test_threshold_is_formed_from_the_float32_p():
    assert O.threshold(0.3) - int(0.3 * 4294967296.0) == 52           # float32(0.3) = 0.300000011920929
    assert O.threshold(0.3) == int(float(np.float32(0.3)) * 2 ** 32)
    assert O.threshold(0.0) == 0 and O.threshold(0.5) == 1 << 31
    assert O.threshold(0.999) < (1 << 32) - 1
    assert O.dropout_scale(0.3) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))
    assert O.dropout_scale(0.0) == 1.0 and O.dropout_scale(0.5) == 2.0


@pytest.mark.parametrize('p', [0.1, 0.3, 0.5, 0.999])
def test_keep_fraction(p):
    n = 1 << 20
    k = O.keep(n, p, 123456789)
    q = 1.0 - float(np.float32(p))
    sd = (q * (1 - q) / n) ** 0.5
    print(f'p {p}: kept {k.mean():.6f}, expected {q:.6f}, {abs(k.mean() - q) / sd:.2f} standard deviations')
    assert abs(k.mean() - q) <= 4 * sd


def test_p_zero_keeps_everything_and_seeds_differ():
    assert O.keep(1 << 20, 0.0, 5).all()
    a, b = O.keep(4096, 0.3, 1), O.keep(4096, 0.3, 2)
    assert not np.array_equal(a, b) and np.array_equal(a, O.keep(4096, 0.3, 1))
    assert np.array_equal(O.keep(100, 0.3, 1, first=17), a[17:117])


def test_dropout_replicas():
    x = torch.tensor([1.5, -2.0, -0.0, 3.0])
    r = torch.tensor([0.25, 0.25, 0.0, -1.0])
    k = np.array([True, False, True, True])
    s = float(O.dropout_scale(0.5))
    y = O.dropout_fwd_f32(x, k, 0.5, r)
    assert y.tolist() == [1.5 * s + 0.25, 0.25, 0.0, 3.0 * s - 1.0]
    assert not np.signbit(y.numpy()[2])                                # (-0.0 * scale) + 0.0 = +0.0: the replica decides
    assert O.dropout_bwd_f32(x, k, 0.5).tolist() == [3.0, 0.0, -0.0, 6.0]
    # bf16: one rounding, of the float32 sum
    xb = torch.tensor([1.0078125, 1.0]).to(torch.bfloat16)
    rb = torch.tensor([0.00390625, 0.0]).to(torch.bfloat16)
    yb = O.dropout_fwd_f32(xb, np.array([True, True]), 0.0, rb)
    assert yb.dtype == torch.bfloat16 and yb.float().tolist() == [1.015625, 1.0]     # 1.01171875 is a tie: to even


def test_narrowing_values_hold_every_case_in_body_and_tail():
    v = O.narrowing_values()
    u = v.view(np.uint32)
    body, tail = u[:O.NARROW_N // 4 * 4], u[O.NARROW_N // 4 * 4:]
    assert len(tail) == 3
    for want in (0x3F808000, 0x3F818000, 0x7F7FFFFF, 0x00000001, 0x80000000):
        assert want in body
    assert {0x3F808000, 0x3F818000, 0x7F7FFFFF, 0x00000001, 0x80000000} <= set(u[-19:].tolist())     # one whole cycle ends in the tail
    b = O.to_bf16(v).view(torch.int16).numpy().view(np.uint16)
    first = dict(zip(u[:19].tolist(), b[:19].tolist()))
    assert first[0x3F808000] == 0x3F80 and first[0x3F818000] == 0x3F82 and first[0x3F808001] == 0x3F81 and first[0x3F817FFF] == 0x3F81
    assert first[0x7F7FFFFF] == 0x7F80 and first[0xFF7FFFFF] == 0xFF80 and first[0x7F7F7FFF] == 0x7F7F
    assert first[0x00000001] == 0 and first[0x00008000] == 0 and first[0x00018000] == 2 and first[0x007FFFFF] == 0x0080
    assert first[0x80000000] == 0x8000


# ---------------------------------------------------------------------------------------------------------------- the ladders
def test_launch_constants():
    assert (O.P_ADAM, O.P_SGD, O.P_SCALE, O.P_DROPOUT, O.P_NORM) == (2097152, 524288, 262144, 4194304, 2097152)
    assert O.ADAM_NS == [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 10007, 2097152, 2097153, 2097159, 4198403]
    assert O.SGD_NS == [1, 255, 256, 257, 524288, 524289, 1200131]
    assert O.SCALE_NS == [1, 257, 262144, 262145, 700001]
    assert O.DROPOUT_NS == [4, 8, 1020, 1024, 1028, 40960, 4194304, 4194308, 9437188]
    assert O.NORM_NS == [4194308, 4194311, 6291460, 6292485]
    assert max(O.ADAM_NS + O.SGD_NS + O.SCALE_NS + O.DROPOUT_NS + O.NORM_NS) < 13_000_000


def _regimes(ns, per_pass, vec):
    """which of the stated regimes a ladder holds"""
    return {'tail only': any(0 < n < vec for n in ns) if vec > 1 else True,
            'one trip exact': per_pass in ns,
            'one into the next trip': per_pass + vec in ns or per_pass + 1 in ns,
            'three trips with a tail': any(O.trips(n, per_pass) == 3 and (n % 4 if vec > 1 else n % O.THREADS) for n in ns)}


@pytest.mark.parametrize('name,ns,per_pass,vec', [('adam', O.ADAM_NS, O.P_ADAM, O.ADAM_VEC), ('sgd', O.SGD_NS, O.P_SGD, 1),
                                                  ('scale', O.SCALE_NS, O.P_SCALE, 1)])
def test_ladders_hold_every_regime(name, ns, per_pass, vec):
    missing = [k for k, ok in _regimes(ns, per_pass, vec).items() if not ok]
    assert not missing, (name, missing)
    assert all(O.trips(n, per_pass) <= 3 for n in ns)


def test_adam_ladder_details():
    ns = O.ADAM_NS
    assert {1, 2, 3} <= set(ns)                                        # the scalar tail alone, every length
    assert 4 in ns and 5 in ns and 7 in ns                             # one vector; a vector and a tail of 1 and of 3
    assert 1023 in ns and 1024 in ns and 1025 in ns                    # either side of one workgroup's 256 x 4
    assert O.P_ADAM + 1 in ns                                          # the second trip is a tail alone
    assert O.P_ADAM + 7 in ns                                          # the second trip: lane 0 a vector, lane 1 the tail
    big = ns[-1]
    assert O.trips(big, O.P_ADAM) == 3 and big % 4 == 3 and (big - 2 * O.P_ADAM) // 4 > O.THREADS  # more than one workgroup in the third trip
    assert set(O.ADAM_CLIP_NS) <= set(ns) and set(O.ADAM_F64_NS) <= set(ns) and set(O.SGD_F64_NS) <= set(O.SGD_NS)


def test_dropout_ladder_details():
    ns = O.DROPOUT_NS
    assert all(n % 4 == 0 for n in ns)
    assert 4 in ns and O.P_DROPOUT in ns and O.P_DROPOUT + 4 in ns
    assert 1020 in ns and 1024 in ns and 1028 in ns
    assert O.trips(ns[-1], O.P_DROPOUT) == 3 and ns[-1] % 1024 != 0
    assert set(O.DROPOUT_EDGE_NS) <= set(ns) and 0.0 in O.DROPOUT_EDGE_PS


def _norm_trips(n):
    """loads of lane 0 of grad_sumsq_kernel: (pairs, singles)"""
    nv, i, pairs = n // 4 * 4, 0, 0
    while i + O.P_NORM < nv:
        pairs, i = pairs + 1, i + 2 * O.P_NORM
    return pairs, int(i < nv)


def test_norm_ladder_details():
    assert [_norm_trips(n) for n in O.NORM_NS] == [(1, 1), (1, 1), (2, 0), (2, 0)]
    assert [n % 4 for n in O.NORM_NS] == [0, 3, 0, 1]
    assert len(O.NORM_SPAN_LENGTHS) == O.NORM_MAX_SPANS and 0 in O.NORM_SPAN_LENGTHS[1:-1]
    assert _norm_trips(O.NORM_SPAN_LENGTHS[0]) == (1, 1)
    spans, total = O.span_layout(O.NORM_SPAN_LENGTHS)
    assert [b - a for a, b in spans] == O.NORM_SPAN_LENGTHS and all(a % 4 == 0 for a, _ in spans)
    assert all(spans[i + 1][0] - spans[i][1] >= 12 for i in range(3)) and spans[0][0] >= 4 and total - spans[-1][1] >= 12
