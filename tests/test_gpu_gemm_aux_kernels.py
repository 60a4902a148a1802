"""The small kernels next to the GEMMs (csrc/gemm.hip: mts_cast, mts_cast_concat, mts_colsum; csrc/norm.hip: mts_gelu_bwd, mts_relu_bwd)
against plain torch / fp64 at the sizes where they change path: vector body and scalar tail, column windows, fewer rows than row
slices, and lengths past one pass of the capped grid (2048 blocks x 256 threads x 4 elements), where the grid-stride loop runs.
"""
import pytest
import torch

from oracle import restatement as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ONE_PASS = 2048 * 256 * 4            # elements one pass of the capped grids covers
NAN_BITS = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC00DEA)}
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope='module')
def ops():
    from multimodaltopicsegmentation_amd import ops as o
    return o


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _sentinel(n, dtype):
    it, bits = NAN_BITS[dtype]
    return torch.full((n,), bits, dtype=it, device=DEV)


def _bits(t):
    return t.view(NAN_BITS[t.dtype][0])


def _rounding_edges():
    """fp32 values at and next to bf16 rounding midpoints (ties go to the even mantissa: 0x3F80 is even, 0x3F81 odd), a mantissa carry into the
    exponent (0x407F), the largest finite values (round up to infinity), signed zeros and infinities."""
    import numpy as np
    hi = np.array([0x3F80, 0x3F81, 0x4000, 0x407F, 0xC2FE, 0xBF81, 0x7F7F, 0x0080], dtype=np.uint32)
    lo = np.array([0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    bits = ((hi[:, None] << 16) | lo[None, :]).reshape(-1)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000], dtype=np.uint32)              # +0, -0, +inf, -inf
    return torch.from_numpy(np.concatenate([bits, special]).view(np.float32).copy())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027, ONE_PASS + 7])
def test_cast_is_round_to_nearest_even_bit_for_bit(ops, dtype, n):
    src = _rnd(n, seed=40 + n % 7)
    edges = _rounding_edges()
    k = min(n, edges.numel())
    src[:k] = edges[:k]
    if n > 2 * edges.numel():
        src[-edges.numel():] = edges                      # ... and in the scalar tail / the last vector
    buf = _sentinel(n + 8, dtype)
    dst = buf.view(dtype)[:n]
    sd = src.to(DEV)
    ops.cast(sd, dst)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst.cpu()), _bits(src.to(dtype)))
    assert bool((buf[n:] == NAN_BITS[dtype][1]).all()), 'written past the end'
    assert torch.equal(sd.cpu().view(torch.int32), src.view(torch.int32))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,D1,D2', [(1, 4, 4), (37, 8, 20), (300, 768, 1024)])
def test_cast_concat_bitwise(ops, dtype, rows, D1, D2):
    x1, x2 = _rnd(rows, D1, seed=51), _rnd(rows, D2, seed=52)
    edges = _rounding_edges()
    k = min(edges.numel(), x2.numel())
    x2.view(-1)[:k] = edges[:k]
    buf = _sentinel(rows * (D1 + D2) + 8, dtype)
    dst = buf.view(dtype)[:rows * (D1 + D2)].view(rows, D1 + D2)
    ops.cast_concat(x1.to(DEV), x2.to(DEV), dst)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst.cpu()), _bits(torch.cat([x1, x2], 1).to(dtype)))
    assert bool((buf[rows * (D1 + D2):] == NAN_BITS[dtype][1]).all()), 'written past the end'


def test_cast_concat_refuses_widths_that_are_no_multiple_of_4(ops):
    x1, x2 = torch.zeros(3, 6, device=DEV), torch.zeros(3, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.cast_concat(x1, x2, torch.zeros(3, 14, device=DEV))
    with pytest.raises(ValueError):
        ops.cast_concat(x2, x1, torch.zeros(3, 14, device=DEV))


@pytest.mark.parametrize('accumulate', [False, True], ids=['overwrite', 'accumulate'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('M,N', [(1, 4), (5, 6), (127, 66), (129, 130), (1000, 264)])
def test_colsum_windows_tails_and_accumulate(ops, dtype, M, N, accumulate):
    """N % 4 != 0 takes the scalar column path for the last columns, M < 128 leaves row slices empty; X is a column window of a wider NaN-filled
    matrix.  Bound: fp32 sums of M terms in the kernel's fixed order, (M + 8) * 2^-23 * sum |x| per column (|out| included when accumulating)."""
    x = _rnd(M, N, seed=60 + N).to(dtype)
    ldx = (N + 3) // 4 * 4 + 8
    xbuf = torch.full((M + 2, ldx), float('nan'), dtype=dtype, device=DEV)
    xw = xbuf[:M, 4:4 + N]
    xw.copy_(x)
    out0 = _rnd(N, seed=61)
    ref = x.double().sum(0) + (out0.double() if accumulate else 0.0)
    lim = (M + 8) * 2.0 ** -23 * (x.double().abs().sum(0) + (out0.double().abs() if accumulate else 0.0))
    outs = []
    for _ in range(2):
        obuf = _sentinel(N + 4, torch.float32)
        out = obuf.view(torch.float32)[:N]
        out.copy_(out0 if accumulate else torch.full((N,), float('nan')))
        ops.colsum(xw, out, accumulate=accumulate)
        outs.append(obuf)
    torch.cuda.synchronize()
    got = outs[0].view(torch.float32)[:N].cpu().double()
    err = (got - ref).abs()
    print(f'colsum {dtype} {M}x{N} accumulate={accumulate}: largest err / bound {float(torch.nan_to_num(err / lim, nan=float("inf")).max()):.4f}')
    assert (err <= lim).all(), f'{int((~(err <= lim)).sum())}/{N} columns outside the bound'
    assert bool((outs[0][N:] == NAN_BITS[torch.float32][1]).all()), 'written past column N'
    assert torch.equal(outs[0], outs[1]), 'two calls differ'
    assert torch.equal(_bits(xw.cpu().contiguous()), _bits(x))


def _act_inputs(n, dtype, seed):
    u = _rnd(n, seed=seed, scale=2.0)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40, 1.0, -1.0], dtype=torch.float32)     # exact zeros, +-tiny (normal and subnormal)
    k = min(n, special.numel())
    u[:k] = special[:k]
    if n > ONE_PASS:
        u[ONE_PASS:ONE_PASS + k] = special[:k]            # ... and in the second pass of the grid-stride loop
    dy = _rnd(n, seed=seed + 1)
    dy[dy == 0] = 1.0
    return u.to(dtype), dy.to(dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [8, ONE_PASS + 4096])
def test_relu_bwd_bitwise(ops, dtype, n):
    """dy *= (u > 0): exact, so bit for bit; u = +-0 and u < 0 give +0, a positive subnormal keeps dy."""
    u, dy = _act_inputs(n, dtype, seed=70)
    ud, dyd = u.to(DEV), dy.to(DEV).clone()
    ops.relu_bwd(ud, dyd)
    torch.cuda.synchronize()
    ref = torch.where(u.float() > 0, dy, torch.zeros_like(dy))
    assert torch.equal(_bits(dyd.cpu()), _bits(ref))
    assert torch.equal(_bits(ud.cpu()), _bits(u))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [8, ONE_PASS + 4096])
def test_gelu_bwd_against_fp64(ops, dtype, n):
    """dy *= Phi(u) + u phi(u) against fp64, at the tolerance of test_gpu_kernels.py::test_gelu_bwd_and_head (the kernel's __expf has no
    derivable bound); the long size runs the grid-stride loop."""
    u, dy = _act_inputs(n, dtype, seed=80)
    ud, dyd = u.to(DEV), dy.to(DEV).clone()
    ops.gelu_bwd(ud, dyd)
    torch.cuda.synchronize()
    u64 = u.double().requires_grad_(True)
    R.gelu_erf(u64).backward(dy.double())
    ref = u64.grad
    rtol, atol = (1e-4, 1e-5) if dtype == torch.float32 else (1e-2, 1e-2)
    err = (dyd.cpu().double() - ref).abs()
    lim = atol + rtol * ref.abs()
    print(f'gelu_bwd {dtype} n={n}: largest err / tolerance {float(torch.nan_to_num(err / lim, nan=float("inf")).max()):.4f}')
    assert (err <= lim).all(), f'{int((~(err <= lim)).sum())}/{n} outside, largest err / tolerance {float((err / lim).max()):.3g}'
    assert torch.equal(_bits(ud.cpu()), _bits(u))


@pytest.mark.parametrize('fn', ['gelu_bwd', 'relu_bwd'])
def test_activation_backward_refuses_lengths_that_are_no_multiple_of_4(ops, fn):
    u, dy = torch.zeros(6, device=DEV), torch.ones(6, device=DEV)
    with pytest.raises(ValueError):
        getattr(ops, fn)(u, dy)
    assert bool((dy == 1).all())
