"""fp64 oracle of mts_gemm's epilogue and the error bound its kernels must meet (plain torch, runs on the CPU).

Order of operations = the one epi_math4 (csrc/gemm_common.h) documents:

    v = op(A) . op(B);  v += bias;  v[:, :ncols_scaled] *= colscale;  v += residual;  pre = v;  out = act(v);  out += base

Operands are taken AS STORED (bf16 or fp32 tensors) and upcast to fp64, so the only error a kernel may add is its fp32
accumulation, the epilogue's fp32 arithmetic and the final rounding of a bf16 store.

Error bound (derived, never measured on the code under test).  Products of two bf16 numbers are exact in fp32.  A length-K fp32
sum in any order plus the epilogue's adds is within

    E = (K + 4) * 2^-23 * S,    S = (|op(A)| . |op(B)| + |bias|) [scaled columns: * |colscale|] + |residual| (+ |base|)

(2^-23 instead of the unit roundoff 2^-24: independent of the matrix core's internal rounding mode).  With an activation
(erf-GELU is 1.13-Lipschitz, ReLU 1-Lipschitz):  1.13 E + 2^-21 (1 + |pre|), the second term for fp32 erff and the 1 + erf
cancellation.  A bf16 store adds one round-to-nearest:  bound + 2^-8 (|ref| + bound).  fp32 operands: the same formula with the
kernel's own K (every product is rounded once, which the factor of two already covers).
"""
import torch

from oracle import restatement as R

LAYOUTS = ('NT', 'NN', 'TN', 'TT')

# name -> (bias, residual, colscale, act, aux, accumulate); the two accumulating ones exist with fp32 C only
EPILOGUES = {
    'none': (0, 0, 0, None, 0, 0),
    'bias': (1, 0, 0, None, 0, 0),
    'res': (0, 1, 0, None, 0, 0),
    'bias+res': (1, 1, 0, None, 0, 0),
    'bias+cs': (1, 0, 1, None, 0, 0),
    'bias+cs+res': (1, 1, 1, None, 0, 0),
    'bias+gelu+aux': (1, 0, 0, 'gelu', 1, 0),
    'bias+relu+aux': (1, 0, 0, 'relu', 1, 0),
    'gelu': (0, 0, 0, 'gelu', 0, 0),
    'bias+res+gelu+aux': (1, 1, 0, 'gelu', 1, 0),
    'accum': (0, 0, 0, None, 0, 1),
    'bias+accum': (1, 0, 0, None, 0, 1),
}
COLSCALE = 0.25

# the shapes of tests/test_gpu_gemm_epilogue.py, by leg: (M, N, K, first tile boundary of the kernel under test)
SHAPES = {
    'f32': [(72, 132, 40, 128), (136, 130, 72, 128)],
    '128': [(136, 136, 64, 128), (136, 136, 200, 128), (136, 132, 64, 128), (136, 130, 64, 128)],
    '256': [(264, 264, 256, 256), (264, 260, 256, 256)],
    '224': [(512, 448, 256, 224), (264, 448, 320, 224)],
}


def ncols_values(N, tile):
    """Column-scale boundaries of a case: 0, N, inside the first tile (a multiple of 4 and not), the first tile boundary and 36 past it."""
    return sorted({v for v in (0, 100, 101, tile, tile + 36, N) if v <= N})


def op_a(layout, A):
    return A if layout in ('NT', 'NN') else A.t()          # [M, K]


def op_b(layout, B):
    return B.t() if layout in ('NT', 'TT') else B          # [K, N]


def make_operands(layout, M, N, K, dtype, seed=0):
    """randn activations, bias, residual and base; weights scaled by 0.2 -- bias / residual mistakes are O(1), rounding O(1e-2).
    Returned as stored: A is [M, K] (NT, NN) or [K, M]; B is [N, K] (NT, TT) or [K, N]."""
    g = torch.Generator().manual_seed(1000 + seed)
    a = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * 0.2).to(dtype)
    return dict(A=(a if layout in ('NT', 'NN') else a.t().contiguous()), B=(w if layout in ('NT', 'TT') else w.t().contiguous()),
                bias=torch.randn(N, generator=g), residual=torch.randn(M, N, generator=g).to(dtype), base=torch.randn(M, N, generator=g))


def product(layout, A, B):
    """(op(A) . op(B), |op(A)| . |op(B)|) in fp64: the part of reference() that does not depend on the epilogue."""
    a, b = op_a(layout, A.double()), op_b(layout, B.double())
    return a @ b, a.abs() @ b.abs()


def reference(layout, A, B, *, bias=None, residual=None, colscale=None, ncols_scaled=0, act=None, base=None, prod=None):
    """-> (pre, out, S), all fp64 [M, N].  prod: a cached product(layout, A, B)."""
    v, S = prod if prod is not None else product(layout, A, B)
    v, S = v.clone(), S.clone()
    if bias is not None:
        v += bias.double()
        S += bias.double().abs()
    if colscale is not None:
        v[:, :ncols_scaled] *= float(colscale)
        S[:, :ncols_scaled] *= abs(float(colscale))
    if residual is not None:
        v += residual.double()
        S += residual.double().abs()
    pre = v
    if act == 'gelu':
        out = R.gelu_erf(v)
    elif act == 'relu':
        out = torch.clamp_min(v, 0.0)
    else:
        assert act is None
        out = v.clone()
    if base is not None:
        out = out + base.double()
        S += base.double().abs()
    return pre, out, S


def bound(S, K, ref, *, act=False, pre=None, bf16=False):
    """Element-wise limit of |got - ref| for a value whose absolute sum is S; act: ref went through GELU / ReLU of `pre`."""
    b = (K + 4) * 2.0 ** -23 * S
    if act:
        b = 1.13 * b + 2.0 ** -21 * (1.0 + pre.abs())
    if bf16:
        b = b + 2.0 ** -8 * (ref.abs() + b)
    return b


def case_reference(ops, layout, epi, ncols_scaled, prod=None):
    """reference() of a named epilogue on make_operands() output."""
    has_bias, has_res, has_cs, act, _, accum = EPILOGUES[epi]
    return reference(layout, ops['A'], ops['B'], bias=ops['bias'] if has_bias else None, residual=ops['residual'] if has_res else None,
                     colscale=COLSCALE if has_cs else None, ncols_scaled=ncols_scaled, act=act, base=ops['base'] if accum else None, prod=prod)
