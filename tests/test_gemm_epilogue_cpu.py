"""The fp64 GEMM-epilogue oracle (tests/gemm_epilogue_oracle.py) and its error bound, checked without a GPU:

* the oracle against independent torch formulations (torch.addmm, F.gelu(approximate='none'), F.relu) for every epilogue and layout;
* torch's own fp32 evaluation of every case of tests/test_gpu_gemm_epilogue.py, rounded to bf16 where a kernel would round, stays
  inside the bound -- the bound is calibrated against the reference, never against the code under test;
* three wrong epilogues (column-scale boundary off by one, residual dropped on the last row, bias shifted by one column) leave it.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_epilogue_oracle as O

ALL_SHAPES = sorted({(leg, s) for leg, shapes in O.SHAPES.items() for s in shapes})
DTYPE_OF_LEG = lambda leg: torch.float32 if leg == 'f32' else torch.bfloat16  # noqa: E731


@functools.lru_cache(maxsize=4)
def _case(layout, M, N, K, dtype):
    ops = O.make_operands(layout, M, N, K, dtype)
    return ops, O.product(layout, ops['A'], ops['B'])


def _epilogues(c_is_f32):
    return [e for e, spec in O.EPILOGUES.items() if c_is_f32 or not spec[5]]


def _ncols(epi, N, tile):
    return O.ncols_values(N, tile) if O.EPILOGUES[epi][2] else [0]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('layout', O.LAYOUTS)
def test_oracle_matches_independent_torch_formulations(layout, dtype):
    M, N, K = 136, 130, 72
    ops, _ = _case(layout, M, N, K, dtype)
    A, B = ops['A'].double(), ops['B'].double()
    a = {'NT': A, 'NN': A, 'TN': A.mT, 'TT': A.mT}[layout]
    b = {'NT': B.mT, 'NN': B, 'TN': B, 'TT': B.mT}[layout]
    assert a.shape == (M, K) and b.shape == (K, N)
    abs_prod = torch.einsum('mk,kn->mn', a.abs(), b.abs())
    for epi, (has_bias, has_res, has_cs, act, _, accum) in O.EPILOGUES.items():
        for ncs in _ncols(epi, N, 128):
            pre, out, S = O.case_reference(ops, layout, epi, ncs)
            bias = ops['bias'].double() if has_bias else torch.zeros(N, dtype=torch.float64)
            scale = torch.ones(N, dtype=torch.float64)
            if has_cs:
                scale[:ncs] = O.COLSCALE
            v = torch.addmm(bias.expand(M, N), a, b) * scale
            s = (abs_prod + bias.abs()) * scale.abs()
            if has_res:
                v = v + ops['residual'].double()
                s = s + ops['residual'].double().abs()
            o = F.gelu(v, approximate='none') if act == 'gelu' else F.relu(v) if act == 'relu' else v
            if accum:
                o = o + ops['base'].double()
                s = s + ops['base'].double().abs()
            tol = 1e-13 * s + 1e-300
            assert ((pre - v).abs() <= tol).all(), (epi, ncs, 'pre')
            assert ((out - o).abs() <= tol).all(), (epi, ncs, 'out')
            assert ((S - s).abs() <= tol).all(), (epi, ncs, 'S')


def test_bound_terms():
    S, ref, pre = (torch.tensor([v], dtype=torch.float64) for v in (2.0, -3.0, -5.0))
    e = 68 * 2.0 ** -23 * 2.0
    assert O.bound(S, 64, ref).item() == e
    assert O.bound(S, 64, ref, act=True, pre=pre).item() == 1.13 * e + 2.0 ** -21 * 6.0
    assert O.bound(S, 64, ref, bf16=True).item() == e + 2.0 ** -8 * (3.0 + e)
    assert O.ncols_values(448, 224) == [0, 100, 101, 224, 260, 448] and O.ncols_values(132, 128) == [0, 100, 101, 128, 132]


def _fp32_eval(layout, ops, epi, ncs, c_dtype, a_dtype):
    """torch's fp32 evaluation of a case, rounded where a kernel rounds: aux to the activation dtype, C to its dtype."""
    has_bias, has_res, has_cs, act, _, accum = O.EPILOGUES[epi]
    v = O.op_a(layout, ops['A'].float()) @ O.op_b(layout, ops['B'].float())
    if has_bias:
        v = v + ops['bias']
    if has_cs:
        v[:, :ncs] *= O.COLSCALE
    if has_res:
        v = v + ops['residual'].float()
    aux = v.to(a_dtype)
    o = F.gelu(v, approximate='none') if act == 'gelu' else F.relu(v) if act == 'relu' else v
    if accum:
        o = ops['base'] + o
    return aux.double(), o.to(c_dtype).double()


@pytest.mark.parametrize('layout', O.LAYOUTS)
@pytest.mark.parametrize('leg,shape', ALL_SHAPES, ids=[f'{leg}-{s[0]}x{s[1]}x{s[2]}' for leg, s in ALL_SHAPES])
def test_torch_fp32_evaluation_stays_inside_the_bound(leg, shape, layout):
    M, N, K, tile = shape
    a_dtype = DTYPE_OF_LEG(leg)
    ops, prod = _case(layout, M, N, K, a_dtype)
    worst = 0.0
    for c_dtype in {a_dtype, torch.float32}:
        for epi in _epilogues(c_dtype == torch.float32):
            for ncs in _ncols(epi, N, tile):
                pre, out, S = O.case_reference(ops, layout, epi, ncs, prod=prod)
                aux, got = _fp32_eval(layout, ops, epi, ncs, c_dtype, a_dtype)
                act = O.EPILOGUES[epi][3] is not None
                lim = O.bound(S, K, out, act=act, pre=pre, bf16=c_dtype == torch.bfloat16)
                lim_aux = O.bound(S, K, pre, bf16=a_dtype == torch.bfloat16)
                assert ((got - out).abs() <= lim).all(), (epi, ncs, c_dtype, float(((got - out).abs() / lim).max()))
                assert ((aux - pre).abs() <= lim_aux).all(), (epi, ncs, 'aux', float(((aux - pre).abs() / lim_aux).max()))
                worst = max(worst, float(((got - out).abs() / lim).max()))
    print(f'{leg} {shape} {layout}: largest err / bound of the fp32 evaluation {worst:.3f}')


@pytest.mark.parametrize('c_dtype', [torch.float32, torch.bfloat16], ids=['c_f32', 'c_bf16'])
@pytest.mark.parametrize('leg,shape', ALL_SHAPES, ids=[f'{leg}-{s[0]}x{s[1]}x{s[2]}' for leg, s in ALL_SHAPES])
def test_wrong_epilogues_leave_the_bound(leg, shape, c_dtype):
    """Each mistake, evaluated exactly (fp64) and rounded like the kernel's store, is outside the bound on at least 90 % of the elements
    it touches: the bound is tight enough to see an off-by-one at a column-scale boundary or one dropped residual row."""
    M, N, K, tile = shape
    a_dtype = DTYPE_OF_LEG(leg)
    if c_dtype == torch.bfloat16 and a_dtype == torch.float32:
        c_dtype = torch.float32                                  # C is fp32 or the operands' dtype
    ops, prod = _case('NT', M, N, K, a_dtype)
    bf16 = c_dtype == torch.bfloat16
    rnd = lambda t: t.to(c_dtype).double()  # noqa: E731

    def outside(wrong, out, S, sel):
        return float(((rnd(wrong) - out).abs() > O.bound(S, K, out, bf16=bf16))[sel].double().mean())

    # column-scale boundary off by one column, at every boundary inside the matrix
    for epi in ('bias+cs', 'bias+cs+res'):
        for ncs in [v for v in O.ncols_values(N, tile) if v < N]:
            _, out, S = O.case_reference(ops, 'NT', epi, ncs, prod=prod)
            _, wrong, _ = O.case_reference(ops, 'NT', epi, ncs + 1, prod=prod)
            sel = (slice(None), ncs)
            assert outside(wrong, out, S, sel) >= 0.9, (epi, ncs)
            assert outside(out, out, S, sel) == 0.0
    # residual omitted on the last row (a tail tile's clamp gone wrong)
    for epi in ('res', 'bias+res', 'bias+cs+res'):
        _, out, S = O.case_reference(ops, 'NT', epi, 100, prod=prod)
        wrong = out.clone()
        wrong[M - 1] -= ops['residual'].double()[M - 1]
        assert outside(wrong, out, S, (M - 1, slice(None))) >= 0.9, epi
    # bias shifted by one column
    for epi in ('bias', 'bias+res'):
        _, out, S = O.case_reference(ops, 'NT', epi, 0, prod=prod)
        shifted = dict(ops, bias=torch.roll(ops['bias'], 1))
        _, wrong, _ = O.case_reference(shifted, 'NT', epi, 0, prod=prod)
        assert outside(wrong, out, S, (slice(None), slice(None))) >= 0.9, epi
