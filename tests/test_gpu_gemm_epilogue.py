"""Every mts_gemm kernel's epilogue against the fp64 oracle (tests/gemm_epilogue_oracle.py) at tile tails and strided outputs.

One helper runs a case: C, aux and the residual live as column windows of wider buffers with extra rows below, the surroundings hold a
NaN bit pattern.  It checks that aux == pre and C == out within the DERIVED bound of the oracle (element-wise), that nothing outside
[0:M, 0:N] of C / aux was written, that the inputs are bitwise unchanged, that a second call gives the same bits, and that
mts_gemm_last_plan reports the kernel the case was written for (a case that lands elsewhere fails).

Legs (the smallest shapes at which each path exists):
  f32   fp32 operands on the matrix-core kernel and on the VALU kernel; (136, 130, 72) has N % 4 != 0: the scalar tail of epilogue4
  128   the 128x128 bf16 kernel: LDS-DMA form (K = 64: one K-tile), register-staged form (K % 64 != 0, and "gemm_glds" = 0),
        N % 8 != 0 (epilogue4's full branch instead of epi_math8), N % 4 != 0 (its scalar tail), and windows whose leading dimensions
        are 4 mod 8 on an 8-byte aligned base (what the kernel's vec_ok gate sends to epilogue4)
  256   the 256x256 kernel: store_tile_256 with and without the folded bias, its non-vector fallback at N = 260
  224   the 256x224 family: four-wave persistent (224), four-wave with the residual through the LDS (226), four-wave NN (225), the
        eight-wave kernel's fast and generic stores -- both in ONE launch at (264, 448, 320): full tile + M tail --, fp32 C
  c8/r4 operands the big tiles' 16-byte accesses must not be given: a bf16 C on an 8-byte aligned base goes to the 128x128 kernel, a
        residual whose rows are 8-byte aligned to the 224 kernels that read it in 8-byte pieces
Layout / shape combinations the entry point refuses by contract are not parametrised (see the comments at the tables).
"""
import contextlib
import functools

import pytest
import torch

from tests import gemm_epilogue_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC00DEA)}      # NaN bit patterns
OPTION_DEFAULTS = {'gemm_tile': 0, 'gemm_variant': 0, 'gemm_f32_mfma': 1, 'gemm_glds': 1}
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}


@pytest.fixture(scope='module')
def ops():
    from multimodaltopicsegmentation_amd import ops as o
    return o


@contextlib.contextmanager
def _options(**kw):
    from multimodaltopicsegmentation_amd import _lib as L
    try:
        for k, v in kw.items():
            L.check(L.lib.mts_set_option(k.encode(), v))
        yield
    finally:
        for k in kw:
            L.lib.mts_set_option(k.encode(), OPTION_DEFAULTS[k])


def _last_plan():
    import ctypes
    from multimodaltopicsegmentation_amd import _lib as L
    t = ctypes.c_int(0)
    L.lib.mts_gemm_last_plan(ctypes.byref(t), None)
    return t.value


def _geometry(N, mode):
    """(column offset, leading dimension) of a window, in elements.
    a16: offset and leading dimension multiples of 8 elements -- 16-byte aligned rows for bf16 and fp32 (what the big tiles are given)
    w4 : leading dimension 4 mod 8, offset 4: bf16 rows are 8-byte aligned only (128x128 kernel: vec_ok must send this to epilogue4)
    c8 : offset 4 with a leading dimension that is a multiple of 8: a bf16 window on an 8-byte aligned base
    r4 : C and aux as a16, the residual as w4 (run_case)
    N % 4 != 0: the window starts the buffer and the leading dimension is N + 2 (130 -> 132)"""
    if N % 4:
        return 0, N + 2
    n8 = (N + 7) // 8 * 8
    return {'a16': (8, n8 + 24), 'w4': (4, n8 + 28), 'c8': (4, n8 + 24), 'r4': (8, n8 + 24)}[mode]


def _window(M, N, dtype, mode, fill=None):
    off, ld = _geometry(N, mode)
    it, bits = SENTINEL[dtype]
    buf = torch.full((M + 3, ld), bits, dtype=it, device=DEV)
    view = buf.view(dtype)[:M, off:off + N]
    if fill is not None:
        view.copy_(fill)
    return buf, view, off


def _outside_untouched(buf, M, N, off, dtype):
    bits = SENTINEL[dtype][1]
    b = buf.clone()
    b[:M, off:off + N] = bits
    return bool((b == bits).all())


@functools.lru_cache(maxsize=2)
def _operands(layout, M, N, K, a_name):
    cpu = O.make_operands(layout, M, N, K, DT[a_name])
    dev = {k: v.to(DEV) for k, v in cpu.items()}
    pristine = {k: v.clone() for k, v in dev.items()}
    return cpu, dev, pristine, O.product(layout, cpu['A'], cpu['B'])


@functools.lru_cache(maxsize=32)
def _reference(layout, M, N, K, a_name, epi, ncs):
    cpu, _, _, prod = _operands(layout, M, N, K, a_name)
    return O.case_reference(cpu, layout, epi, ncs, prod=prod)


def _bits(t):
    return t.view(SENTINEL[t.dtype][0])


def run_case(ops, tag, layout, shape, a_name, c_name, epi, ncs, expect_plan, mode):
    """One mts_gemm case, every check of the module docstring; returns the list of failures (empty = passed)."""
    from multimodaltopicsegmentation_amd import _lib as L
    M, N, K = shape
    a_dtype, c_dtype = DT[a_name], DT[c_name]
    has_bias, has_res, has_cs, act, want_aux, accum = O.EPILOGUES[epi]
    cpu, dev, pristine, _ = _operands(layout, M, N, K, a_name)
    pre, out, S = _reference(layout, M, N, K, a_name, epi, ncs)
    rbuf = rview = rbuf0 = None
    if has_res:
        rbuf, rview, _ = _window(M, N, a_dtype, 'w4' if mode == 'r4' else mode, fill=dev['residual'])
        rbuf0 = rbuf.clone()
    runs = []
    for _ in range(2):
        cbuf, cview, coff = _window(M, N, c_dtype, 'a16' if (c_dtype == torch.float32 and mode == 'c8') else mode, fill=dev['base'] if accum else None)
        abuf = aview = None
        aoff = 0
        if want_aux:
            abuf, aview, aoff = _window(M, N, a_dtype, mode)
        ops.gemm(getattr(L, layout), dev['A'], dev['B'], cview, M=M, N=N, K=K, bias=dev['bias'] if has_bias else None, residual=rview, aux=aview,
                 gelu=act == 'gelu', relu=act == 'relu', colscale=O.COLSCALE if has_cs else None, ncols_scaled=ncs if has_cs else 0,
                 accumulate=bool(accum))
        runs.append((cbuf, cview, coff, abuf, aview, aoff, _last_plan()))
    torch.cuda.synchronize()
    cbuf, cview, coff, abuf, aview, aoff, plan = runs[0]
    fails = []
    got = cview.cpu().double()
    lim = O.bound(S, K, out, act=act is not None, pre=pre, bf16=c_dtype == torch.bfloat16)
    ratio = float(torch.nan_to_num((got - out).abs() / lim, nan=float('inf')).max())
    ratio_aux = 0.0
    if want_aux:
        got_aux = aview.cpu().double()
        lim_aux = O.bound(S, K, pre, bf16=a_dtype == torch.bfloat16)
        ratio_aux = float(torch.nan_to_num((got_aux - pre).abs() / lim_aux, nan=float('inf')).max())
    print(f'GEMM-EPI {tag} {layout} {M}x{N}x{K} c={c_name} mode={mode} epi={epi} ncs={ncs} plan={plan} err/bound C {ratio:.4f} aux {ratio_aux:.4f}')
    where = f'{epi} ncols_scaled={ncs}'
    if plan != expect_plan:
        fails.append(f'{where}: mts_gemm_last_plan reports {plan}, the case was written for {expect_plan}')
    ok = (got - out).abs() <= lim                                  # (a NaN -- an element never written -- compares false)
    if not ok.all():
        bad = (~ok).nonzero()
        fails.append(f'{where}: C outside the bound at {int((~ok).sum())}/{ok.numel()} elements, first (m, n) = {tuple(bad[0].tolist())}, '
                     f'largest err / bound {ratio:.3g}')
    if want_aux:
        ok = (got_aux - pre).abs() <= lim_aux
        if not ok.all():
            bad = (~ok).nonzero()
            fails.append(f'{where}: aux outside the bound at {int((~ok).sum())}/{ok.numel()} elements, first (m, n) = {tuple(bad[0].tolist())}, '
                         f'largest err / bound {ratio_aux:.3g}')
        if not _outside_untouched(abuf, M, N, aoff, a_dtype):
            fails.append(f'{where}: aux buffer written outside [0:M, 0:N]')
        if not torch.equal(abuf, runs[1][3]):
            fails.append(f'{where}: aux differs between two identical calls')
    if not _outside_untouched(cbuf, M, N, coff, c_dtype):
        fails.append(f'{where}: C buffer written outside [0:M, 0:N]')
    if not torch.equal(cbuf, runs[1][0]):
        fails.append(f'{where}: C differs between two identical calls')
    if runs[1][6] != plan:
        fails.append(f'{where}: the second call ran kernel {runs[1][6]}, the first {plan}')
    for k in ('A', 'B', 'bias'):
        if not torch.equal(_bits(dev[k]), _bits(pristine[k])):
            fails.append(f'{where}: input {k} was modified')
    if has_res and not torch.equal(rbuf, rbuf0):
        fails.append(f'{where}: the residual buffer was modified')
    return fails


def _expect_224(layout, c_name, variant, M, K, epi, ncs, mode='a16'):
    """What mts_launch_gemm224 picks (csrc/gemm224.hip): 224 = the eight-wave kernel or the four-wave persistent one (gemm224p.hip),
    225 = gemm224n.hip, 226 = gemm224r.hip.  The four-wave kernels take bias / column scale / residual only, M % 256 == 0 and a column-scale
    boundary that is a multiple of 4; the NT ones K % 128 == 0 and K >= 256, the NN one K >= 128.  225 and 226 copy the residual tile to the LDS
    in 16-byte pieces: a residual whose rows are only 8-byte aligned (mode r4) goes to the kernels that read it in 8-byte pieces."""
    _, has_res, has_cs, act, _, accum = O.EPILOGUES[epi]
    if mode == 'r4' and has_res:
        return 224
    four = c_name == 'bf16' and act is None and not accum and M % 256 == 0 and (not has_cs or ncs % 4 == 0)
    if layout == 'NT' and four and K % 128 == 0 and K >= 256:
        if variant == 9 or (variant == 0 and has_res):
            return 226
    if layout == 'NN' and four and variant == 0 and K >= 128:
        return 225
    return 224


# (tag, leg, layout, (M, N, K), tile of the kernel, operand dtype, C dtype, window mode, options)
CONFIGS = []
for mfma in (1, 0):
    for shp in O.SHAPES['f32']:
        for lay in O.LAYOUTS:
            CONFIGS.append((f'f32-mfma{mfma}', 'f32', lay, shp[:3], 128 if mfma else 64, 'f32', 'f32', 'a16', {'gemm_f32_mfma': mfma}))
for c in ('bf16', 'f32'):
    for glds, shp in ((1, (136, 136, 64)), (1, (136, 136, 200)), (0, (136, 136, 64))):
        for lay in O.LAYOUTS:
            CONFIGS.append((f'128-glds{glds}', '128', lay, shp, 128, 'bf16', c, 'a16', {'gemm_tile': 128, 'gemm_glds': glds}))
        if glds:
            CONFIGS.append(('128-glds1', '128', 'NT', shp, 128, 'bf16', c, 'w4', {'gemm_tile': 128, 'gemm_glds': 1}))
    # N = 132, 130 -- NT only: "mts_gemm(bf16,NN): K,N % 8" and "mts_gemm(bf16,TN): M,N % 8" refuse N % 8 != 0
    CONFIGS.append(('128-glds1', '128', 'NT', (136, 132, 64), 128, 'bf16', c, 'a16', {'gemm_tile': 128, 'gemm_glds': 1}))
    CONFIGS.append(('128-glds1', '128', 'NT', (136, 130, 64), 128, 'bf16', c, 'a16', {'gemm_tile': 128, 'gemm_glds': 1}))
    for lay in O.LAYOUTS:
        CONFIGS.append(('256', '256', lay, (264, 264, 256), 256, 'bf16', c, 'a16', {'gemm_tile': 256}))
    # N = 260 -- NT only: "mts_gemm(bf16,NN): K,N % 8" and "mts_gemm(bf16,TN): M,N % 8"
    CONFIGS.append(('256', '256', 'NT', (264, 260, 256), 256, 'bf16', c, 'a16', {'gemm_tile': 256}))
for lay, variant in (('NT', 0), ('NT', 12), ('NT', 9), ('NT', 6), ('NT', 1), ('NN', 0), ('NN', 6), ('TT', 0)):
    CONFIGS.append((f'224-v{variant}', '224', lay, (512, 448, 256), 224, 'bf16', 'bf16', 'a16', {'gemm_tile': 224, 'gemm_variant': variant}))
for lay in ('NT', 'NN'):
    CONFIGS.append(('224-v0', '224', lay, (264, 448, 320), 224, 'bf16', 'bf16', 'a16', {'gemm_tile': 224, 'gemm_variant': 0}))
    for shp in ((512, 448, 256), (264, 448, 320)):
        CONFIGS.append(('224-v0', '224', lay, shp, 224, 'bf16', 'f32', 'a16', {'gemm_tile': 224, 'gemm_variant': 0}))
# bf16 C on an 8-byte aligned base with the big tiles forced: their stores move 16 bytes whenever N % 8 == 0 and ldc % 8 == 0, so the
# entry point gives such a C to the 128x128 kernel (expected plan 128)
CONFIGS.append(('256-c8', 'c8', 'NT', (264, 264, 256), 256, 'bf16', 'bf16', 'c8', {'gemm_tile': 256}))
CONFIGS.append(('224-c8', 'c8', 'NT', (512, 448, 256), 224, 'bf16', 'bf16', 'c8', {'gemm_tile': 224, 'gemm_variant': 0}))

# a residual with ldr = 4 mod 8 on an 8-byte aligned base: the two kernels that move it in 16-byte pieces must decline (plan 224, not 226 / 225)
for lay in ('NT', 'NN'):
    CONFIGS.append(('224-r4', '224', lay, (512, 448, 256), 224, 'bf16', 'bf16', 'r4', {'gemm_tile': 224, 'gemm_variant': 0}))

CASES = [(cfg, epi) for cfg in CONFIGS for epi, spec in O.EPILOGUES.items() if cfg[6] == 'f32' or not spec[5]]


def _case_id(case):
    (tag, _, lay, shp, _, _, c, mode, _), epi = case
    return f'{tag}-{lay}-{shp[0]}x{shp[1]}x{shp[2]}-c_{c}-{mode}-{epi}'


@pytest.mark.parametrize('case', CASES, ids=[_case_id(c) for c in CASES])
def test_gemm_epilogue_against_fp64(ops, case):
    (tag, leg, layout, shape, tile, a_name, c_name, mode, options), epi = case
    M, N, K = shape
    fails = []
    with _options(**options):
        for ncs in (O.ncols_values(N, tile) if O.EPILOGUES[epi][2] else [0]):
            if leg == '224':
                expect = _expect_224(layout, c_name, options['gemm_variant'], M, K, epi, ncs, mode)
            else:
                expect = {'f32': 128, '128': 128, '256': 256, 'c8': 128}[leg]
            fails += run_case(ops, tag, layout, shape, a_name, c_name, epi, ncs, expect, mode)
    assert not fails, '\n'.join(fails)


def test_fp32_operands_refuse_misaligned_aux_and_residual(ops):
    """epilogue4 moves fp32 aux and residual as float4: a leading dimension that is no multiple of 4, or a base off 16 bytes, is MTS_ERR_INVALID
    before any launch (C stays untouched)."""
    from multimodaltopicsegmentation_amd import _lib as L
    M, N, K = 8, 8, 8
    a, b, bias = torch.zeros(M, K, device=DEV), torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
    wide = torch.zeros(M + 1, 16, device=DEV)
    for kw in (dict(aux=wide.view(-1)[:M * 10].view(M, 10)[:, :N], gelu=True),            # ldaux = 10
               dict(aux=wide[:M, 2:2 + N], gelu=True),                                       # base 8 bytes past a 16-byte boundary
               dict(residual=wide[:M, 2:2 + N])):
        c = torch.full((M, N), 7.0, device=DEV)
        with pytest.raises(ValueError):
            ops.gemm(L.NT, a, b, c, M=M, N=N, K=K, bias=bias, **kw)
        assert bool((c == 7.0).all())


def test_every_kernel_of_the_224_family_is_reached():
    """The expected plans of the parametrisation above name all three values, with and without a residual, and the activation epilogues on the
    four-wave shapes expect the generic path: a change of the table that loses a kernel fails here, on the table itself."""
    seen = set()
    for (tag, leg, layout, shape, tile, a_name, c_name, mode, options), epi in CASES:
        if leg != '224':
            continue
        for ncs in (O.ncols_values(shape[1], tile) if O.EPILOGUES[epi][2] else [0]):
            if mode == 'a16':
                seen.add((layout, options['gemm_variant'], epi, ncs, _expect_224(layout, c_name, options['gemm_variant'], shape[0], shape[2], epi, ncs)))
    assert ('NT', 0, 'bias', 0, 224) in seen and ('NT', 0, 'bias+res', 0, 226) in seen and ('NT', 12, 'bias+res', 0, 224) in seen
    assert ('NT', 9, 'bias+cs', 224, 226) in seen and ('NN', 0, 'bias+cs+res', 260, 225) in seen
    assert ('NT', 0, 'bias+cs+res', 101, 224) in seen and ('NN', 0, 'bias+cs', 101, 224) in seen      # the four-wave kernels decline 101
    assert ('NT', 0, 'bias+res+gelu+aux', 0, 224) in seen and ('NT', 9, 'bias+relu+aux', 0, 224) in seen
