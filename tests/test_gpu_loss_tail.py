"""The loss kernels (csrc/loss.hip: mts_tagger_loss, mts_greedy_decode) and the last layer's one-pass tail (csrc/norm.hip: mts_layernorm_loss_tail)
against the fp64 reference of tests/loss_tail_oracle.py, in every launch regime the kernels have:

  A  the tail in fp32 against fp64: 2 workgroups with idle waves, 512 workgroups with one row per wave, a second and a third row for some waves (the
     software-pipelined fetch of the next row), 250 workgroups (the final kernel's unrolled loop plus its tail loop), NV = 1, 2, 4, 7, 8, padded and
     packed batches, Lt > L, all three losses, grad_scale 1 and 0.5
  B  the same shapes in bf16: bit for bit against the four launches the tail replaces, and stage by stage against fp64 on the bf16-rounded input
  C  mts_tagger_loss: one workgroup (512 rows), two, an odd row count (the U = 2 row tail), 2100 rows, 525 200 rows (the 1024-workgroup cap and its
     grid-stride loop), packed forms, n_out 1..4, lengths = NULL, dscores = NULL, saturated scores in a later workgroup's share, all-ignored batches,
     workspace = NULL and a 4-float workspace
  D  mts_greedy_decode values for n_out 1..4

Bars.  Every tensor is held to tol * max|ref| of ITS OWN reference -- no max(1, .): the gradients of a mean loss over a few thousand rows are about
4e-5 at most, and a floor of 1 would pass an error of 50 %.  tol = 2e-5 is the project's fp32 figure (tests/test_gpu_norm_fused.py); the same formula
in fp32 torch on the CPU (tail_reference(dtype=torch.float32)) deviates from fp64 by at most 1.1e-6 of max|ref| on any output of any case of this
file (dhead_b and dbeta of the focal cases; 4.6e-7 at most on scores and dx), so the bar sits about 20 x above rounding noise.  Loss: 2e-6 * max(1, |ref|) and dscores rtol 2e-4 as tests/test_gpu_kernels.py::test_tagger_loss_and_decode, its
atol 1e-8 (set at about 100 averaged rows) scaled with the 1 / count every gradient carries: 1e-6 / count.  bf16: the bars of
test_head_parameter_gradients_from_the_layernorm_backward (scores 3e-2 absolute, dx 1e-2, parameter gradients 2e-5), relative to max|ref|.
Every check prints `[ratio] section tensor err bar ratio` before it asserts (pytest -s shows them)."""
import functools

import pytest
import torch

from tests import loss_tail_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 1e-12
ALPHA, GAMMA_F = 0.9, 2.0
KINDS = [O.FOCAL, O.BCE, O.CE]
KIND_IDS = {O.FOCAL: 'focal', O.BCE: 'bce', O.CE: 'ce'}


@pytest.fixture(scope='module')
def ops():
    from multimodaltopicsegmentation_amd import ops as o
    return o


def _rel(section, name, got, ref, tol):
    """max|got - ref| <= tol * max|ref|, max|ref| > 0 (NaN in got fails: the comparison is false)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    m = ref.abs().max().item()
    assert m > 0, name
    d = (got - ref).abs().max().item()
    print(f'[ratio] {section} {name} err {d:.3e} bar {tol * m:.3e} ratio {d / (tol * m):.4f}')
    assert d <= tol * m, (name, d, m)


def _loss_close(section, got, ref, name='loss'):
    bar = 2e-6 * max(1.0, abs(ref))
    d = abs(got - ref)
    print(f'[ratio] {section} {name} err {d:.3e} bar {bar:.3e} ratio {d / bar:.4f}')
    assert d <= bar, (name, got, ref)


# ------------------------------------------------------------------------------------------------ A / B: the one-pass tail
TAIL_CASES = {
    # 2 workgroups, 3 idle waves
    'r5_d256': dict(D=256, B=1, L=5, Lt=5, lengths=[5], packed=False, gs=1.0),
    # 512 workgroups, one row per wave
    'r2048_d256': dict(D=256, B=8, L=256, Lt=256, lengths=[256] * 8, packed=False, gs=1.0),
    # 13 waves take a second row (the pipelined fetch); packed, Lt > L
    'r2061_d256_packed': dict(D=256, B=9, L=300, Lt=303, lengths=[300, 1, 287, 300, 150, 300, 263, 300, 160], packed=True, gs=0.5),
    # NV = 7, padded and ragged, Lt > L
    'r2100_d1792': dict(D=1792, B=7, L=300, Lt=303, lengths=[300, 1, 120, 300, 77, 250, 299], packed=False, gs=1.0),
    # a third row for 4 waves, NV = 8; packed
    'r4100_d2048_packed': dict(D=2048, B=16, L=300, Lt=300, lengths=[300] * 5 + [1] + [300] * 5 + [299, 250, 200, 175, 175], packed=True, gs=1.0),
    # 250 workgroups: the final kernel's eight-deep loop once, then its tail loop; NV = 2 and 4
    'r1000_d512': dict(D=512, B=4, L=250, Lt=250, lengths=[250, 1, 180, 250], packed=False, gs=0.5),
    'r1000_d1024': dict(D=1024, B=4, L=250, Lt=250, lengths=[250, 1, 180, 250], packed=False, gs=1.0),
}
assert sum(TAIL_CASES['r2061_d256_packed']['lengths']) == 2061 and sum(TAIL_CASES['r4100_d2048_packed']['lengths']) == 4100


def _targets(g, B, L, Lt, lengths, n_classes, ignore_some, pad=-1.0):
    """[B, Lt] fp32: class 1 at rate 0.3 (classes 2.. share another 0.3 when n_classes > 2) inside a document, `pad` after it, 7 in the columns at or
    past L (never to be read); ignore_some: the middle sentence of the first three documents is -1 as well"""
    tg = torch.full((B, Lt), pad)
    for b, n in enumerate(lengths):
        u = torch.rand(n, generator=g)
        y = (u < 0.3).float()
        for c in range(2, n_classes):
            y[(u >= 0.3 + 0.3 * (c - 2) / (n_classes - 2)) & (u < 0.3 + 0.3 * (c - 1) / (n_classes - 2))] = float(c)
        tg[b, :n] = y
    tg[:, L:] = 7.0
    if ignore_some:
        for b in range(min(3, B)):
            tg[b, lengths[b] // 2] = -1.0
    return tg


@functools.lru_cache(maxsize=None)
def _tail_inputs(case, kind):
    """CPU fp32 inputs of one tail case, built once and never modified"""
    c = TAIL_CASES[case]
    D, B, L = c['D'], c['B'], c['L']
    n_out = 2 if kind == O.CE else 1
    g = torch.Generator().manual_seed(1000 * kind + D + sum(c['lengths']))
    row_src = O.pack_rows(c['lengths'], L) if c['packed'] else None
    rows = row_src.numel() if c['packed'] else B * L
    x = torch.randn(rows, D, generator=g) * 1.7 + 0.3
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    hw, hb = torch.randn(n_out, D, generator=g) / D ** 0.5, torch.randn(n_out, generator=g)
    tg = _targets(g, B, L, c['Lt'], c['lengths'], 2, ignore_some=(kind == O.CE))
    return dict(x=x, gamma=gamma, beta=beta, hw=hw, hb=hb, tg=tg, lengths=torch.tensor(c['lengths']), row_src=row_src, rows=rows, n_out=n_out,
                shape=(B, L), gs=c['gs'], D=D)


def _dev(inp, dtype):
    d = {k: inp[k].to(DEV) for k in ('gamma', 'beta', 'hw', 'hb', 'tg')}
    d['x'] = inp['x'].to(dtype).to(DEV)
    d['li32'] = inp['lengths'].to(torch.int32).to(DEV)
    d['rs'] = inp['row_src'].to(DEV) if inp['row_src'] is not None else None
    return d


def _nan_outputs(inp, dtype):
    rows, D, n_out = inp['rows'], inp['D'], inp['n_out']
    nan = lambda *s, dt=torch.float32: torch.full(s, float('nan'), dtype=dt, device=DEV)
    return dict(scores=nan(rows, n_out), loss=nan(2), dx=nan(rows, D, dt=dtype), dgamma=nan(D), dbeta=nan(D), dxsum=nan(D), dhead_w=nan(n_out, D),
                dhead_b=nan(n_out))


def _run_tail(ops, kind, inp, dtype):
    d, o = _dev(inp, dtype), _nan_outputs(inp, dtype)
    ops.layernorm_loss_tail(kind, d['x'], d['gamma'], d['beta'], EPS, d['hw'], d['hb'], d['tg'], d['li32'], ALPHA, GAMMA_F, inp['gs'], o['scores'],
                            o['loss'], o['dx'], o['dgamma'], o['dbeta'], o['dxsum'], o['dhead_w'], o['dhead_b'], inp['shape'], row_src=d['rs'])
    torch.cuda.synchronize()
    return o


def _run_four_launches(ops, kind, inp, dtype):
    """what the tail replaces: mts_layernorm_fwd (y not stored, fused head), mts_tagger_loss, mts_scale, mts_layernorm_bwd (fused head, dhead_w)"""
    d, o = _dev(inp, dtype), _nan_outputs(inp, dtype)
    rows, n_out, (B, L) = inp['rows'], inp['n_out'], inp['shape']
    mean, rstd = torch.full((rows, 1), float('nan'), device=DEV), torch.full((rows, 1), float('nan'), device=DEV)
    ops.layernorm_fwd(d['x'], d['gamma'], d['beta'], EPS, None, mean, rstd, head_w=d['hw'], head_b=d['hb'], scores=o['scores'])
    ds = torch.full((rows, n_out), float('nan'), device=DEV)
    if d['rs'] is None:
        ops.tagger_loss(kind, o['scores'].view(B, L, n_out), d['tg'], d['li32'], ALPHA, GAMMA_F, o['loss'], ds.view(B, L, n_out))
    else:
        ops.tagger_loss(kind, o['scores'], d['tg'], d['li32'], ALPHA, GAMMA_F, o['loss'], ds, row_src=d['rs'], batch_shape=(B, L))
    ops.scale_(ds, inp['gs'])
    ops.layernorm_bwd(d['x'], None, d['gamma'], mean, rstd, o['dx'], o['dgamma'], o['dbeta'], dxsum=o['dxsum'], dlogit=ds, head_w=d['hw'], beta=d['beta'],
                      dhead_w=o['dhead_w'], dhead_b=o['dhead_b'])
    torch.cuda.synchronize()
    return o


def _tail_params():
    return [pytest.param(case, kind, id=f'{case}-{KIND_IDS[kind]}') for case in TAIL_CASES for kind in KINDS]


@pytest.mark.parametrize('case,kind', _tail_params())
def test_tail_fp32_against_fp64(ops, case, kind):
    """A.  fp32 inputs; scores, dx, dgamma, dbeta, dhead_w, dhead_b to 2e-5 * max|ref| of each tensor, the loss to 2e-6 * max(1, |ref|), the count
    exactly, dxsum against the column sums of the dx the kernel stored."""
    inp = _tail_inputs(case, kind)
    ref = O.tail_reference(inp['x'], inp['gamma'], inp['beta'], EPS, inp['hw'], inp['hb'], inp['tg'], inp['lengths'], kind, ALPHA, GAMMA_F, inp['gs'],
                           inp['shape'], inp['row_src'])
    got = _run_tail(ops, kind, inp, torch.float32)
    lengths_sum = int(inp['lengths'].sum())
    assert ref['count'] == (lengths_sum - min(3, inp['shape'][0]) if kind == O.CE else lengths_sum)
    assert float(got['loss'][1]) == float(ref['count'])
    _loss_close('A', float(got['loss'][0]), ref['loss'])
    for name in ('scores', 'dx', 'dgamma', 'dbeta', 'dhead_w', 'dhead_b'):
        _rel('A', name, got[name], ref[name].view(got[name].shape), 2e-5)
    _rel('A', 'dxsum', got['dxsum'], got['dx'].double().sum(0), 2e-5)


@pytest.mark.parametrize('case,kind', _tail_params())
def test_tail_bf16_bitwise_against_the_four_launches(ops, case, kind):
    """B.i  the header's contract: scores and every gradient bitwise those of the four launches, the loss up to the grouping of its partial sums."""
    inp = _tail_inputs(case, kind)
    one = _run_tail(ops, kind, inp, torch.bfloat16)
    four = _run_four_launches(ops, kind, inp, torch.bfloat16)
    for name in ('scores', 'dx', 'dgamma', 'dbeta', 'dxsum', 'dhead_w', 'dhead_b'):
        assert not torch.isnan(four[name].float()).any(), name
        assert torch.equal(one[name], four[name]), name
        assert torch.count_nonzero(one[name]) > 0, name
    assert float(one['loss'][1]) == float(four['loss'][1]) > 0
    _loss_close('B.i', float(one['loss'][0]), float(four['loss'][0]))


@pytest.mark.parametrize('case,kind', _tail_params())
def test_tail_bf16_against_fp64_stage_by_stage(ops, case, kind):
    """B.ii  fp64 on the bf16-ROUNDED x.  Forward: scores to 3e-2 absolute (the head reads y rounded to bf16), loss and count from the oracle at the
    kernel's stored scores.  Backward: d loss / d scores from the oracle at the kernel's stored scores, then dx to 1e-2 * max|ref| (one bf16 rounding)
    and dgamma / dbeta / dhead_w / dhead_b to 2e-5 * max|ref| (fp32 throughout).  dxsum is the fp32 column sum of the ROUNDED dx: compared with
    the stored dx at 2e-5 as in A; against fp64 it would need a bar of its own, so that is left to B.i."""
    inp = _tail_inputs(case, kind)
    got = _run_tail(ops, kind, inp, torch.bfloat16)
    xr = inp['x'].to(torch.bfloat16).double()
    B, L = inp['shape']
    sc = got['scores'].cpu().double()
    shaped = sc if inp['row_src'] is not None else sc.view(B, L, -1)
    lref = O.loss_reference(shaped, inp['tg'], inp['lengths'], kind, ALPHA, GAMMA_F, inp['shape'], inp['row_src'])
    ref = O.tail_backward_reference(xr, inp['gamma'], inp['beta'], EPS, inp['hw'], inp['hb'], lref['dscores'].view(sc.shape) * inp['gs'])
    d = (sc - ref['scores']).abs().max().item()
    print(f'[ratio] B.ii scores err {d:.3e} bar 3.000e-02 ratio {d / 3e-2:.4f}')
    assert d <= 3e-2
    assert float(got['loss'][1]) == float(lref['count'])
    _loss_close('B.ii', float(got['loss'][0]), lref['loss'])
    _rel('B.ii', 'dx', got['dx'].float(), ref['dx'], 1e-2)
    for name in ('dgamma', 'dbeta', 'dhead_w', 'dhead_b'):
        _rel('B.ii', name, got[name], ref[name].view(got[name].shape), 2e-5)
    _rel('B.ii', 'dxsum', got['dxsum'], got['dx'].double().sum(0), 2e-5)


# ------------------------------------------------------------------------------------------------ C: mts_tagger_loss
def _ragged(g, B, L):
    n = torch.randint(1, L + 1, (B,), generator=g).tolist()
    n[0], n[1], n[-1] = L, 1, L
    return n


_L525 = [4040] * 130
_L525[1], _L525[5], _L525[77] = 1, 2021, 4039
LOSS_CASES = {
    'n512': dict(B=4, L=128, Lt=128, packed=False),                    # the last single-workgroup size
    'n513': dict(B=3, L=171, Lt=171, packed=False),                    # two workgroups, the second holds one row
    'n1023': dict(B=3, L=341, Lt=341, packed=False),                   # odd: the second row of the last pair is out of range
    'n2100': dict(B=7, L=300, Lt=303, packed=False),                   # 5 workgroups, Lt > L
    'n2100_packed': dict(B=7, L=300, Lt=303, packed=True),
    'n525200': dict(B=130, L=4040, Lt=4040, packed=False),             # 1026 shares on 1024 workgroups: the grid-stride loop
    'n525200_packed': dict(B=130, L=4040, Lt=4040, packed=True, lengths=_L525),     # 519 141 rows, 1014 workgroups
}
LOSS_VARIANTS = [(O.FOCAL, 1), (O.BCE, 1), (O.CE, 2), (O.CE, 3), (O.CE, 4)]
VARIANT_IDS = [f'{KIND_IDS[k]}{n}' for k, n in LOSS_VARIANTS]


@functools.lru_cache(maxsize=None)
def _loss_inputs(case, kind, n_out, no_lengths=False):
    """CPU inputs of one mts_tagger_loss case.  Scores 2 * randn: BCELoss on sigmoid(x) loses 1 - p to fp32 rounding as x grows (at x = 10 the
    log is already off by 1e-3), which is the reference model's own arithmetic and not what is under test; the three saturated rows (0, +40, -40, as
    test_tagger_loss_and_decode) are the LAST three rows -- the last workgroup's share, a second grid-stride pass at 525 200 rows."""
    c = LOSS_CASES[case]
    B, L, Lt = c['B'], c['L'], c['Lt']
    g = torch.Generator().manual_seed(7 * B + L + 100 * kind + n_out)
    lengths = [L] * B if no_lengths else (c.get('lengths') or _ragged(g, B, L))
    row_src = O.pack_rows(lengths, L) if c['packed'] else None
    N = row_src.numel() if c['packed'] else B * L
    sc = 2.0 * torch.randn(N, n_out, generator=g)
    tg = _targets(g, B, L, Lt, lengths, max(n_out, 2), ignore_some=(kind == O.CE))
    sc[N - 3:] = 0.0
    sc[N - 2, 0], sc[N - 1, 0] = 40.0, -40.0
    tg[B - 1, L - 3:L] = torch.tensor([1.0, 1.0, 0.0] if kind == O.CE else [1.0, 0.0, 1.0])
    return dict(sc=sc, tg=tg, lengths=None if no_lengths else torch.tensor(lengths), row_src=row_src, N=N, shape=(B, L), n_out=n_out)


def _run_loss(ops, kind, inp, alpha=ALPHA, gamma_f=GAMMA_F, want_grad=True):
    B, L = inp['shape']
    sc = inp['sc'].to(DEV)
    out = torch.full((2,), float('nan'), device=DEV)
    ds = torch.full_like(sc, float('nan')) if want_grad else None
    li32 = inp['lengths'].to(torch.int32).to(DEV) if inp['lengths'] is not None else None
    if inp['row_src'] is None:
        ops.tagger_loss(kind, sc.view(B, L, -1), inp['tg'].to(DEV), li32, alpha, gamma_f, out, ds.view(B, L, -1) if want_grad else None)
    else:
        ops.tagger_loss(kind, sc, inp['tg'].to(DEV), li32, alpha, gamma_f, out, ds, row_src=inp['row_src'].to(DEV), batch_shape=(B, L))
    torch.cuda.synchronize()
    return out.cpu(), (ds.cpu() if want_grad else None)


def _check_loss(section, kind, inp, out, ds, alpha=ALPHA, gamma_f=GAMMA_F):
    B, L = inp['shape']
    sc = inp['sc'] if inp['row_src'] is not None else inp['sc'].view(B, L, -1)
    ref = O.loss_reference(sc, inp['tg'], inp['lengths'], kind, alpha, gamma_f, inp['shape'], inp['row_src'])
    assert ref['count'] > 0 and float(out[1]) == float(ref['count'])
    _loss_close(section, float(out[0]), ref['loss'])
    if ds is None:
        return ref
    rg = ref['dscores'].view(ds.shape)
    err = (ds.double() - rg).abs()
    lim = 2e-4 * rg.abs() + 1e-6 / ref['count']
    print(f'[ratio] {section} dscores err {err.max().item():.3e} ratio {(err / lim).max().item():.4f}')
    assert not torch.isnan(ds).any()
    assert bool((err <= lim).all()), (int((err > lim).sum()), err.max().item())
    assert float(rg.abs().max()) > 0
    use, _, _ = O.averaged_rows(inp['tg'].double(), inp['lengths'], kind, inp['shape'], inp['row_src'])
    assert torch.all(ds[~use] == 0)                 # rows outside a document, or with target -1: exactly 0
    if inp['row_src'] is None and inp['lengths'] is not None:
        assert int((~use).sum()) > 0
    return ref


@pytest.mark.parametrize('kind,n_out', LOSS_VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize('case', list(LOSS_CASES))
def test_tagger_loss_against_fp64(ops, case, kind, n_out):
    """C.  loss, count and dscores in every launch regime; dscores = NULL gives the same loss"""
    inp = _loss_inputs(case, kind, n_out)
    out, ds = _run_loss(ops, kind, inp)
    _check_loss('C', kind, inp, out, ds)
    out2, _ = _run_loss(ops, kind, inp, want_grad=False)
    assert torch.equal(out, out2)


@pytest.mark.parametrize('kind', [O.FOCAL, O.BCE], ids=lambda k: KIND_IDS[k])
@pytest.mark.parametrize('case', ['n1023', 'n2100'])
def test_tagger_loss_without_lengths(ops, case, kind):
    """lengths = NULL: every one of the B * L rows is averaged"""
    inp = _loss_inputs(case, kind, 1, no_lengths=True)
    out, ds = _run_loss(ops, kind, inp)
    ref = _check_loss('C', kind, inp, out, ds)
    assert ref['count'] == inp['N']


@pytest.mark.parametrize('alpha,gamma_f', [(-1.0, 2.0), (0.9, 0.0), (0.5, 3.0)])
def test_focal_loss_parameters(ops, alpha, gamma_f):
    """alpha < 0 (no class weight), gamma = 0 (the modulating factor is 1) and gamma = 3 (the powf branch) over five workgroups"""
    inp = _loss_inputs('n2100', O.FOCAL, 1)
    out, ds = _run_loss(ops, O.FOCAL, inp, alpha, gamma_f)
    _check_loss('C', O.FOCAL, inp, out, ds, alpha, gamma_f)


@pytest.mark.parametrize('kind,n_out', LOSS_VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize('case', ['n512', 'n2100', 'n2100_packed'])
def test_all_ignored_batch_gives_zero(ops, case, kind, n_out):
    """CE with every target -1, BCE / focal with every length 0: {0, 0}, all-zero dscores, no NaN (cnt > 0 ? ... : 0 in both kernels)"""
    inp = dict(_loss_inputs(case, kind, n_out))
    inp['tg'] = torch.full_like(inp['tg'], -1.0)
    if kind != O.CE:
        inp['lengths'] = torch.zeros_like(inp['lengths'])
    out, ds = _run_loss(ops, kind, inp)
    assert out.tolist() == [0.0, 0.0]
    assert torch.all(ds == 0)
    B, L = inp['shape']
    ref = O.loss_reference(inp['sc'] if inp['row_src'] is not None else inp['sc'].view(B, L, -1), inp['tg'], inp['lengths'], kind, ALPHA, GAMMA_F,
                           inp['shape'], inp['row_src'])
    assert ref['loss'] == 0.0 and ref['count'] == 0


@pytest.mark.parametrize('kind,n_out', LOSS_VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize('ws_floats', [0, 4])
def test_tagger_loss_with_no_and_with_a_small_workspace(ops, ws_floats, kind, n_out):
    """Through the C ABI at 2100 rows: workspace = NULL (one workgroup walks all five shares) and a 4-float workspace (four workgroups, the first takes
    a second share): the header promises the same result up to fp32 summation order"""
    from multimodaltopicsegmentation_amd import _lib as Lb
    inp = _loss_inputs('n2100', kind, n_out)
    B, L = inp['shape']
    sc, tg, li32 = inp['sc'].to(DEV), inp['tg'].to(DEV), inp['lengths'].to(torch.int32).to(DEV)
    out = torch.full((2,), float('nan'), device=DEV)
    ds = torch.full_like(sc, float('nan'))
    ws = torch.full((ws_floats,), float('nan'), device=DEV) if ws_floats else None
    Lb.check(Lb.lib.mts_tagger_loss(Lb.stream_ptr(), kind, B, L, tg.shape[1], n_out, Lb.ptr(sc), Lb.ptr(tg), Lb.ptr(li32), ALPHA, GAMMA_F, Lb.ptr(out),
                                    Lb.ptr(ds), Lb.ptr(ws), 4 * ws_floats, None, 0))
    torch.cuda.synchronize()
    _check_loss('C', kind, inp, out.cpu(), ds.cpu())


# ------------------------------------------------------------------------------------------------ D: mts_greedy_decode
@pytest.mark.parametrize('n_out', [1, 2, 3, 4])
def test_greedy_decode_values(ops, n_out):
    """D.  tags against the fp64 decode for four thresholds; a row whose fp64 probability lies within 1e-6 of the threshold may go either way in
    fp32 and is left out -- at most 0.5 % of the rows (none at all for these seeds at n_out 3 and 4)"""
    B, L = 7, 300
    lengths = torch.tensor([300, 1, 120, 300, 77, 250, 299])
    g = torch.Generator().manual_seed(50 + n_out)
    sc = 2.0 * torch.randn(B, L, n_out, generator=g)
    scd, li32 = sc.to(DEV), lengths.to(torch.int32).to(DEV)
    for th in (0.4, 0.5, 0.05, 0.95):
        want, prob = O.decode_reference(sc, lengths, th)
        tags = torch.full((B, L), 7, dtype=torch.uint8, device=DEV)
        ops.greedy_decode(scd, li32, th, tags)
        torch.cuda.synchronize()
        tags = tags.cpu()
        unsure = (prob - th).abs() <= 1e-6
        assert int(unsure.sum()) <= 0.005 * B * L
        assert 0 < int(want.sum()) < int(lengths.sum())
        assert torch.equal(tags[~unsure], want[~unsure]), (n_out, th, int((tags != want).sum()))
        assert torch.all((tags == 0) | (tags == 1))
        for b, n in enumerate(lengths.tolist()):
            assert int(tags[b, n:].sum()) == 0                                   # positions past the length are 0
    want_none, prob = O.decode_reference(sc, None, 0.4)                          # lengths = NULL: every position is decoded
    tags = torch.full((B, L), 7, dtype=torch.uint8, device=DEV)
    ops.greedy_decode(scd, None, 0.4, tags)
    sure = (prob - 0.4).abs() > 1e-6
    assert torch.equal(tags.cpu()[sure], want_none[sure])
