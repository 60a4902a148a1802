"""GPU tests of RecurrentLongT5: the LongT5 local-attention and RMSNorm kernels against fp64 on their own operands, and the model
against the reference's fixture g18 and the fp64 oracle (tests/longt5_oracle.py)."""
import numpy as np
import pytest
import torch

from tests import longt5_oracle as O
from tests.full_attention_oracle import keep_mask
from tests.helpers import load

pytestmark = pytest.mark.gpu

GUARD = 7


def _l2(got, want):
    return ((got - want).norm() / want.norm().clamp(min=1e-30)).item()


def _check(got, want, dtype, what):
    got, want = got.double().cpu(), want.double().cpu()
    tol, l2 = (2e-4, 2e-5) if dtype == torch.float32 else (4e-2, 1e-2)
    scale = max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert err <= tol * scale, (what, err, scale)
    if want.norm() > 0:
        assert _l2(got, want) <= l2, (what, _l2(got, want))


def _attn_case(dtype, B, L, heads, radius, lengths, drop_p=0.0, seed=11):
    from multimodaltopicsegmentation_amd import ops
    from multimodaltopicsegmentation_amd.t5_taggers import num_buckets, relative_position_buckets
    torch.manual_seed(seed)
    inner, N = heads * 64, B * L
    dev = 'cuda'
    qkv = (torch.randn(N + GUARD, 3 * inner) * 0.5).to(dtype).to(dev)
    nb = num_buckets(radius)
    table = (torch.randn(nb, heads) * 0.5).to(dev)
    bkt = relative_position_buckets(radius).to(torch.int32).to(dev)
    li = torch.tensor(lengths, dtype=torch.int32, device=dev)
    ctx = torch.full((N + GUARD, inner), 7.0, dtype=dtype, device=dev)
    lse = torch.zeros(N, heads, device=dev)
    dseed = 1234 + seed
    ops.t5_local_attn_fwd(qkv[:N], li, B, L, heads, radius, table, bkt, ctx[:N], lse, drop_p, dseed)
    dctx = (torch.randn(N + GUARD, inner) * 0.5).to(dtype).to(dev)
    dqkv = torch.full((N + GUARD, 3 * inner), 7.0, dtype=dtype, device=dev)
    dtable = torch.full((nb, heads), 7.0, device=dev)
    ops.t5_local_attn_bwd(qkv[:N], li, B, L, heads, radius, table, bkt, lse, ctx[:N], dctx[:N], dqkv[:N], dtable, drop_p, dseed)
    dqkv2, dtable2 = torch.empty_like(dqkv[:N]), torch.empty_like(dtable)
    ops.t5_local_attn_bwd(qkv[:N], li, B, L, heads, radius, table, bkt, lse, ctx[:N], dctx[:N], dqkv2, dtable2, drop_p, dseed)
    torch.cuda.synchronize()
    # guard rows past each output: untouched
    assert (ctx[N:].float() == 7.0).all() and (dqkv[N:].float() == 7.0).all()
    # a second backward: bitwise the same
    assert torch.equal(dqkv2, dqkv[:N]) and torch.equal(dtable2, dtable)

    # fp64 on the kernel's own operands
    q64 = qkv[:N].double().cpu().view(B, L, 3, heads, 64)
    q, k, v = (q64[:, :, s].clone().requires_grad_(True) for s in range(3))
    t64 = table.double().cpu().requires_grad_(True)
    lens = torch.tensor(lengths)
    keep = None
    if drop_p:
        km = keep_mask(N * heads * (2 * radius + 1), drop_p, dseed).reshape(B, L, heads, 2 * radius + 1)
        keep = torch.from_numpy(km.astype(np.float64)) / (1.0 - np.float32(drop_p))
    want, lse_w = O.local_attention(q, k, v, lens, radius, t64, bkt.long().cpu(), keep=keep, return_lse=True)
    valid = (torch.arange(L).view(1, L) < lens.view(B, 1))
    _check(ctx[:N].view(B, L, heads, 64), want.detach(), dtype, 'ctx')
    assert (lse.cpu().view(B, L, heads)[valid] - lse_w.detach()[valid]).abs().max().item() < (1e-4 if dtype == torch.float32 else 3e-2)
    do = dctx[:N].double().cpu().view(B, L, heads, 64) * valid.view(B, L, 1, 1)     # padded rows' dctx is not read
    (want * do).sum().backward()
    got = dqkv[:N].double().cpu().view(B, L, 3, heads, 64)
    for s, t, name in ((0, q, 'dq'), (1, k, 'dk'), (2, v, 'dv')):
        _check(got[:, :, s], t.grad, dtype, name)
    # padded rows carry no gradient: dq of padded queries, dk / dv of padded keys are exactly 0
    pad = ~valid
    assert (got[pad] == 0).all()
    _check(dtable, t64.grad, dtype, 'dtable')
    reach = torch.zeros(nb, dtype=torch.bool)
    reach[bkt.long().cpu()] = True
    assert (dtable.cpu()[~reach] == 0).all()


ATTN_CASES = [
    # B, L, heads, radius, lengths, drop_p
    (3, 23, 4, 8, [23, 1, 17], 0.0),
    (2, 19, 2, 3, [19, 7], 0.0),
    (3, 40, 2, 15, [40, 29, 3], 0.0),
    (2, 70, 2, 1, [70, 33], 0.0),
    (2, 256, 8, 120, [256, 131], 0.0),
    (1, 2437, 2, 200, [2437], 0.0),
    (2, 300, 2, 200, [300, 1], 0.0),
    (1, 1, 2, 3, [1], 0.0),
    (3, 96, 4, 15, [96, 50, 1], 0.1),
    (2, 256, 8, 120, [256, 200], 0.1),
]


MODES = ('fp32', 'mfma', 'generic')     # mfma: bf16 on the matrix-core kernels (the default); generic: bf16 with t5_mfma 0


class _t5_mfma:
    """mts_set_option("t5_mfma", on) for this thread while the block runs (the option is per host thread)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from multimodaltopicsegmentation_amd import _lib as Lb
        assert Lb.lib.mts_set_option(b't5_mfma', int(self.on)) == 0

    def __exit__(self, *a):
        from multimodaltopicsegmentation_amd import _lib as Lb
        Lb.lib.mts_set_option(b't5_mfma', 1)
        return False


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ATTN_CASES, ids=[f'B{c[0]}_L{c[1]}_h{c[2]}_r{c[3]}_p{c[5]}' for c in ATTN_CASES])
def test_local_attention_kernels_against_fp64(case, mode):
    B, L, heads, radius, lengths, p = case
    with _t5_mfma(mode != 'generic'):
        _attn_case(torch.float32 if mode == 'fp32' else torch.bfloat16, B, L, heads, radius, lengths, p)


def test_matrix_core_and_generic_bf16_agree():
    """the two bf16 paths compute the same thing: ctx / dqkv / dtable within bf16 rounding of each other, at the bench shape"""
    from multimodaltopicsegmentation_amd import ops
    from multimodaltopicsegmentation_amd.t5_taggers import num_buckets, relative_position_buckets
    torch.manual_seed(3)
    B, L, heads, r = 4, 256, 8, 120
    N, inner = B * L, heads * 64
    qkv = (torch.randn(N, 3 * inner) * 0.5).to(torch.bfloat16).cuda()
    dctx = (torch.randn(N, inner) * 0.5).to(torch.bfloat16).cuda()
    table = (torch.randn(num_buckets(r), heads) * 0.5).cuda()
    bkt = relative_position_buckets(r).to(torch.int32).cuda()
    li = torch.tensor([256, 200, 77, 1], dtype=torch.int32).cuda()
    out = {}
    for on in (1, 0):
        with _t5_mfma(on):
            ctx, lse = torch.empty(N, inner, dtype=torch.bfloat16).cuda(), torch.empty(N, heads).cuda()
            dqkv, dt = torch.empty_like(qkv), torch.empty_like(table)
            ops.t5_local_attn_fwd(qkv, li, B, L, heads, r, table, bkt, ctx, lse)
            ops.t5_local_attn_bwd(qkv, li, B, L, heads, r, table, bkt, lse, ctx, dctx, dqkv, dt)
            torch.cuda.synchronize()
            out[on] = (ctx.double().cpu(), dqkv.double().cpu(), dt.double().cpu())
    for a, b_, name in zip(out[1], out[0], ('ctx', 'dqkv', 'dtable')):
        assert _l2(a, b_) < 1e-2, (name, _l2(a, b_))


def test_local_attention_refuses_misaligned_operands_before_launch():
    from multimodaltopicsegmentation_amd import ops
    from multimodaltopicsegmentation_amd.t5_taggers import relative_position_buckets
    N, inner = 16, 128
    qkv = torch.zeros(N * 3 * inner + 1, dtype=torch.bfloat16, device='cuda')[1:].view(N, 3 * inner)      # 2-byte offset
    table = torch.zeros(4, 2, device='cuda')
    bkt = relative_position_buckets(3).to(torch.int32).cuda()
    ctx, lse = torch.zeros(N, inner, dtype=torch.bfloat16, device='cuda'), torch.zeros(N, 2, device='cuda')
    with pytest.raises(NotImplementedError):
        ops.t5_local_attn_fwd(qkv, None, 1, N, 2, 3, table, bkt, ctx, lse)
    x = torch.zeros(4 * 64 + 1, device='cuda')[1:].view(4, 64)
    with pytest.raises(NotImplementedError):
        ops.rmsnorm_fwd(x, torch.ones(64, device='cuda'), 1e-6, torch.zeros(4, 64, device='cuda'), torch.zeros(4, 1, device='cuda'))
    # RMSNorm: D above 8 x 256 columns, D no multiple of 4 (NotImplementedError); dx aliasing x (ValueError).  Nothing is written.
    for dtype in (torch.float32, torch.bfloat16):
        for D in (2052, 6):
            x, dy = torch.ones(3, D, dtype=dtype, device='cuda'), torch.ones(3, D, dtype=dtype, device='cuda')
            w, rstd = torch.ones(D, device='cuda'), torch.full((3, 1), 7.0, device='cuda')
            y, dx, dw = torch.full_like(x, 7.0), torch.full_like(x, 7.0), torch.full((D,), 7.0, device='cuda')
            with pytest.raises(NotImplementedError):
                ops.rmsnorm_fwd(x, w, 1e-6, y, rstd)
            with pytest.raises(NotImplementedError):
                ops.rmsnorm_bwd(x, dy, w, rstd, dx, dw)
            torch.cuda.synchronize()
            assert (y == 7.0).all() and (rstd == 7.0).all() and (dx == 7.0).all() and (dw == 7.0).all()
        x, dy = torch.ones(3, 64, dtype=dtype, device='cuda'), torch.ones(3, 64, dtype=dtype, device='cuda')
        w, rstd, dw = torch.ones(64, device='cuda'), torch.ones(3, 1, device='cuda'), torch.full((64,), 7.0, device='cuda')
        with pytest.raises(ValueError):
            ops.rmsnorm_bwd(x, dy, w, rstd, x, dw)
        torch.cuda.synchronize()
        assert (x == 1.0).all() and (dw == 7.0).all()


def test_local_attention_refuses_other_head_dims_before_launch():
    from multimodaltopicsegmentation_amd import _lib as Lb
    rc = Lb.lib.mts_t5_local_attn_fwd(None, 0, 1, 8, 2, 32, 3, None, None, None, 4, None, None, None, 0.0, 0)
    assert rc == 2


# (rows, D).  Lane l of a row's wave holds columns 4 l + 256 k, k < NV = 1 / 2 / 4 / 8 (tests/test_instantiation_cover_cpu.py keeps
# the list of what has to be reached)
RMS_CASES = [(1, 64), (37, 128), (16384, 512), (300, 1792),
             (2, 4),                 # the smallest D: one live lane
             (5, 260),               # NV = 2, the second slot holds 4 columns; D % 16 = 4 in the dw reduce
             (70, 772),              # NV = 4, last slot partial; 18 backward workgroups: the reduce's 16 parts are unevenly filled
             (9, 1024),              # NV = 4 full
             (1030, 768),            # NV = 4; 258 row groups on 256 workgroups: the backward strides; rows % 4 = 2
             (3, 2044),              # NV = 8, last slot partial
             (6, 2048),              # NV = 8 full, the largest D
             (3, 256)]               # NV = 1 full


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('rows,D', RMS_CASES)
def test_rmsnorm_kernels_against_fp64(rows, D, dtype):
    from multimodaltopicsegmentation_amd import ops
    torch.manual_seed(rows + D)
    x = torch.randn(rows, D).to(dtype).cuda()
    w = (1 + 0.1 * torch.rand(D)).cuda()
    y = torch.empty_like(x)
    rstd = torch.empty(rows, 1, device='cuda')
    ops.rmsnorm_fwd(x, w, 1e-6, y, rstd)
    dy = torch.randn(rows, D).to(dtype).cuda()
    dres = torch.randn(rows, D).to(dtype).cuda()
    dx = dres.clone()
    dw = torch.full((D,), 7.0, device='cuda')
    ops.rmsnorm_bwd(x, dy, w, rstd, dx, dw, dres=dx)
    dx2, dw2 = torch.empty_like(dx), torch.empty_like(dw)
    ops.rmsnorm_bwd(x, dy, w, rstd, dx2, dw2)
    torch.cuda.synchronize()
    x64 = x.double().cpu().requires_grad_(True)
    w64 = w.double().cpu().requires_grad_(True)
    want = O.rms(x64, w64)
    _check(y, want.detach(), dtype, 'y')
    (want * dy.double().cpu()).sum().backward()
    _check(dx2, x64.grad, dtype, 'dx')
    _check(dx, x64.grad + dres.double().cpu(), dtype, 'dx + dres')
    _check(dw2, w64.grad, dtype, 'dw')
    assert torch.equal(dw, dw2)


# ------------------------------------------------------------------------------------------------ model level
def _model_from_params(D, H, heads, r, NL, loss_fn, p, dtype):
    from multimodaltopicsegmentation_amd import RecurrentLongT5
    m = RecurrentLongT5(2, D, H, num_layers=NL, nheads=heads, loss_fn=loss_fn, window_size=r, compute_dtype=dtype, seed=0)
    m.load_state_dict({n: t.float() for n, t in p.items()})
    return m.cuda().eval()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('c', ['a', 'b', 'c'])
def test_fixture_g18(c, dtype):
    g = load('g18_recurrent_longt5')
    D, H, heads, r, NL = (int(v) for v in g[f'{c}_cfg'])
    loss_fn = {'a': 'FocalLoss', 'b': 'BinaryCrossEntropy', 'c': 'FocalLoss'}[c]
    seed = int(g[f'{c}_seed'])
    shapes = O.param_shapes(D, H, heads, r, NL)
    p = {n: torch.from_numpy(O.seeded_longt5_param(n, s, seed)) for n, s in shapes.items()}
    m = _model_from_params(D, H, heads, r, NL, loss_fn, p, dtype)
    x = torch.from_numpy(g[f'{c}_x']).cuda()
    lengths = torch.from_numpy(g[f'{c}_lengths'])
    tags = torch.from_numpy(g[f'{c}_tags']).cuda()
    tol = 2e-5 if dtype == 'fp32' else 3e-2
    m.th = 0.5
    scores, tag_lists = m(x, lengths)
    ref = torch.from_numpy(g[f'{c}_scores'])
    assert scores.shape == ref.shape
    # fp32: 2e-5 on every row; bf16 (weights and activations in bf16 against the fixture's fp32 run): 5e-2 on every row
    assert (scores.cpu() - ref).abs().max().item() < (2e-5 if dtype == 'fp32' else 5e-2) * max(1.0, ref.abs().max().item())
    if dtype == 'fp32':
        assert np.concatenate([np.array(t, dtype=np.int64) for t in tag_lists]).tolist() == g[f'{c}_tags0.5'].tolist()
    m.zero_grad()
    loss = m.loss(x, lengths, tags)
    loss.backward()
    want = float(g[f'{c}_loss'])
    assert abs(loss.item() - want) < tol * max(1.0, abs(want))
    grads = {n: t.grad.detach().cpu().double() for n, t in m.named_parameters()}
    # fp32: element by element.  bf16 (weights rounded to bf16 against the fixture's fp32 ones, two blocks of bf16 recurrences and
    # attention): per tensor, the L2 ratio / the norms -- the element-wise bf16 bars are the full-size test's, against the oracle
    for n in shapes:
        got = grads[n].numpy()
        if f'{c}_g.{n}' in g:
            w = g[f'{c}_g.{n}']
            if dtype == 'fp32':
                assert np.abs(got - w).max() <= 1e-4 * max(1e-3, np.abs(w).max()), n
            else:
                assert np.linalg.norm(got - w) <= 0.1 * np.linalg.norm(w), (n, np.linalg.norm(got - w) / np.linalg.norm(w))
        else:
            w = g[f'{c}_gsum.{n}']
            cs = np.array([got.sum(), np.abs(got).sum(), (got * got).sum()])
            rt = 1e-3 if dtype == 'fp32' else 0.1
            assert abs(cs[1] - w[1]) <= rt * w[1] and abs(np.sqrt(cs[2]) - np.sqrt(w[2])) <= rt * np.sqrt(w[2]), (n, cs, w)


def _full_size(equal, seed=5):
    B, L, D, H, heads, r, NL = 64, 256, 512, 256, 8, 120, 2
    rng = np.random.default_rng(seed)
    lengths = [L] * B if equal else [int(v) for v in rng.integers(1, L + 1, size=B)]
    lengths[0] = L
    if not equal:
        lengths[1] = 1
    x = torch.from_numpy(rng.standard_normal((B, L, D)).astype(np.float32)).to(torch.bfloat16).float()   # bf16-exact inputs
    tags = torch.full((B, L), -1.0)
    for b, n in enumerate(lengths):
        x[b, n:] = 0.0
        t = (rng.random(n) < 0.25).astype(np.float32)
        t[-1] = 0
        tags[b, :n] = torch.from_numpy(t)
    shapes = O.param_shapes(D, H, heads, r, NL)
    p = {n: torch.from_numpy(O.seeded_longt5_param(n, s, seed)) for n, s in shapes.items()}
    return dict(B=B, L=L, D=D, H=H, heads=heads, r=r, NL=NL, lengths=torch.tensor(lengths), x=x, tags=tags, p=p)


def _oracle(cs, need_grad, p=None):
    p = {n: t.detach().double().requires_grad_(need_grad) for n, t in (p or cs['p']).items()}
    scores = O.recurrent_longt5_scores(cs['x'].double(), cs['lengths'], p, cs['heads'], cs['r'], cs['NL'])
    loss = O.tagger_loss(scores, cs['lengths'], cs['tags'].double(), 'FocalLoss')
    if need_grad:
        loss.backward()
    return scores.detach(), loss.detach(), p


# Bars of the full-size bf16 test.  The protocol is test_gpu_parity_fullsize.py's (bf16-exact master weights and inputs, every row,
# every gradient tensor, none skipped) and so are the loss and the scores-max bars.  Two bars are wider, by what the model's depth
# costs in bf16: two recurrences and two LongT5 layers whose residual stream and its gradient are stored in bf16 (measured on one
# MI355X, matrix-core and generic attention alike, so not an attention-kernel effect):
#   scores mean |d|: 3.2e-3 (equal batch) against the parity files' 3e-3 -> 4e-3;
#   per gradient tensor: worst max ratio 5.0e-2 and L2 ratio 5.0e-2, both on relative_attention_bias.weight (a sum of ~10^6 dS terms
#   per (offset, head) that largely cancel); every other tensor <= 3.4e-2 (block 0's W_ih and q / k) -> 6e-2 for both.
FULL_BAR_MAX, FULL_BAR_L2, FULL_BAR_MEAN = 6e-2, 6e-2, 4e-3


@pytest.mark.parametrize('equal', [True, False], ids=['equal', 'ragged'])
def test_full_size_bf16_against_oracle(equal):
    """bf16-exact master weights and inputs on both sides; loss within 2e-3 relative; scores of every row (padded ones included) max
    <= 3e-2, mean <= FULL_BAR_MEAN; every gradient tensor max <= FULL_BAR_MAX * max |g_ref| and L2 <= FULL_BAR_L2 * ||g_ref||."""
    from tests.test_gpu_parity_fullsize import _round_to_bf16_
    cs = _full_size(equal)
    m = _round_to_bf16_(_model_from_params(cs['D'], cs['H'], cs['heads'], cs['r'], cs['NL'], 'FocalLoss', cs['p'], 'bf16'))
    x, tags = cs['x'].cuda(), cs['tags'].cuda()
    loss, out = m.loss_and_grad(x, cs['lengths'], tags, True)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    s_ref, l_ref, p = _oracle(cs, True, {k: v.cpu() for k, v in m.state_dict().items()})
    assert abs(float(loss) - float(l_ref)) <= 2e-3 * abs(float(l_ref)), (float(loss), float(l_ref))
    d = (out.detach().cpu().double().view_as(s_ref) - s_ref).abs()
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= FULL_BAR_MEAN, (float(d.max()), float(d.mean()))
    views = m.grad_views()
    assert set(views) == set(p)
    worst = {}
    for name, gv in views.items():
        a, r = gv.detach().cpu().double(), p[name].grad.double()
        rmax, rl2 = float(r.abs().max()), float(r.norm())
        assert rmax > 0, name
        dmax, dl2 = float((a - r).abs().max()), float((a - r).norm())
        worst[name] = (dmax / rmax, dl2 / rl2)
        assert dmax <= FULL_BAR_MAX * rmax and dl2 <= FULL_BAR_L2 * rl2, (name, dmax / rmax, dl2 / rl2)
    print('recurrent longt5 64x256 bf16 worst (max-ratio, l2-ratio):', max(v[0] for v in worst.values()), max(v[1] for v in worst.values()))


def test_full_size_fp32_boundaries_match_oracle():
    cs = _full_size(False, seed=9)
    s_ref, _, _ = _oracle(cs, False)
    m = _model_from_params(cs['D'], cs['H'], cs['heads'], cs['r'], cs['NL'], 'FocalLoss', cs['p'], 'fp32')
    scores, tags = m(cs['x'].cuda(), cs['lengths'])
    assert (scores.cpu().double() - s_ref).abs().max().item() < 1e-3
    from oracle.restatement import greedy_decode
    want = greedy_decode(s_ref, cs['lengths'], None, True)
    assert tags == want


def test_training_mode_dropout_statistics():
    """dropout_in = 0.1 in training mode: the T5 layer's dropouts and the attention dropout are live; the loss moves with the seed,
    its mean stays near the eval loss, and eval mode is deterministic."""
    from multimodaltopicsegmentation_amd import RecurrentLongT5
    torch.manual_seed(0)
    B, L, D, H = 8, 64, 128, 64
    x = torch.randn(B, L, D).cuda()
    lengths = torch.tensor([64, 50, 33, 64, 1, 20, 64, 40])
    tags = (torch.rand(B, L) < 0.25).float().cuda()
    m = RecurrentLongT5(2, D, H, num_layers=2, nheads=2, loss_fn='FocalLoss', window_size=15, dropout_in=0.1, compute_dtype='fp32',
                        seed=1).cuda()
    m.dropout_in = 0.0                                   # eval reference without the RNN's always-on input dropout
    m.eval()
    ref = m.loss_and_grad(x, lengths, tags, False)[0].item()
    assert m.loss_and_grad(x, lengths, tags, False)[0].item() == ref
    m.dropout_in = 0.1
    m.train()
    vals = [m.loss_and_grad(x, lengths, tags, True)[0].item() for _ in range(12)]
    assert len(set(vals)) == len(vals)
    assert abs(np.mean(vals) - ref) < 0.25 * abs(ref) + 5 * np.std(vals) / np.sqrt(len(vals))
    assert all(np.isfinite(m.grad_flat().cpu().numpy()))


def test_training_mode_dropout_gradients_by_finite_differences():
    """Training mode with every dropout live (the RNN's input / output dropouts of each block, the T5 layer's five dropouts and the
    attention dropout): with the dropout calls replayed (same seeds), the derivative of the loss along each parameter tensor's own
    gradient, by central differences in fp32, equals ||g||^2 -- a missing or mismatched mask in the backward breaks it."""
    from multimodaltopicsegmentation_amd import RecurrentLongT5
    torch.manual_seed(0)
    B, L, D, H = 3, 40, 64, 32
    x = torch.randn(B, L, D).cuda()
    lengths = torch.tensor([40, 23, 9])
    tags = torch.full((B, L), -1.0)
    for b, n in enumerate(lengths.tolist()):
        tags[b, :n] = (torch.rand(n) < 0.3).float()
        tags[b, n - 1] = 0
    tags = tags.cuda()
    m = RecurrentLongT5(2, D, H, num_layers=2, nheads=2, loss_fn='FocalLoss', window_size=8, dropout_in=0.2, dropout_out=0.2,
                        compute_dtype='fp32', seed=7).cuda()
    m.train()
    c0 = m._drop_calls

    def run(want_grad):
        m._drop_calls = c0                       # replay the same dropout seeds
        return float(m.loss_and_grad(x, lengths, tags, want_grad)[0])

    l0 = run(True)
    g = {n: v.clone() for n, v in m.grad_views().items()}
    assert run(True) == l0 and all(torch.equal(g[n], v) for n, v in m.grad_views().items())
    m.eval()
    m.dropout_in = m.dropout_out = 0.0
    assert abs(run(False) - l0) > 1e-6 * abs(l0)   # the masks are live
    m.dropout_in = m.dropout_out = 0.2
    m.train()
    params = dict(m.named_parameters())
    checked = 0
    for n, u in g.items():
        uu = float((u.double() ** 2).sum())
        if uu < 1e-12:
            continue
        eps = 1e-3 * abs(l0) / uu
        with torch.no_grad():
            params[n].add_(u, alpha=eps)
            lp = run(False)
            params[n].add_(u, alpha=-2 * eps)
            lm = run(False)
            params[n].add_(u, alpha=eps)
        fd = (lp - lm) / (2 * eps)
        assert abs(fd - uu) <= 2e-2 * uu, (n, fd, uu)
        checked += 1
    assert checked >= 30, checked


def test_native_trainer_adam_step_matches_oracle_gradients():
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    g = load('g18_recurrent_longt5')
    c = 'a'
    D, H, heads, r, NL = (int(v) for v in g[f'{c}_cfg'])
    shapes = O.param_shapes(D, H, heads, r, NL)
    p = {n: torch.from_numpy(O.seeded_longt5_param(n, s, int(g[f'{c}_seed']))) for n, s in shapes.items()}
    m = _model_from_params(D, H, heads, r, NL, 'FocalLoss', p, 'fp32')
    lengths = torch.from_numpy(g[f'{c}_lengths'])
    tags = torch.from_numpy(g[f'{c}_tags'])
    x = torch.from_numpy(g[f'{c}_x'])
    p64 = {n: t.double().requires_grad_(True) for n, t in p.items()}
    sc = O.recurrent_longt5_scores(x.double(), lengths, p64, heads, r, NL)
    O.tagger_loss(sc, lengths, tags.double(), 'FocalLoss').backward()
    lr = 1e-3
    tr = NativeTrainer(m, lr=lr, optimizer='Adam')
    tr.step({'src_tokens': x.cuda(), 'src_lengths': lengths, 'tgt_tokens': tags.cuda()})
    torch.cuda.synchronize()
    sd = m.state_dict()
    for n, t in p64.items():
        gr = t.grad
        step = lr * gr / (gr.abs() + 1e-7)               # Adam's first step: lr * g / (|g| + eps) (bias-corrected moments)
        want = p[n].double() - step
        got = sd[n].cpu().double()
        big = gr.abs() > 1e-4                            # where the sign of g is unambiguous
        assert (got[big] - want[big]).abs().max().item() < 1e-6 + 2e-5 * lr, n
        assert (got - p[n].double()).abs().max().item() <= lr * 1.0001, n
