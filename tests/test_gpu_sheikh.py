"""GPU tests of SheikhBiLSTM: the adjacent-pair score kernels against fp64 on their own operands, and the model against the reference's
fixture g19 and the fp64 oracle (tests/sheikh_oracle.py)."""
import numpy as np
import pytest
import torch

from tests import sheikh_oracle as O
from tests.helpers import load, seeded_param
from tests.test_gpu_recurrent_longt5 import _check
from tests.test_sheikh_cpu import case_params, flat_tags

pytestmark = pytest.mark.gpu

GUARD = 7
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}

# (B, L, H): L = 1 (no pair at all) and 2 (one pair); odd row counts that are no multiple of the 4 rows of a workgroup; H below one 16-byte
# vector per lane (8, 32), exactly one pass of 64 lanes in fp32 (256), a partial second pass (264: bf16 33 vectors, fp32 66; 520: bf16 65
# vectors = one past a full pass, fp32 130 = two passes + 2); the bench shape
KERNEL_CASES = [(1, 1, 8), (1, 2, 8), (3, 23, 32), (2, 257, 256), (5, 64, 264), (2, 31, 520), (64, 256, 256)]


def _pair_reference(F, G, ds, B, L, H):
    """fp64 scores / dF / dG of the kernel's own operands"""
    F64, G64 = F.double().cpu().reshape(B, L, H), G.double().cpu().reshape(B, L, H)
    s = torch.cat(((F64[:, :-1] * G64[:, 1:]).sum(-1), torch.ones(B, 1, dtype=torch.float64)), dim=1)
    d = ds.double().cpu()[:, :-1, None]
    z = torch.zeros(B, 1, H, dtype=torch.float64)
    return s, torch.cat((d * G64[:, 1:], z), dim=1), torch.cat((z, d * F64[:, :-1]), dim=1)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', KERNEL_CASES, ids=[f'B{c[0]}_L{c[1]}_H{c[2]}' for c in KERNEL_CASES])
def test_pair_score_kernels_against_fp64(case, dtype):
    from multimodaltopicsegmentation_amd import ops
    B, L, H = case
    dt, N, dev = DTYPES[dtype], B * L, 'cuda'
    torch.manual_seed(1000 * B + L + H)
    FG = (torch.randn(N + GUARD, 2 * H) * 0.5).to(dt).to(dev)           # F | G: the two halves of one buffer, ld = 2H
    FG0 = FG.clone()
    F, G = FG[:N, :H], FG[:N, H:]
    scores = torch.full((N + GUARD,), 7.0, device=dev)
    ops.pair_score_fwd(F, G, B, L, scores[:N])
    ds = torch.randn(B, L).to(dev)
    dA = torch.full((N + GUARD, 2 * H), 7.0, dtype=dt, device=dev)        # dF = left half of dA, dG = right half of dB
    dB = torch.full((N + GUARD, 2 * H), 7.0, dtype=dt, device=dev)
    dF, dG = dA[:N, :H], dB[:N, H:]
    ops.pair_score_bwd(F, G, ds, B, L, dF, dG)
    dF2, dG2 = torch.full((N, H), 3.0, dtype=dt, device=dev), torch.full((N, H), 3.0, dtype=dt, device=dev)
    ops.pair_score_bwd(F, G, ds, B, L, dF2, dG2)
    # rows no pair reads: the last F row and the first G row of every document (the neighbouring document's rows sit right behind / before)
    FGm = FG.clone()
    FGm[:N].view(B, L, 2 * H)[:, L - 1, :H] = 5.0
    FGm[:N].view(B, L, 2 * H)[:, 0, H:] = -5.0
    scores_m = torch.full((N,), 7.0, device=dev)
    ops.pair_score_fwd(FGm[:N, :H], FGm[:N, H:], B, L, scores_m)
    torch.cuda.synchronize()

    assert torch.equal(FG, FG0)
    # guard rows and the untouched half-columns: still 7.0
    assert (scores[N:] == 7.0).all()
    assert (dA[N:].float() == 7.0).all() and (dA[:N, H:].float() == 7.0).all()
    assert (dB[N:].float() == 7.0).all() and (dB[:N, :H].float() == 7.0).all()
    # a second backward: bitwise the same
    assert torch.equal(dF2, dF) and torch.equal(dG2, dG)
    # a pair never crosses a document
    assert torch.equal(scores_m, scores[:N])

    s_ref, dF_ref, dG_ref = _pair_reference(F, G, ds, B, L, H)
    got = scores[:N].view(B, L)
    assert (got[:, L - 1] == 1.0).all()                                   # the appended step, exactly
    _check(got, s_ref, torch.float32, 'scores')                           # fp32 sums over the kernel's own operands: the fp32 bar in both modes
    gF, gG = dF.reshape(B, L, H), dG.reshape(B, L, H)
    assert (gF[:, L - 1].float() == 0).all() and (gG[:, 0].float() == 0).all()
    _check(gF, dF_ref, dt, 'dF')
    _check(gG, dG_ref, dt, 'dG')


def test_pair_score_refuses_uncovered_operands_before_launch():
    from multimodaltopicsegmentation_amd import ops
    dev = 'cuda'
    sc, ds = torch.zeros(4, device=dev), torch.zeros(1, 4, device=dev)
    FG = torch.zeros(4, 24, dtype=torch.bfloat16, device=dev)             # H = 12 in bf16: rows are no 16-byte vectors
    dFG = torch.zeros(4, 24, dtype=torch.bfloat16, device=dev)
    with pytest.raises(NotImplementedError):
        ops.pair_score_fwd(FG[:, :12], FG[:, 12:], 1, 4, sc)
    with pytest.raises(NotImplementedError):
        ops.pair_score_bwd(FG[:, :12], FG[:, 12:], ds, 1, 4, dFG[:, :12], dFG[:, 12:])
    off = torch.zeros(4 * 32 + 1, dtype=torch.bfloat16, device=dev)[1:].view(4, 32)      # 2-byte offset base
    ok = torch.zeros(4, 32, dtype=torch.bfloat16, device=dev)
    with pytest.raises(NotImplementedError):
        ops.pair_score_fwd(off[:, :16], off[:, 16:], 1, 4, sc)
    with pytest.raises(NotImplementedError):
        ops.pair_score_bwd(ok[:, :16], ok[:, 16:], ds, 1, 4, off[:, :16], off[:, 16:])
    torch.cuda.synchronize()
    assert not sc.any() and not dFG.any()


# ------------------------------------------------------------------------------------------------ model level
def _model_from_params(D, H, NL, p, dtype, dropout_in=0.0):
    from multimodaltopicsegmentation_amd import SheikhBiLSTM
    m = SheikhBiLSTM(2, D, H, NL, dropout_in=dropout_in, compute_dtype=dtype, seed=0)
    m.load_state_dict({n: t.float() for n, t in p.items()})
    return m.cuda().eval()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('c', ['a', 'b', 'c'])
def test_fixture_g19(c, dtype):
    """test_fixture_g18's bars: scores of every row 2e-5 / 5e-2 x max(1, max |ref|), loss 2e-5 / 3e-2 relative, gradients element by element
    1e-4 max(1e-3, max |g|) in fp32 and per-tensor L2 <= 0.1 ||g|| in bf16, decode lists identical in fp32."""
    g = load('g19_sheikh_bilstm')
    D, H, NL, p = case_params(g, c, torch.float32)
    m = _model_from_params(D, H, NL, p, dtype)
    x = torch.from_numpy(g[f'{c}_x']).cuda()
    lengths = torch.from_numpy(g[f'{c}_lengths'])
    tags = torch.from_numpy(g[f'{c}_tags']).cuda()
    ref = torch.from_numpy(g[f'{c}_scores'])
    for th in g[f'{c}_ths'].tolist():
        m.th = th
        scores, tag_lists = m(x, lengths)
        assert scores.shape == ref.shape
        err = (scores.cpu() - ref).abs().max().item()
        print(f'g19 {c} {dtype}: scores max err {err:.3e} (max |ref| {ref.abs().max().item():.3f})')
        assert err < (2e-5 if dtype == 'fp32' else 5e-2) * max(1.0, ref.abs().max().item())
        if dtype == 'fp32':
            assert flat_tags(tag_lists).tolist() == g[f'{c}_tags{th}'].tolist(), th
    m.zero_grad()
    loss = m.loss(x, lengths, tags)
    loss.backward()
    want = float(g[f'{c}_loss'])
    print(f'g19 {c} {dtype}: loss {loss.item():.8f} reference {want:.8f}')
    assert abs(loss.item() - want) < (2e-5 if dtype == 'fp32' else 3e-2) * abs(want)
    grads = {n: m.logical_view({n: t.grad.detach()}, n).cpu().double().numpy() for n, t in m.named_parameters()}
    assert sorted(grads) == sorted(g[f'{c}_live_keys'].tolist())
    for n, got in grads.items():
        w = g[f'{c}_g.{n}']
        assert got.shape == w.shape, n
        if dtype == 'fp32':
            assert np.abs(got - w).max() <= 1e-4 * max(1e-3, np.abs(w).max()), (n, np.abs(got - w).max(), np.abs(w).max())
        else:
            assert np.linalg.norm(got - w) <= 0.1 * np.linalg.norm(w), (n, np.linalg.norm(got - w) / np.linalg.norm(w))


def _mid_case(seed=7):
    B, L, D, H, NL = 8, 96, 128, 256, 2
    rng = np.random.default_rng(seed)
    lengths = [96, 1, 2, 57, 96, 33, 80, 14]
    x = torch.from_numpy(rng.standard_normal((B, L, D)).astype(np.float32)).to(torch.bfloat16).float()      # bf16-exact inputs
    tags = torch.full((B, L), -1.0)
    for b, n in enumerate(lengths):
        x[b, n:] = 0.0
        t = (rng.random(n) < 0.25).astype(np.float32)
        t[-1] = 0
        tags[b, :n] = torch.from_numpy(t)
    p = {n: torch.from_numpy(seeded_param(n, s, seed)) for n, s in O.param_shapes(D, H, NL).items()}
    return dict(B=B, L=L, D=D, H=H, NL=NL, lengths=torch.tensor(lengths), x=x, tags=tags, p=p)


def test_mid_size_bf16_against_oracle():
    """test_gpu_parity_fullsize.py's protocol and bars: bf16-exact master weights and inputs on both sides; loss 2e-3 relative; scores of
    every row (padded ones and the appended 1.0 included) max <= 3e-2 max(1, max |s_ref|), mean <= 3e-3; every gradient tensor max <= 2e-2
    max |g_ref| and L2 <= 1e-2 ||g_ref||, none skipped."""
    from tests.test_gpu_parity_fullsize import BAR_L2, BAR_MAX, _round_to_bf16_
    cs = _mid_case()
    m = _round_to_bf16_(_model_from_params(cs['D'], cs['H'], cs['NL'], cs['p'], 'bf16'))
    loss, out = m.loss_and_grad(cs['x'].cuda(), cs['lengths'], cs['tags'].cuda(), True)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {n: t.detach().cpu().double().requires_grad_(True) for n, t in m.state_dict().items()}
    s_ref = O.scores(cs['x'].double(), cs['lengths'], p)
    l_ref = O.loss(s_ref, cs['lengths'], cs['tags'].double())
    l_ref.backward()
    s_ref, l_ref = s_ref.detach(), l_ref.detach()
    d = (out.detach().cpu().double().view_as(s_ref) - s_ref).abs()
    scale = max(1.0, float(s_ref.abs().max()))
    views = m.grad_views()
    assert set(views) == set(p)
    worst = {}
    for name, gv in views.items():
        a, r = gv.detach().cpu().double(), p[name].grad.double()
        worst[name] = (float((a - r).abs().max()) / float(r.abs().max()), float((a - r).norm()) / float(r.norm()))
    print('sheikh 8x96 bf16: loss', float(loss), 'oracle', float(l_ref), 'scores max / mean |d|', float(d.max()), float(d.mean()), 'scale', scale)
    for name, w in worst.items():
        print(f'  {name}: max-ratio {w[0]:.3e} l2-ratio {w[1]:.3e}')
    assert abs(float(loss) - float(l_ref)) <= 2e-3 * abs(float(l_ref)), (float(loss), float(l_ref))
    assert float(d.max()) <= 3e-2 * scale and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    for name, (rmax, rl2) in worst.items():
        assert rmax <= BAR_MAX and rl2 <= BAR_L2, (name, rmax, rl2)


def _small_batch(seed=3, B=4, L=30, D=64):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.tensor([30, 12, 1, 22])
    x = torch.randn(B, L, D, generator=g)
    tags = torch.full((B, L), -1.0)
    for b, n in enumerate(lengths.tolist()):
        tags[b, :n] = (torch.rand(n, generator=g) < 0.3).float()
        tags[b, n - 1] = 0
    return x, lengths, tags


@pytest.mark.parametrize('H', [32, 12])
def test_loss_and_grad_equals_autograd_front_end_bitwise(H):
    from multimodaltopicsegmentation_amd import SheikhBiLSTM
    x, lengths, tags = _small_batch()
    m = SheikhBiLSTM(2, 64, H, 2, dropout_in=0.0, compute_dtype='fp32', seed=5).cuda()
    loss, _ = m.loss_and_grad(x.cuda(), lengths, tags.cuda(), True)
    native = {n: v.clone() for n, v in m.grad_views().items()}
    assert all(torch.isfinite(v).all() for v in native.values()) and sum(float(v.abs().sum()) for v in native.values()) > 0
    m.grad_flat().zero_()
    m.zero_grad()
    l2 = m.loss(x.cuda(), lengths, tags.cuda())
    assert l2.requires_grad and l2.item() == loss.item()
    l2.backward()
    for n, prm in m.named_parameters():
        assert torch.equal(prm.grad, native[n]), n
    with torch.no_grad():
        assert m.loss(x.cuda(), lengths, tags.cuda()).item() == loss.item()


def test_padded_input_rows_do_not_reach_the_gradients():
    """rows at or past a document's length: whatever they hold, the loss and every gradient (the input-facing weight_ih_l0 included) are
    the same bits -- their gate gradients are exactly 0, so they add 0 x value to the weight gradient"""
    from multimodaltopicsegmentation_amd import SheikhBiLSTM
    x, lengths, tags = _small_batch()
    m = SheikhBiLSTM(2, 64, 32, 2, dropout_in=0.0, compute_dtype='fp32', seed=6).cuda()
    x0, x1 = x.clone(), x.clone()
    for b, n in enumerate(lengths.tolist()):
        x0[b, n:] = 0.0
        x1[b, n:] = 3.0 + torch.arange(x.shape[1] - n).view(-1, 1)
    l0, s0 = m.loss_and_grad(x0.cuda(), lengths, tags.cuda(), True)
    l0, s0 = l0.item(), s0.clone()
    g0 = {n: v.clone() for n, v in m.grad_views().items()}
    l1, s1 = m.loss_and_grad(x1.cuda(), lengths, tags.cuda(), True)
    assert l1.item() == l0 and torch.equal(s1, s0)
    for n, v in m.grad_views().items():
        assert torch.equal(v, g0[n]), n
    assert float(g0['lstm.rnn.weight_ih_l0'].abs().max()) > 0 and float(g0['lstm.rnn.weight_ih_l0_reverse'].abs().max()) > 0


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_all_length_one_batch_is_nan_with_zero_gradients(dtype):
    """as upstream (fixture g19 len1_*): the mean over zero elements is NaN, every gradient is zero, the scores are the appended ones"""
    from multimodaltopicsegmentation_amd import SheikhBiLSTM
    g = load('g19_sheikh_bilstm')
    assert np.isnan(float(g['len1_loss'])) and float(g['len1_gmax']) == 0.0
    x, lengths, tags = _small_batch(D=24)
    m = SheikhBiLSTM(2, 24, 12, 1, dropout_in=0.0, compute_dtype=dtype, seed=8).cuda()
    m.loss_and_grad(x.cuda(), lengths, tags.cuda(), True)                 # leaves non-zero gradients behind
    assert float(m.grad_flat().abs().max()) > 0
    x1 = torch.from_numpy(g['len1_x']).cuda()
    loss, scores = m.loss_and_grad(x1, torch.tensor([1, 1, 1]), torch.zeros(3, 1).cuda(), True)
    assert torch.isnan(loss)
    assert scores.shape == (3, 1, 1) and (scores == 1.0).all()
    for n, v in m.grad_views().items():
        assert not v.any(), n
    m.th = 0.4
    sc, lists = m(x1, torch.tensor([1, 1, 1]))
    assert (sc.cpu().numpy() == g['len1_scores']).all() and flat_tags(lists).tolist() == g['len1_tags0.4'].tolist()


def test_text_segmenter_steps():
    from multimodaltopicsegmentation_amd import SheikhBiLSTM, TextSegmenter
    torch.manual_seed(11)
    ts = TextSegmenter(2, 64, 32, num_layers=2, architecture='SheikhBiLSTM', threshold=0.45, compute_dtype='fp32').cuda()
    assert isinstance(ts.model, SheikhBiLSTM) and ts.model.dropout_in == 0.5
    x, lengths, tags = _small_batch()
    batch = {'src_tokens': x.cuda(), 'src_lengths': lengths, 'tgt_tokens': tags.cuda(), 'src_tokens2': None}
    loss = ts.training_step(batch, 0)                                     # model.loss has no `segments`: the TypeError fallback, as upstream
    assert loss.requires_grad and np.isfinite(loss.item())
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in ts.parameters())
    with pytest.raises(AttributeError):
        ts.predict_step(batch, 0)                                         # .th is assigned by test_step only, as upstream
    res = ts.test_step(batch, 0)
    assert ts.model.th == 0.45 and all(np.isfinite(float(v)) for v in res.values())
    assert [len(t) for t in ts.predict_step(batch, 0)] == lengths.tolist()
    # dropout 0.5 on the input is live in eval mode too: the seed decides
    ts.eval()
    torch.manual_seed(1)
    a, _ = ts.model(batch['src_tokens'], lengths)
    torch.manual_seed(2)
    b, _ = ts.model(batch['src_tokens'], lengths)
    assert not torch.equal(a, b)
    calls = ts.model._drop_calls
    torch.manual_seed(1)
    ts.model._drop_calls = calls - 2
    c, _ = ts.model(batch['src_tokens'], lengths)
    assert torch.equal(a, c)
