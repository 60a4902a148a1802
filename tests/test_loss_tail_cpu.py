"""CPU pins of tests/loss_tail_oracle.py, the fp64 reference the GPU tests of the loss kernels and the one-pass tail compare against
(tests/test_gpu_loss_tail.py): against oracle.restatement and torch's own operators on padded and packed batches, against the reference's fixture
g6_focal for every (alpha, gamma) in it, and the packed description of a batch against the padded one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests import loss_tail_oracle as O
from tests.helpers import load

LENGTHS = [23, 17, 1, 9, 23, 0]
B, L, LT = len(LENGTHS), 23, 26


def _batch(n_out, seed=0, ignore_some=False):
    """-> scores [B, L, n_out] fp64, targets [B, LT] (pad -1; columns past L hold 7: never to be read), lengths"""
    g = torch.Generator().manual_seed(seed)
    sc = torch.randn(B, L, n_out, generator=g, dtype=torch.float64) * 3
    tg = torch.full((B, LT), -1.0, dtype=torch.float64)
    for b, n in enumerate(LENGTHS):
        tg[b, :n] = torch.randint(0, max(n_out, 2), (n,), generator=g).double()
    tg[:, L:] = 7.0
    if ignore_some:
        tg[0, 3] = tg[4, 22] = tg[1, 0] = -1.0
    return sc, tg, torch.tensor(LENGTHS)


def _autograd(fn, sc):
    s = sc.clone().requires_grad_(True)
    loss = fn(s)
    (g,) = torch.autograd.grad(loss, s)
    return loss.item(), g


@pytest.mark.parametrize('kind', [O.FOCAL, O.BCE, O.CE])
@pytest.mark.parametrize('packed', [False, True])
def test_oracle_against_the_restatement(kind, packed):
    n_out = 2 if kind == O.CE else 1
    sc, tg, lengths = _batch(n_out, seed=kind)
    want_loss, want_grad = _autograd(lambda s: R.tagger_loss(s, lengths, tg, O.KIND_NAMES[kind], 0.9, 2.0), sc)
    if packed:
        rs = O.pack_rows(LENGTHS, L)
        got = O.loss_reference(sc.view(B * L, n_out)[rs.long()], tg, lengths, kind, 0.9, 2.0, (B, L), rs)
        want_grad = want_grad.view(B * L, n_out)[rs.long()]
    else:
        got = O.loss_reference(sc, tg, lengths, kind, 0.9, 2.0)
    assert got['count'] == sum(LENGTHS)
    assert abs(got['loss'] - want_loss) <= 1e-13 * max(1.0, abs(want_loss))
    assert torch.allclose(got['dscores'], want_grad, rtol=1e-11, atol=1e-16)
    assert float(got['dscores'].abs().max()) > 0


@pytest.mark.parametrize('n_out', [2, 3, 4])
@pytest.mark.parametrize('packed', [False, True])
def test_cross_entropy_against_torch(n_out, packed):
    """nn.CrossEntropyLoss(ignore_index=-1) over every row, with in-length targets ignored too: count < sum(lengths)"""
    sc, tg, lengths = _batch(n_out, seed=10 + n_out, ignore_some=True)
    flat_t = tg[:, :L].reshape(-1).long()
    want_loss, want_grad = _autograd(lambda s: F.cross_entropy(s.view(-1, n_out), flat_t, ignore_index=-1), sc)
    if packed:
        rs = O.pack_rows(LENGTHS, L)
        got = O.loss_reference(sc.view(B * L, n_out)[rs.long()], tg, lengths, O.CE, batch_shape=(B, L), row_src=rs)
        want_grad = want_grad.view(B * L, n_out)[rs.long()]
    else:
        got = O.loss_reference(sc, tg, None, O.CE)
    assert got['count'] == sum(LENGTHS) - 3 == int((flat_t != -1).sum())
    assert abs(got['loss'] - want_loss) <= 1e-13 * max(1.0, abs(want_loss))
    assert torch.allclose(got['dscores'], want_grad, rtol=1e-11, atol=1e-16)
    if not packed:                                   # rows with target -1 (pad or ignored): gradient exactly 0
        assert torch.all(got['dscores'].view(-1, n_out)[flat_t == -1] == 0)


def test_focal_fixture_every_alpha_and_gamma():
    """fixture g6_focal (the reference's sigmoid_focal_loss in fp32, saturated logits among them): loss and gradient, the bars of
    test_oracle_vs_golden.py::test_focal_edge_cases"""
    g = load('g6_focal')
    x, y = torch.from_numpy(g['x']).double(), torch.from_numpy(g['y']).double()
    n = x.numel()
    pairs = sorted((float(k[6:].split('_g')[0]), float(k.split('_g')[1])) for k in g if k.startswith('loss_a'))
    assert len(pairs) == 5 and (-1.0, 2.0) in pairs and (0.9, 0.0) in pairs and (0.5, 3.0) in pairs
    for alpha, gamma in pairs:
        for lengths in (None, torch.tensor([n])):
            got = O.loss_reference(x.view(1, n, 1), y.view(1, n), lengths, O.FOCAL, alpha, gamma)
            want = float(g[f'loss_a{alpha}_g{gamma}'])
            assert got['count'] == n
            assert abs(got['loss'] - want) < 3e-7 * max(1.0, abs(want)), (alpha, gamma)                    # the fixture is fp32
            np.testing.assert_allclose(got['dscores'].view(-1).numpy(), g[f'grad_a{alpha}_g{gamma}'], rtol=2e-4, atol=1e-8)


def test_bce_saturated_rows_have_a_finite_gradient():
    """x = +-40: sigmoid is exactly 1 / about 4e-18 in fp64.  The loss is nn.BCELoss's (log clamped at -100); the gradient is that of the clamped
    logs, 0 where the clamp is active -- bce_on_probs itself hands autograd 0 / 0 = NaN at x = 40."""
    x = torch.tensor([0.0, 40.0, -40.0, 40.0, -40.0], dtype=torch.float64).view(1, 5, 1)
    y = torch.tensor([[1.0, 0.0, 1.0, 1.0, 0.0]], dtype=torch.float64)
    got = O.loss_reference(x, y, None, O.BCE)
    assert abs(got['loss'] - float(torch.nn.BCELoss()(torch.sigmoid(x.view(-1)), y.view(-1)))) < 1e-12
    assert abs(got['loss'] - float(R.bce_on_probs(x.view(-1), y.view(-1)))) < 1e-12
    assert abs(got['loss'] - (np.log(2.0) + 100.0 + 40.0) / 5) < 1e-9
    ds = got['dscores'].view(-1) * 5
    assert torch.isfinite(ds).all()
    assert abs(float(ds[0]) + 0.5) < 1e-15 and float(ds[1]) == 0.0 and abs(float(ds[2]) + 1.0) < 1e-15 and abs(float(ds[3])) < 1e-15 and abs(float(ds[4])) < 1e-15


@pytest.mark.parametrize('kind', [O.FOCAL, O.BCE, O.CE])
def test_all_ignored_batch_is_zero(kind):
    n_out = 2 if kind == O.CE else 1
    sc, tg, _ = _batch(n_out, seed=3)
    got = O.loss_reference(sc, torch.full_like(tg, -1.0), torch.zeros(B, dtype=torch.long), kind)
    assert got['loss'] == 0.0 and got['count'] == 0 and torch.all(got['dscores'] == 0)


def _tail_inputs(D, n_out, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * L, D, generator=g, dtype=torch.float64) * 1.7 + 0.3
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g, dtype=torch.float64), 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    hw, hb = torch.randn(n_out, D, generator=g, dtype=torch.float64) / D ** 0.5, torch.randn(n_out, generator=g, dtype=torch.float64)
    return x, gamma, beta, hw, hb


@pytest.mark.parametrize('kind', [O.FOCAL, O.BCE, O.CE])
def test_tail_against_torch_operators_padded_and_packed(kind):
    """tail_reference against F.layer_norm + F.linear + the restatement's loss, gradients of grad_scale * loss; then the packed description of the same
    batch (only the valid rows are given): the same loss, count, and the same numbers on the rows that both hold"""
    n_out, D, eps, gs = (2 if kind == O.CE else 1), 24, 1e-5, 0.5
    x, gamma, beta, hw, hb = _tail_inputs(D, n_out, 20 + kind)
    _, tg, lengths = _batch(n_out, seed=30 + kind)
    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta, hw, hb)]
    sc = F.linear(F.layer_norm(leaves[0], (D,), leaves[1], leaves[2], eps), leaves[3], leaves[4])
    loss = R.tagger_loss(sc.view(B, L, n_out), lengths, tg, O.KIND_NAMES[kind], 0.9, 2.0)
    want = torch.autograd.grad(gs * loss, leaves)
    got = O.tail_reference(x, gamma, beta, eps, hw, hb, tg, lengths, kind, 0.9, 2.0, gs, (B, L))
    assert got['count'] == sum(LENGTHS) and abs(got['loss'] - loss.item()) <= 1e-13 * max(1.0, abs(loss.item()))
    assert torch.allclose(got['scores'], sc.detach(), rtol=0, atol=1e-13)
    for name, w in zip(('dx', 'dgamma', 'dbeta', 'dhead_w', 'dhead_b'), want):
        assert float(w.abs().max()) > 0
        assert float((got[name] - w).abs().max()) <= 1e-12 * float(w.abs().max()), name
    rs = O.pack_rows(LENGTHS, L)
    pk = O.tail_reference(x[rs.long()], gamma, beta, eps, hw, hb, tg, lengths, kind, 0.9, 2.0, gs, (B, L), rs)
    assert pk['count'] == got['count'] and abs(pk['loss'] - got['loss']) <= 1e-14
    assert torch.allclose(pk['scores'], got['scores'][rs.long()], rtol=0, atol=1e-14)
    assert torch.allclose(pk['dx'], got['dx'][rs.long()], rtol=0, atol=1e-16)
    pad = torch.ones(B * L, dtype=torch.bool)
    pad[rs.long()] = False
    assert torch.all(got['dx'][pad] == 0)                                    # rows outside a document: gradient exactly 0
    for name in ('dgamma', 'dbeta', 'dhead_w', 'dhead_b'):
        assert float((pk[name] - got[name]).abs().max()) <= 1e-13 * float(got[name].abs().max()), name
    # the backward half alone, fed the loss gradient at those scores, gives the same gradients
    ds = O.loss_reference(got['scores'].view(B, L, n_out), tg, lengths, kind, 0.9, 2.0)['dscores'].view(B * L, n_out) * gs
    bw = O.tail_backward_reference(x, gamma, beta, eps, hw, hb, ds)
    for name in ('dx', 'dgamma', 'dbeta', 'dhead_w', 'dhead_b'):
        assert float((bw[name] - got[name]).abs().max()) <= 1e-12 * float(got[name].abs().max()), name


@pytest.mark.parametrize('n_out', [1, 2, 3, 4])
def test_decode_reference(n_out):
    sc, _, lengths = _batch(n_out, seed=40 + n_out)
    for th in (0.4, 0.5, 0.05, 0.95):
        tags, prob = O.decode_reference(sc, lengths, th)
        if n_out <= 2:
            assert O.decode_lists(tags, lengths) == R.greedy_decode(sc, lengths, th, bce=(n_out == 1))
        e = torch.exp(sc - sc.max(-1, keepdim=True).values)
        want_p = 1 / (1 + torch.exp(-sc[..., 0])) if n_out == 1 else e[..., 1] / e.sum(-1)
        assert torch.allclose(prob, want_p, rtol=1e-13, atol=0)
        for b, n in enumerate(LENGTHS):
            assert tags[b, :n].tolist() == (want_p[b, :n] > th).to(torch.uint8).tolist()
            assert int(tags[b, n:].sum()) == 0
    tags, prob = O.decode_reference(torch.zeros(1, 3, n_out, dtype=torch.float64), None, 1.0 / max(n_out, 2))
    assert int(tags.sum()) == 0                                               # p == threshold: strict >
