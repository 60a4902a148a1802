"""GPU tests of the cosine auxiliary segment loss: the segment-cosine kernels against fp64 on their own operands, BiLSTM / BiLSTMLateFusion
with `segments=` against the reference's fixture g21 and the fp64 oracle (tests/cosine_oracle.py), the two front ends, and the plumbing
(TextSegmenter(cosine_loss=True), NativeTrainer(cosine_loss=True)) end to end."""
import numpy as np
import pytest
import torch

from tests import cosine_oracle as O
from tests.helpers import load, seeded_param
from tests.test_cosine_cpu import CASES, case
from tests.test_gpu_recurrent_longt5 import _check

pytestmark = pytest.mark.gpu

GUARD = 5          # rows behind the batch
GUARD_COLS = 16    # columns behind W (ldx = W + 16: rows stay 16-byte aligned in both dtypes)
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def _ends_every(rng, n, lo, hi):
    ends, s = [], 0
    while True:
        s += int(rng.integers(lo, hi))
        if s > n:
            return ends
        ends.append(s)


def _kernel_case(name):
    """(B, L, W), lengths, segments.  W 16: below one 16-byte vector per lane; 64 / 512: whole lanes; 528 and 1040: a partial second (bf16:
    first / third) lane pass; L = 1 and 2: the smallest documents; 257 rows in one segment next to singletons; the bench shape with a
    boundary about every 10 rows."""
    rng = np.random.default_rng(len(name) + 17)
    if name == 'one_row':
        return (1, 1, 16), [1], [[1]]
    if name == 'two_rows':
        return (1, 2, 16), [2], [[2]]
    if name == 'mixed':
        return (3, 23, 64), [23, 17, 9], [[1, 4, 9, 16, 23], [5, 6, 12], []]
    if name == 'long_segment':
        return (2, 257, 512), [257, 200], [[257], [1, 2, 3, 100, 101]]
    if name == 'w528':
        lengths = [64, 1, 37, 50, 2]
        return (5, 64, 528), lengths, [_ends_every(rng, n, 1, 9) for n in lengths]
    if name == 'w1040':
        lengths = [31, 18]
        return (2, 31, 1040), lengths, [_ends_every(rng, n, 1, 6) for n in lengths]
    assert name == 'bench'
    lengths = [int(v) for v in rng.integers(128, 257, size=64)]
    lengths[0] = 256
    return (64, 256, 512), lengths, [_ends_every(rng, n, 5, 16) for n in lengths]


KERNEL_CASES = ['one_row', 'two_rows', 'mixed', 'long_segment', 'w528', 'w1040', 'bench']
_REFERENCE = {}


def _operands_and_reference(name, dtype):
    """x (with guard rows and columns) and its fp64 cosine loss / per-pair cosines / gradient of the MEAN loss: computed once per
    (case, dtype) and shared, never modified.  The bench shape (seconds of fp64 autograd) uses bf16-exact operands in both modes and
    shares one reference between them."""
    key = (name, 'bf16' if name == 'bench' else dtype)
    if key not in _REFERENCE:
        (B, L, W), lengths, segments = _kernel_case(name)
        torch.manual_seed(1000 * B + L + W)
        x = (torch.randn(B * L + GUARD, W + GUARD_COLS) * 0.5).to(DTYPES[key[1]])
        e = x[:B * L, :W].double().reshape(B, L, W).clone().requires_grad_(True)
        loss, cos, tgt = O.cosine_loss(e, lengths, segments)
        loss.backward()
        _REFERENCE[key] = (x, loss.detach(), cos.detach(), tgt, e.grad.reshape(B * L, W))
    return _REFERENCE[key]


def _run(ops, x, tab, W, scale, dx, accumulate):
    N = tab.B * tab.L
    out = torch.full((2 + GUARD,), 7.0, device='cuda')
    pc = torch.full((tab.n_pair + GUARD,), 7.0, device='cuda')
    ws = ops.segment_cosine_fwd(x[:N, :W], tab, out[:2], pc[:tab.n_pair])
    ops.segment_cosine_bwd(tab, scale, dx[:N, :W], ws, accumulate=accumulate)
    return out, pc


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', KERNEL_CASES)
def test_segment_cosine_kernels_against_fp64(name, dtype):
    from multimodaltopicsegmentation_amd import ops
    (B, L, W), lengths, segments = _kernel_case(name)
    dt, N, dev = DTYPES[dtype], B * L, 'cuda'
    x_h, loss_ref, cos_ref, tgt, gx_ref = _operands_and_reference(name, dtype)
    x = x_h.to(dt).to(dev)
    x0 = x.clone()
    tab = ops.segment_tables(segments, torch.tensor(lengths), B, L, dev)
    P = tab.n_pair
    assert P == cos_ref.numel() and P > 0
    # the kernel multiplies the gradient of the SUM of the terms by `scale` (the caller folds 1 / P in): chosen from the reference so that
    # the largest expected element is 1 and the elementwise bar means something
    gmax = float(gx_ref.abs().max())
    mult = 1.0 / gmax if gmax > 0 else 1.0
    scale = mult / P
    dx = torch.full((N + GUARD, W + GUARD_COLS), 7.0, dtype=dt, device=dev)
    out, pc = _run(ops, x, tab, W, scale, dx, False)
    dx2 = torch.full((N + GUARD, W + GUARD_COLS), 3.0, dtype=dt, device=dev)
    out2, pc2 = _run(ops, x, tab, W, scale, dx2, False)                   # a second forward and backward
    base = (torch.randn(N + GUARD, W + GUARD_COLS) * 0.01).to(dt).to(dev)
    acc = base.clone()
    _run(ops, x, tab, W, scale, acc, True)
    row_map = tab.row_map.cpu()
    outside = (row_map < 0).to(dev)                                       # rows past the length, documents with []
    xg = x.clone()
    xg[:N][outside] = float('nan')                                        # garbage in rows no segment holds
    xg[N:] = float('nan')
    xg[:, W:] = float('nan')
    dxg = torch.full((N + GUARD, W + GUARD_COLS), 7.0, dtype=dt, device=dev)
    outg, pcg = _run(ops, xg, tab, W, scale, dxg, False)
    torch.cuda.synchronize()

    assert torch.equal(x, x0)                                             # inputs unmodified
    assert (out[2:] == 7.0).all() and (pc[P:] == 7.0).all()
    assert (dx[N:].float() == 7.0).all() and (dx[:N, W:].float() == 7.0).all()           # guard rows and guard columns
    assert (acc[N:] == base[N:]).all() and (acc[:N, W:] == base[:N, W:]).all()
    assert torch.equal(out2, out) and torch.equal(pc2, pc) and torch.equal(dx2[:N, :W], dx[:N, :W])      # bitwise repeatable
    assert torch.equal(outg, out) and torch.equal(pcg, pc) and torch.equal(dxg[:N, :W], dx[:N, :W])      # garbage changes no bit
    got = dx[:N, :W]
    assert (got[outside].float() == 0).all() and outside.sum().item() == N - sum(n for n, e in zip(lengths, segments) if e)
    assert torch.equal(acc[:N, :W][outside], base[:N, :W][outside])       # accumulate: rows in no segment are left alone
    # accumulate = write-then-add: bitwise in fp32 (one fp32 add either way); in bf16 the sum is rounded once instead of twice, so the
    # two differ by at most the rounding of the written term plus the rounding of the sum: bf16 keeps 8 significant bits, unit roundoff
    # 2^-8, so 2^-8 (|term| + |sum|)
    wta = base[:N, :W].float() + got.float()
    if dtype == 'fp32':
        assert torch.equal(acc[:N, :W], wta)
    else:
        assert ((acc[:N, :W].float() - wta).abs() <= 2.0 ** -8 * 1.01 * (got.float().abs() + wta.abs())).all()

    assert out[1].item() == P
    print(f'{name} {dtype}: P {P}, loss {out[0].item():.8f} fp64 {loss_ref.item():.8f}, max |d cos| {(pc[:P].cpu().double() - cos_ref).abs().max().item():.2e}')
    _check(out[:1], loss_ref.reshape(1), torch.float32, 'loss')           # fp32 sums over the kernel's own operands: the fp32 bar in both modes
    _check(pc[:P], cos_ref, torch.float32, 'cos')
    _check(got, mult * gx_ref, dt, 'dx')
    neg = cos_ref[(tgt < 0)]
    if name == 'one_row':
        assert P == 1 and out[0].item() == 0.0 and pc[0].item() == 0.0 and not got.any()      # one pair with an empty partner: exactly 0
    elif name != 'two_rows':
        assert (neg > 0.01).any() and (neg < -0.01).any()                 # the random operands reach both sides of the clamp


def test_no_pair_and_refused_operands():
    from multimodaltopicsegmentation_amd import ops
    dev = 'cuda'
    # P = 0: {0, 0}, nothing launched; the backward adds nothing / writes zeros
    tab = ops.segment_tables([[], []], torch.tensor([4, 2]), 2, 4, dev)
    assert tab.n_pair == 0 and tab.n_seg == 0
    x = torch.randn(8, 32, device=dev).to(torch.bfloat16)
    out = torch.full((2,), 7.0, device=dev)
    ws = ops.segment_cosine_fwd(x, tab, out)
    dx = torch.full((8, 32), 7.0, dtype=torch.bfloat16, device=dev)
    ops.segment_cosine_bwd(tab, 1.0, dx, ws, accumulate=True)
    torch.cuda.synchronize()
    assert out.tolist() == [0.0, 0.0] and (dx.float() == 7.0).all()
    ops.segment_cosine_bwd(tab, 1.0, dx, ws, accumulate=False)
    torch.cuda.synchronize()
    assert not dx.any()
    # refused before any launch: W no whole 16-byte vectors, a misaligned base, a misaligned leading dimension
    tab = ops.segment_tables([[2, 4]], torch.tensor([4]), 1, 4, dev)
    out = torch.full((2,), 7.0, device=dev)
    for dt, W in ((torch.bfloat16, 12), (torch.float32, 6)):
        x = torch.ones(4, W, dtype=dt, device=dev)
        dx = torch.full((4, W), 7.0, dtype=dt, device=dev)
        with pytest.raises(NotImplementedError):
            ops.segment_cosine_fwd(x, tab, out)
        with pytest.raises(NotImplementedError):
            ops.segment_cosine_bwd(tab, 1.0, dx, torch.zeros(4096, dtype=torch.uint8, device=dev), accumulate=False)
        assert (dx.float() == 7.0).all()
    off = torch.ones(4 * 32 + 1, dtype=torch.bfloat16, device=dev)[1:].view(4, 32)       # 2-byte offset base
    odd_ld = torch.ones(4, 36, dtype=torch.bfloat16, device=dev)[:, :32]                 # rows 72 bytes apart
    good = torch.ones(4, 32, dtype=torch.bfloat16, device=dev)
    for bad in (off, odd_ld):
        with pytest.raises(NotImplementedError):
            ops.segment_cosine_fwd(bad, tab, out)
    ws = ops.segment_cosine_fwd(good, tab, torch.empty(2, device=dev))
    dbad = torch.full((4 * 32 + 1,), 7.0, dtype=torch.bfloat16, device=dev)
    with pytest.raises(NotImplementedError):
        ops.segment_cosine_bwd(tab, 1.0, dbad[1:].view(4, 32), ws, accumulate=False)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (dbad.float() == 7.0).all()


# ------------------------------------------------------------------------------------------------ model level
def _model(cs, dtype, seed=0):
    from multimodaltopicsegmentation_amd import BiLSTM, BiLSTMLateFusion
    cls = BiLSTMLateFusion if cs['late'] else BiLSTM
    m = cls(2, list(cs['D']) if cs['late'] else cs['D'], cs['H'], cs['NL'], loss_fn=cs['loss_fn'], compute_dtype=dtype, seed=seed)
    m.load_state_dict({n: t.float() for n, t in cs['p'].items()})
    return m.cuda().eval()


def _grads(m):
    return {n: m.logical_view({n: t.grad.detach()}, n).cpu().double().numpy() for n, t in m.named_parameters()}


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('c', CASES)
def test_fixture_g21(c, dtype):
    """test_fixture_g19's bars: loss 2e-5 / 3e-2 relative, gradients element by element 1e-4 max(1e-3, max |g|) in fp32 and per-tensor
    L2 <= 0.1 ||g|| in bf16; the same for the batch without any pair (cosine term 0, main loss unmasked)."""
    g = load('g21_cosine_loss')
    cs = case(g, c, torch.float32)
    m = _model(cs, dtype)
    xs = [x.cuda() for x in cs['xs']]
    lengths, tags = cs['lengths'], cs['tags'].cuda()
    m.zero_grad()
    loss = m.loss(*xs, lengths, tags, segments=cs['segments'])
    loss.backward()
    want = float(g[f'{c}_loss'])
    print(f'g21 {c} {dtype}: loss {loss.item():.8f} reference {want:.8f}')
    assert abs(loss.item() - want) < (2e-5 if dtype == 'fp32' else 3e-2) * abs(want)
    grads = _grads(m)
    assert sorted('g.' + n for n in grads) == sorted(k[len(c) + 1:] for k in g if k.startswith(f'{c}_g.'))
    for n, got in grads.items():
        w = g[f'{c}_g.{n}']
        assert got.shape == w.shape, n
        if dtype == 'fp32':
            assert np.abs(got - w).max() <= 1e-4 * max(1e-3, np.abs(w).max()), (n, np.abs(got - w).max(), np.abs(w).max())
        else:
            assert np.linalg.norm(got - w) <= 0.1 * np.linalg.norm(w), (n, np.linalg.norm(got - w) / np.linalg.norm(w))
    m.zero_grad()
    loss0 = m.loss(*xs, lengths, tags, segments=[[] for _ in cs['segments']])
    loss0.backward()
    want0 = float(g[f'{c}_p0_loss'])
    assert abs(loss0.item() - want0) < (2e-5 if dtype == 'fp32' else 3e-2) * abs(want0)
    gb, wb = _grads(m)['classification.bias'], g[f'{c}_p0_g.classification.bias']
    if dtype == 'fp32':
        assert np.abs(gb - wb).max() <= 1e-4 * max(1e-3, np.abs(wb).max())
    else:
        assert np.linalg.norm(gb - wb) <= 0.1 * np.linalg.norm(wb)


def test_reference_errors_on_the_device_path():
    from multimodaltopicsegmentation_amd import BiLSTM
    g = load('g21_cosine_loss')
    cs = case(g, 'bc', torch.float32)
    x, lengths, tags = cs['xs'][0].cuda(), cs['lengths'], cs['tags'].cuda()
    long_tags = torch.cat((tags, torch.full((tags.shape[0], 1), -1.0, device='cuda')), dim=1)
    pad = tags.clone()
    for b, n in enumerate(lengths.tolist()):
        pad[b, n:] = -1
    for loss_fn in ('FocalLoss', 'BinaryCrossEntropy', 'CrossEntropy'):
        m = BiLSTM(2, cs['D'], cs['H'], cs['NL'], loss_fn=loss_fn, compute_dtype='fp32', seed=1).cuda()
        with pytest.raises(ValueError) as e:
            m.loss(x, lengths, long_tags, segments=cs['segments'])
        assert str(e.value) == str(g[f'err_tags_{loss_fn}_msg'])
        with pytest.raises(IndexError) as e:
            m.loss(x, lengths, tags, segments=cs['segments'][:-1])
        assert str(e.value) == str(g['err_short_msg'])
        with pytest.raises(ValueError):
            m.loss(x, lengths, tags, segments=[[4, 3, 11, 19], [2, 5], []])           # not ascending: refused before any launch
        if loss_fn == 'BinaryCrossEntropy':
            with pytest.raises(RuntimeError) as e:
                m.loss(x, lengths, pad, segments=cs['segments'])
            assert str(e.value) == str(g['err_bce_pad_msg'])
        else:
            assert np.isfinite(m.loss(x, lengths, pad, segments=cs['segments']).item())


def _small_batch(seed=3, B=4, L=30, D=64, lengths=(30, 12, 1, 22)):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.tensor(lengths)
    x = torch.randn(B, L, D, generator=g)
    tags = torch.full((B, L), -1.0)
    for b, n in enumerate(lengths.tolist()):
        tags[b, :n] = (torch.rand(n, generator=g) < 0.3).float()
        tags[b, n - 1] = 0
    return x, lengths, tags


SMALL_SEGMENTS = [[3, 4, 11, 30], [5, 9], [1], []]


@pytest.mark.parametrize('arch', ['BiLSTM', 'BiLSTMLateFusion'])
@pytest.mark.parametrize('H', [32, 12])
def test_front_ends_agree_bitwise(arch, H):
    """loss_and_grad and the autograd front end: the same bits, with segments; segments=None: the same bits as the call without it."""
    from multimodaltopicsegmentation_amd import BiLSTM, BiLSTMLateFusion
    x, lengths, tags = _small_batch()
    x2 = _small_batch(seed=4, D=24)[0]
    late = arch == 'BiLSTMLateFusion'
    m = (BiLSTMLateFusion(2, [64, 24], H, 2, loss_fn='FocalLoss', compute_dtype='fp32', seed=5) if late
         else BiLSTM(2, 64, H, 2, loss_fn='FocalLoss', compute_dtype='fp32', seed=5)).cuda()
    xs = (x.cuda(), x2.cuda()) if late else (x.cuda(),)
    tg = tags.cuda()
    loss, _ = m.loss_and_grad(*xs, lengths, tg, True, segments=SMALL_SEGMENTS)
    loss = loss.item()
    native = {n: v.clone() for n, v in m.grad_views().items()}
    assert all(torch.isfinite(v).all() for v in native.values()) and sum(float(v.abs().sum()) for v in native.values()) > 0
    m.grad_flat().zero_()
    m.zero_grad()
    l2 = m.loss(*xs, lengths, tg, segments=SMALL_SEGMENTS)
    assert l2.requires_grad and l2.item() == loss
    l2.backward()
    for n, prm in m.named_parameters():
        assert torch.equal(prm.grad, native[n]), n
    with torch.no_grad():
        assert m.loss(*xs, lengths, tg, segments=SMALL_SEGMENTS).item() == loss
    # segments=None is the call without the argument
    la, _ = m.loss_and_grad(*xs, lengths, tg, True)
    la, ga = la.item(), m.grad_flat().clone()
    lb, _ = m.loss_and_grad(*xs, lengths, tg, True, segments=None)
    assert lb.item() == la and torch.equal(m.grad_flat(), ga) and la != loss
    assert m.loss(*xs, lengths, tg, segments=None).item() == la


@pytest.mark.parametrize('loss_fn', ['FocalLoss', 'CrossEntropy'])
def test_empty_segment_lists_leave_the_unmasked_main_loss(loss_fn):
    """segments = [[]] * B: on an unpadded batch the plain loss, bit for bit; on a ragged one the main loss over ALL positions (the
    reference does not un-pad in this branch), checked against the oracle at the fp32 bar of test_fixture_g21 (2e-5 relative)."""
    from multimodaltopicsegmentation_amd import BiLSTM
    m = BiLSTM(2, 64, 32, 2, loss_fn=loss_fn, compute_dtype='fp32', seed=9).cuda()
    x, lengths, tags = _small_batch(lengths=(30, 30, 30, 30))
    plain, _ = m.loss_and_grad(x.cuda(), lengths, tags.cuda(), True)
    plain, gp = plain.item(), m.grad_flat().clone()
    empty, _ = m.loss_and_grad(x.cuda(), lengths, tags.cuda(), True, segments=[[]] * 4)
    assert empty.item() == plain and torch.equal(m.grad_flat(), gp)
    x, lengths, tags = _small_batch()
    plain = m.loss_and_grad(x.cuda(), lengths, tags.cuda(), False)[0].item()
    empty = m.loss_and_grad(x.cuda(), lengths, tags.cuda(), False, segments=[[]] * 4)[0].item()
    p = {n: t.detach().cpu().double() for n, t in m.state_dict().items()}
    want = O.loss(x.double(), lengths, tags.double(), [[]] * 4, p, loss_fn)[0].item()
    assert abs(empty - want) < 2e-5 * abs(want)
    if loss_fn == 'FocalLoss':
        assert abs(empty - plain) > 1e-3 * abs(plain)                     # the padded positions count (CrossEntropy ignores -1 either way)
    else:
        assert empty == plain


def _mid_case(seed=7):
    B, L, D, H, NL = 8, 96, 128, 256, 2
    rng = np.random.default_rng(seed)
    lengths = [96, 1, 2, 57, 96, 33, 80, 14]
    x = torch.from_numpy(rng.standard_normal((B, L, D)).astype(np.float32)).to(torch.bfloat16).float()      # bf16-exact inputs
    tags = torch.full((B, L), -1.0)
    segments = []
    for b, n in enumerate(lengths):
        x[b, n:] = 0.0
        t = (rng.random(n) < 0.15).astype(np.float32)
        t[-1] = 0
        tags[b, :n] = torch.from_numpy(t)
        segments.append((np.flatnonzero(t == 1) + 1).tolist())            # the collater's rule
    p = {n: torch.from_numpy(seeded_param(n, s, seed)) for n, s in O.param_shapes(D, H, NL, 1).items()}
    return dict(B=B, L=L, D=D, H=H, NL=NL, late=False, loss_fn='FocalLoss', lengths=torch.tensor(lengths), x=x, tags=tags, p=p,
                segments=segments)


def test_mid_size_bf16_against_oracle():
    """test_gpu_parity_fullsize.py's protocol and bars: bf16-exact master weights and inputs on both sides; loss 2e-3 relative; scores of
    every row max <= 3e-2 max(1, max |s_ref|), mean <= 3e-3; every gradient tensor max <= BAR_MAX max |g_ref| and L2 <= BAR_L2 ||g_ref||.
    Precondition on the inputs (not on the result): every negative pair with a partner has |cos| >= 0.05 in the oracle, so bf16 cannot
    flip a clamp."""
    from tests.test_gpu_parity_fullsize import BAR_L2, BAR_MAX, _round_to_bf16_
    cs = _mid_case()
    m = _round_to_bf16_(_model(cs, 'bf16'))
    loss, out = m.loss_and_grad(cs['x'].cuda(), cs['lengths'], cs['tags'].cuda(), True, segments=cs['segments'])
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {n: t.detach().cpu().double().requires_grad_(True) for n, t in m.state_dict().items()}
    l_ref, cos, s_ref = O.loss(cs['x'].double(), cs['lengths'], cs['tags'].double(), cs['segments'], p, 'FocalLoss')
    l_ref.backward()
    s_ref, l_ref = s_ref.detach(), l_ref.detach()
    nonzero = cos.detach()[cos.detach() != 0]
    assert cos.numel() > 40 and float(nonzero.abs().min()) >= 0.05, float(nonzero.abs().min())
    d = (out.detach().cpu().double().view_as(s_ref) - s_ref).abs()
    scale = max(1.0, float(s_ref.abs().max()))
    views = m.grad_views()
    assert set(views) == set(p)
    worst = {}
    for name, gv in views.items():
        a, r = gv.detach().cpu().double(), p[name].grad.double()
        worst[name] = (float((a - r).abs().max()) / float(r.abs().max()), float((a - r).norm()) / float(r.norm()))
    print('cosine 8x96 bf16: loss', float(loss), 'oracle', float(l_ref), 'scores max / mean |d|', float(d.max()), float(d.mean()), 'pairs', cos.numel())
    for name, w in worst.items():
        print(f'  {name}: max-ratio {w[0]:.3e} l2-ratio {w[1]:.3e}')
    assert abs(float(loss) - float(l_ref)) <= 2e-3 * abs(float(l_ref)), (float(loss), float(l_ref))
    assert float(d.max()) <= 3e-2 * scale and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    for name, (rmax, rl2) in worst.items():
        assert rmax <= BAR_MAX and rl2 <= BAR_L2, (name, rmax, rl2)


# ------------------------------------------------------------------------------------------------ end to end
def _dataset(late):
    from multimodaltopicsegmentation_amd.encoder_dataset import AudioPortionDataset
    rng = np.random.default_rng(21)
    lines, second = [], []
    for i, n in enumerate([30, 12, 1, 22]):
        t = (rng.random(n) < 0.3).astype(np.float32)
        t[-1] = 0.0
        lines.append((torch.from_numpy(rng.standard_normal((n, 64)).astype(np.float32)), t.tolist(), f'doc{i}'))
        second.append((torch.from_numpy(rng.standard_normal((n, 24)).astype(np.float32)), t.tolist(), f'doc{i}'))
    ds = AudioPortionDataset(lines, None, CRF=False, truncate=False, second_input=second if late else None, segments=True)
    batch = ds.collater([ds[i] for i in range(4)])
    assert sum(len(s) for s in batch['src_segments']) > 3
    for k in ('src_tokens', 'src_tokens2', 'tgt_tokens'):
        if batch[k] is not None:
            batch[k] = batch[k].cuda()
    return batch


@pytest.mark.parametrize('arch', ['BiLSTM', 'BiLSTMLateFusion'])
def test_text_segmenter_trains_with_the_cosine_loss(arch):
    from multimodaltopicsegmentation_amd import TextSegmenter
    late = arch == 'BiLSTMLateFusion'
    torch.manual_seed(11)
    ts = TextSegmenter(2, [64, 24] if late else 64, 32, num_layers=2, architecture=arch, loss_fn='FocalLoss', cosine_loss=True,
                       compute_dtype='fp32').cuda()
    batch = _dataset(late)
    loss = ts.training_step(batch, 0)
    assert loss.requires_grad and np.isfinite(loss.item())
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in ts.parameters())
    plain = ts.model.loss_and_grad(*([batch['src_tokens'], batch['src_tokens2']] if late else [batch['src_tokens']]), batch['src_lengths'],
                                   batch['tgt_tokens'], False)[0].item()
    assert loss.item() != plain                                           # the segments did reach the model
    with pytest.raises(KeyError, match='src_segments'):
        ts.training_step({k: v for k, v in batch.items() if k != 'src_segments'}, 0)


def test_native_trainer_steps_with_the_cosine_loss():
    from multimodaltopicsegmentation_amd import BiLSTM
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    m = BiLSTM(2, 64, 32, 2, loss_fn='FocalLoss', compute_dtype='bf16', seed=3).cuda()
    batch = _dataset(False)
    before = m.flat.clone()
    tr = NativeTrainer(m, lr=1e-3, optimizer='Adam', cosine_loss=True)
    loss = tr.step(batch)
    assert np.isfinite(loss.item()) and not torch.equal(m.flat, before) and torch.isfinite(m.flat).all()
    want, _ = m.loss_and_grad(batch['src_tokens'], batch['src_lengths'], batch['tgt_tokens'], False, segments=batch['src_segments'])
    assert np.isfinite(want.item()) and want.item() != loss.item()        # the parameters moved
    with pytest.raises(KeyError, match='src_segments'):
        tr.step({k: v for k, v in batch.items() if k != 'src_segments'})
