"""GPU tests of SwitchBiLSTM: the domain-switched head kernels against fp64 on their own operands, and the model against the reference's
fixture g20 and the fp64 oracle (tests/switch_oracle.py)."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests import switch_oracle as O
from tests.helpers import load, seeded_param
from tests.test_gpu_recurrent_longt5 import _check
from tests.test_switch_cpu import CASES, case_params, flat_tags

pytestmark = pytest.mark.gpu

GUARD = 7
PAD = 8                    # x and dx are the left D columns of a buffer D + PAD wide
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}

# (B, L, D, n_out, domains): one row; two documents that both read document 0; odd row counts, mixed groups 3 / 2 and 1 / 4; a head nobody
# uses; D = 528 (no multiple of 256: the bounds-checked parameter kernel, 3 column slots with the last one partial); the bench shape
KERNEL_CASES = [(1, 1, 16, 1, [1]), (2, 2, 16, 1, [1, 0]), (5, 23, 64, 2, [1, 0, 1, 1, 0]), (5, 7, 32, 1, [0, 1, 1, 1, 1]),
                (3, 257, 512, 1, [0, 0, 0]), (4, 64, 528, 2, [1, 1, 0, 1]), (64, 256, 512, 1, [i & 1 for i in range(64)]),
                # the parameter pass's other instantiations (tests/test_instantiation_cover_cpu.py keeps the list)
                (3, 5, 256, 3, [1, 0, 1]),              # NV = 1 full; n_out = 3
                (2, 9, 772, 4, [0, 1]),                 # NV = 4 bounds-checked, the 4th slot holds 4 columns; n_out = 4
                (2, 6, 1024, 2, [1, 1]),                # NV = 4 full; an idle head
                (2, 5, 1028, 1, [1, 0]),                # NV = 8, one chunk, slot 4 holds 4 columns
                (2, 5, 2048, 2, [0, 1]),                # NV = 8 full
                (3, 7, 2052, 3, [1, 1, 0]),             # two chunks, the second 4 columns wide
                (2, 3, 4096, 4, [1, 0]),                # two full-width chunks (bounds-checked: D != 2048)
                # 2061 rows: rows % 4 == 1 and above the 512-workgroup cap, so the pass strides; head 1 has one document, so most of
                # its workgroups take no row and flag 0 sits among flag 1
                (9, 229, 16, 2, [0] * 8 + [1]),
                (2, 5, 260, 2, [0, 1])]                 # NV = 2 bounds-checked, the second slot holds 4 columns


def _reference(x, w, b, ds, doms, B, L, D, n_out):
    """fp64 scores / dw / db / dx of the kernels' own operands, from the maps written out"""
    from multimodaltopicsegmentation_amd import ops
    src, head, tgt = ops.switch_doc_maps(doms, B)
    x64, w64, b64, d64 = x.double().cpu().reshape(B, L, D), w.double().cpu(), b.double().cpu(), ds.double().cpu()
    s = torch.stack([x64[src[i]] @ w64[head[i]].t() + b64[head[i]] for i in range(B)])
    dw, db, dx = torch.zeros(2, n_out, D, dtype=torch.float64), torch.zeros(2, n_out, dtype=torch.float64), torch.zeros(B, L, D, dtype=torch.float64)
    for i in range(B):
        dw[head[i]] += d64[i].t() @ x64[src[i]]
        db[head[i]] += d64[i].sum(0)
        dx[src[i]] += d64[i] @ w64[head[i]]
    unread = [r for r in range(B) if tgt[r] < 0 and tgt[B + r] < 0]
    return s, dw, db, dx, unread, sorted(set((0, 1)) - set(head))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', KERNEL_CASES, ids=[f'B{c[0]}_L{c[1]}_D{c[2]}_n{c[3]}' for c in KERNEL_CASES])
def test_switch_head_kernels_against_fp64(case, dtype):
    from multimodaltopicsegmentation_amd import ops
    B, L, D, n_out, doms = case
    dt, N, dev = DTYPES[dtype], B * L, 'cuda'
    torch.manual_seed(1000 * B + L + D)
    xb = (torch.randn(N + GUARD, D + PAD) * 0.5).to(dt).to(dev)
    w = (torch.randn(2, n_out, D) * 0.5).to(dev)
    b = torch.randn(2, n_out).to(dev)
    ds = torch.randn(B, L, n_out).to(dev)
    keep = [t.clone() for t in (xb, w, b, ds)]
    x = xb[:N, :D]
    scores = torch.full((N + GUARD, n_out), 7.0, device=dev)
    ops.switch_head_fwd(x, w, b, doms, B, L, scores[:N])
    dwb = torch.full((2 * n_out * D + GUARD,), 7.0, device=dev)
    dbb = torch.full((2 * n_out + GUARD,), 7.0, device=dev)
    dw, db = dwb[:2 * n_out * D].view(2, n_out, D), dbb[:2 * n_out].view(2, n_out)
    ops.switch_head_bwd_params(x, ds, doms, B, L, dw, db)
    dxb = torch.full((N + GUARD, D + PAD), 7.0, dtype=dt, device=dev)
    dx = dxb[:N, :D]
    ops.switch_head_bwd_data(ds, w, doms, B, L, dx)
    dw2, db2 = torch.full((2, n_out, D), 3.0, device=dev), torch.full((2, n_out), 3.0, device=dev)
    dx2 = torch.full((N, D), 3.0, dtype=dt, device=dev)
    ops.switch_head_bwd_params(x, ds, doms, B, L, dw2, db2)
    ops.switch_head_bwd_data(ds, w, doms, B, L, dx2)
    torch.cuda.synchronize()

    for t, t0 in zip((xb, w, b, ds), keep):                               # inputs unchanged
        assert torch.equal(t, t0)
    # guard rows behind every output and the columns right of D: still 7.0
    assert (scores[N:] == 7.0).all() and (dwb[2 * n_out * D:] == 7.0).all() and (dbb[2 * n_out:] == 7.0).all()
    assert (dxb[N:].float() == 7.0).all() and (dxb[:N, D:].float() == 7.0).all()
    # a second backward: bitwise the same
    assert torch.equal(dw2, dw) and torch.equal(db2, db) and torch.equal(dx2, dx)

    s_ref, dw_ref, db_ref, dx_ref, unread, idle_heads = _reference(x, w, b, ds, doms, B, L, D, n_out)
    _check(scores[:N].view(B, L, n_out), s_ref, torch.float32, 'scores')   # fp32 sums over the kernel's own operands: the fp32 bar in both modes
    _check(dw, dw_ref, torch.float32, 'dw')
    _check(db, db_ref, torch.float32, 'db')
    _check(dx.reshape(B, L, D), dx_ref, dt, 'dx')
    for r in unread:                                                       # documents nobody reads: exact zeros
        assert not dx.reshape(B, L, D)[r].any(), r
    for k in idle_heads:                                                   # a head no document uses: exact zeros over the stale 7.0
        assert not dw[k].any() and not db[k].any(), k
    if doms == [1, 0]:
        assert unread == [1]
    if doms == [0, 0, 0]:
        assert idle_heads == [0]


def test_switch_head_refuses_uncovered_operands_before_launch():
    from multimodaltopicsegmentation_amd import ops
    dev = 'cuda'
    B, L = 2, 3
    sc, ds = torch.zeros(B * L, 1, device=dev), torch.ones(B, L, 1, device=dev)
    ok = torch.ones(B * L, 16, dtype=torch.bfloat16, device=dev)
    w, b = torch.ones(2, 1, 16, device=dev), torch.ones(2, 1, device=dev)
    dw, db, dx = torch.zeros(2, 1, 16, device=dev), torch.zeros(2, 1, device=dev), torch.zeros(B * L, 16, dtype=torch.bfloat16, device=dev)
    for doms in ([1], [1, 0, 1], [1, 2], [1.0, 0.0], 'ab', None):         # malformed domains
        with pytest.raises(ValueError):
            ops.switch_head_fwd(ok, w, b, doms, B, L, sc)
        with pytest.raises(ValueError):
            ops.switch_head_bwd_params(ok, ds, doms, B, L, dw, db)
        with pytest.raises(ValueError):
            ops.switch_head_bwd_data(ds, w, doms, B, L, dx)
    x18 = torch.ones(B * L, 18, dtype=torch.float32, device=dev)         # D % 4 != 0
    w18, dw18 = torch.ones(2, 1, 18, device=dev), torch.zeros(2, 1, 18, device=dev)
    with pytest.raises(ValueError):
        ops.switch_head_fwd(x18, w18, b, [1, 0], B, L, sc)
    with pytest.raises(ValueError):
        ops.switch_head_bwd_params(x18, ds, [1, 0], B, L, dw18, db)
    with pytest.raises(ValueError):
        ops.switch_head_bwd_data(ds, w18, [1, 0], B, L, torch.zeros_like(x18))
    off = torch.ones(B * L * 16 + 1, dtype=torch.bfloat16, device=dev)[1:].view(B * L, 16)     # 2-byte offset base: no 8-byte vectors
    with pytest.raises(ValueError):
        ops.switch_head_fwd(off, w, b, [1, 0], B, L, sc)
    with pytest.raises(ValueError):
        ops.switch_head_bwd_params(off, ds, [1, 0], B, L, dw, db)
    with pytest.raises(ValueError):
        ops.switch_head_bwd_data(ds, w, [1, 0], B, L, off)
    with pytest.raises(ValueError):                                        # a row stride that is no multiple of 4
        ops.switch_head_fwd(torch.ones(B * L, 18, dtype=torch.bfloat16, device=dev)[:, :16], w, b, [1, 0], B, L, sc)
    torch.cuda.synchronize()
    assert not sc.any() and not dw.any() and not db.any() and not dx.any()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_parameter_pass_refuses_what_it_does_not_cover(dtype):
    """D = 4100 > 4096: the parameter pass (two column chunks of 8 x 256 at the most) raises NotImplementedError and writes nothing; the
    forward and the data pass have no such limit and are right there."""
    from multimodaltopicsegmentation_amd import ops
    B, L, D, n_out, doms = 2, 3, 4100, 2, [1, 0]
    dt, N, dev = DTYPES[dtype], B * L, 'cuda'
    torch.manual_seed(4100)
    x = (torch.randn(N, D) * 0.5).to(dt).to(dev)
    w, b, ds = (torch.randn(2, n_out, D) * 0.5).to(dev), torch.randn(2, n_out).to(dev), torch.randn(B, L, n_out).to(dev)
    dw, db = torch.full((2, n_out, D), 7.0, device=dev), torch.full((2, n_out), 7.0, device=dev)
    with pytest.raises(NotImplementedError, match='4096'):
        ops.switch_head_bwd_params(x, ds, doms, B, L, dw, db)
    scores = torch.full((N + GUARD, n_out), 7.0, device=dev)
    ops.switch_head_fwd(x, w, b, doms, B, L, scores[:N])
    dxb = torch.full((N + GUARD, D), 7.0, dtype=dt, device=dev)
    ops.switch_head_bwd_data(ds, w, doms, B, L, dxb[:N])
    torch.cuda.synchronize()
    assert (dw == 7.0).all() and (db == 7.0).all()
    assert (scores[N:] == 7.0).all() and (dxb[N:].float() == 7.0).all()
    s_ref, _, _, dx_ref, unread, _ = _reference(x, w, b, ds, doms, B, L, D, n_out)
    _check(scores[:N].view(B, L, n_out), s_ref, torch.float32, 'scores')
    _check(dxb[:N].reshape(B, L, D), dx_ref, dt, 'dx')
    assert unread == [1] and not dxb[:N].reshape(B, L, D)[1].any()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_map_entries_outside_their_range_contribute_nothing(dtype):
    """csrc/switch_head.hip: "A map entry outside its range contributes nothing: the row is written as 0 (forward, data) or skipped
    (params), and no address is ever formed from it."  The wrappers build valid maps only, so the maps here are hand-built and go through
    the C ABI.  x and ds carry one guard document of finite nonzero values in front of and behind the B documents, so whatever row a
    kernel that ignored its range check formed from -1 or 4 lies inside the test's own buffers and shows as a wrong number."""
    from multimodaltopicsegmentation_amd import _lib as Lb
    from multimodaltopicsegmentation_amd.ops import dtype_code, ptr, stream_ptr
    B, L, D, n_out = 4, 6, 64, 2
    dt, N, dev = DTYPES[dtype], B * L, 'cuda'
    doc_src, doc_head = [0, 4, -1, 2], [1, 0, 0, 2]
    doc_tgt = [[-1, 4, 0, -7], [1, -1, 9, -1]]          # -7 and 9: the data pass alone reads doc_tgt, as (unsigned)tg < (unsigned)B
    src, head = (torch.tensor(v, dtype=torch.int32, device=dev) for v in (doc_src, doc_head))
    tgt = torch.tensor(doc_tgt, dtype=torch.int32, device=dev).reshape(-1)
    torch.manual_seed(46)
    xg = (torch.randn((B + 2) * L, D) * 0.5 + 3.0).to(dt).to(dev)          # guard documents included: nowhere near 0
    dsg = (torch.randn(B + 2, L, n_out) + 3.0).to(dev)
    w, b = (torch.randn(2, n_out, D) * 0.5).to(dev), (torch.randn(2, n_out) + 3.0).to(dev)
    x, ds = xg[L:L + N], dsg[1:1 + B]                                      # the interior: what the kernels are handed
    scores = torch.full((N + GUARD, n_out), 7.0, device=dev)
    dw, db = torch.full((2, n_out, D), 7.0, device=dev), torch.full((2, n_out), 7.0, device=dev)
    dxb = torch.full((N + GUARD, D), 7.0, dtype=dt, device=dev)
    ws = torch.empty(Lb.lib.mts_switch_head_bwd_workspace(D), dtype=torch.uint8, device=dev)
    code = dtype_code(dt)
    Lb.check(Lb.lib.mts_switch_head_fwd(stream_ptr(), code, B, L, D, n_out, ptr(x), D, ptr(w), ptr(b), ptr(src), ptr(head), ptr(scores)))
    Lb.check(Lb.lib.mts_switch_head_bwd_params(stream_ptr(), code, B, L, D, n_out, ptr(x), D, ptr(ds), ptr(src), ptr(head), ptr(dw), ptr(db),
                                               ptr(ws)))
    Lb.check(Lb.lib.mts_switch_head_bwd_data(stream_ptr(), code, B, L, D, n_out, ptr(ds), ptr(w), ptr(tgt), ptr(dxb), D))
    torch.cuda.synchronize()
    x64, d64, w64, b64 = x.double().cpu().view(B, L, D), ds.double().cpu(), w.double().cpu(), b.double().cpu()
    sc = scores[:N].view(B, L, n_out)
    assert (scores[N:] == 7.0).all() and (dxb[N:].float() == 7.0).all()
    # forward: document 0 from its own rows under head 1; source 4, source -1 and head 2 are out of range: exact zeros, no bias either
    _check(sc[0], x64[0] @ w64[1].t() + b64[1], torch.float32, 'scores of document 0')
    assert not sc[1:].any()
    # parameters: document 0's contribution only, under head 1; head 0 (documents 1 and 2, neither with a source in range): exact zeros
    _check(dw[1], d64[0].t() @ x64[0], torch.float32, 'dw of head 1')
    _check(db[1], d64[0].sum(0), torch.float32, 'db of head 1')
    assert not dw[0].any() and not db[0].any()
    # data: row 0 is read by document 1 under head 1, row 2 by document 0 under head 0; rows 1 and 3 have no entry in range: exact zeros
    dx = dxb[:N].view(B, L, D)
    _check(dx[0], d64[1] @ w64[1], dt, 'dx of document 0')
    _check(dx[2], d64[0] @ w64[0], dt, 'dx of document 2')
    assert not dx[1].any() and not dx[3].any()


# ------------------------------------------------------------------------------------------------ model level
def _model(cs, p, dtype, **kw):
    from multimodaltopicsegmentation_amd import SwitchBiLSTM
    m = SwitchBiLSTM(2, cs['D'], cs['H'], cs['NL'], loss_fn=cs['loss_fn'], switch_lstm_adapt=cs['mode'] == 'lstm',
                     switch_dense_adapt=cs['mode'] == 'dense', compute_dtype=dtype, seed=0, **kw)
    m.load_state_dict({n: t.float() for n, t in p.items()})
    return m.cuda().eval()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('c', CASES)
def test_fixture_g20(c, dtype):
    """test_fixture_g19's bars: scores of every row 2e-5 / 5e-2 x max(1, max |ref|), loss 2e-5 / 3e-2 relative, gradients element by element
    1e-4 max(1e-3, max |g|) in fp32 and per-tensor L2 <= 0.1 ||g|| in bf16, decode lists identical in fp32; the names whose grad is None
    through loss().backward() are the reference's."""
    g = load('g20_switch_bilstm')
    cs, p = case_params(g, c, torch.float32)
    m = _model(cs, p, dtype)
    x, lengths, tags, doms = cs['x'].cuda(), cs['lengths'], cs['tags'].cuda(), cs['domains']
    ref = torch.from_numpy(g[f'{c}_scores'])
    for th in g[f'{c}_ths'].tolist():
        m.th = th
        scores, tag_lists = m(x, lengths, doms)
        assert scores.shape == ref.shape
        err = (scores.cpu() - ref).abs().max().item()
        print(f'g20 {c} {dtype}: scores max err {err:.3e} (max |ref| {ref.abs().max().item():.3f})')
        assert err < (2e-5 if dtype == 'fp32' else 5e-2) * max(1.0, ref.abs().max().item())
        if dtype == 'fp32':
            assert flat_tags(tag_lists).tolist() == g[f'{c}_tags{th}'].tolist(), th
    m.zero_grad()
    loss = m.loss(x, lengths, tags, doms)
    loss.backward()
    want = float(g[f'{c}_loss'])
    print(f'g20 {c} {dtype}: loss {loss.item():.8f} reference {want:.8f}')
    assert abs(loss.item() - want) < (2e-5 if dtype == 'fp32' else 3e-2) * abs(want)
    assert sorted(n for n, t in m.named_parameters() if t.grad is None) == sorted(g[f'{c}_none_keys'].tolist())
    grads = {n: m.logical_view({n: t.grad.detach()}, n).cpu().double().numpy() for n, t in m.named_parameters() if t.grad is not None}
    assert sorted(grads) == sorted(k[len(c) + 3:] for k in g if k.startswith(f'{c}_g.'))
    for n, got in grads.items():
        w = g[f'{c}_g.{n}']
        assert got.shape == w.shape, n
        if dtype == 'fp32':
            assert np.abs(got - w).max() <= 1e-4 * max(1e-3, np.abs(w).max()), (n, np.abs(got - w).max(), np.abs(w).max())
        else:
            assert np.linalg.norm(got - w) <= 0.1 * np.linalg.norm(w), (n, np.linalg.norm(got - w) / np.linalg.norm(w))
    # the spans the batch did not read are zeros in the flat gradient
    views = m.grad_views()
    for n in g[f'{c}_none_keys'].tolist():
        assert not views[n].any(), n


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
    p = {n: torch.from_numpy(seeded_param(n, s, seed)) for n, s in O.param_shapes(D, H, NL, 1, 'dense').items()}
    return dict(B=B, L=L, D=D, H=H, NL=NL, lengths=torch.tensor(lengths), x=x, tags=tags, p=p, domains=[1, 0, 0, 1, 1, 0, 1, 0],
                loss_fn='FocalLoss', mode='dense')


def test_mid_size_bf16_against_oracle():
    """test_gpu_parity_fullsize.py's protocol and bars: bf16-exact master weights and inputs on both sides; loss 2e-3 relative; scores of
    every row (padded ones included) max <= 3e-2 max(1, max |s_ref|), mean <= 3e-3; every gradient tensor max <= 2e-2 max |g_ref| and
    L2 <= 1e-2 ||g_ref||, none skipped."""
    from tests.test_gpu_parity_fullsize import BAR_L2, BAR_MAX, _round_to_bf16_
    cs = _mid_case()
    m = _round_to_bf16_(_model(cs, cs['p'], 'bf16'))
    loss, out = m.loss_and_grad(cs['x'].cuda(), cs['lengths'], cs['tags'].cuda(), cs['domains'], True)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {n: t.detach().cpu().double().requires_grad_(True) for n, t in m.state_dict().items()}
    s_ref = O.scores(cs['x'].double(), cs['lengths'], cs['domains'], p, 'dense')
    l_ref = R.tagger_loss(s_ref, cs['lengths'], cs['tags'].double(), 'FocalLoss')
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
    print('switch 8x96 bf16: loss', float(loss), 'oracle', float(l_ref), 'scores max / mean |d|', float(d.max()), float(d.mean()), 'scale', scale)
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


@pytest.mark.parametrize('loss_fn', ['FocalLoss', 'CrossEntropy'])
def test_plain_mode_equals_bilstm_bitwise(loss_fn):
    """neither flag: BiLSTM's path launch for launch -- same weights, same scores, loss and every gradient, bit for bit"""
    from multimodaltopicsegmentation_amd import BiLSTM, SwitchBiLSTM
    x, lengths, tags = _small_batch()
    ref = BiLSTM(2, 64, 12, 2, loss_fn=loss_fn, compute_dtype='fp32', seed=5).cuda()
    m = SwitchBiLSTM(2, 64, 12, 2, loss_fn=loss_fn, compute_dtype='fp32', seed=9)
    m.load_state_dict(ref.state_dict())
    m = m.cuda()
    assert list(m._layout.entries.items()) == list(ref._layout.entries.items()) and torch.equal(m.flat, ref.flat)
    l0, s0 = ref.loss_and_grad(x.cuda(), lengths, tags.cuda(), True)
    l1, s1 = m.loss_and_grad(x.cuda(), lengths, tags.cuda(), [1, 0, 0, 1], True)
    assert l0.item() == l1.item() and torch.equal(s0, s1)
    assert torch.equal(m.grad_flat(), ref.grad_flat()) and float(m.grad_flat().abs().sum()) > 0
    assert m._unused_params == frozenset()
    a, ta = ref(x.cuda(), lengths)
    b, tb = m(x.cuda(), lengths, (d for d in [0, 0, 1, 1]))              # ignored, but iterated
    assert torch.equal(a, b) and ta == tb
    with pytest.raises(TypeError):
        m(x.cuda(), lengths, None)


@pytest.mark.parametrize('mode,doms', [('dense', [1, 0, 0, 1]), ('dense', [0, 0, 0, 0]), ('lstm', [1, 1, 1, 1]), ('lstm', [0, 0, 0, 0])])
def test_loss_and_grad_equals_autograd_front_end_bitwise(mode, doms):
    from multimodaltopicsegmentation_amd import SwitchBiLSTM
    x, lengths, tags = _small_batch()
    m = SwitchBiLSTM(2, 64, 12, 2, loss_fn='FocalLoss', switch_lstm_adapt=mode == 'lstm', switch_dense_adapt=mode == 'dense',
                     compute_dtype='fp32', seed=5).cuda()
    m.grad_flat().fill_(7.0)                                               # stale values: every span is overwritten, unread ones with zeros
    loss, _ = m.loss_and_grad(x.cuda(), lengths, tags.cuda(), doms, True)
    native = {n: v.clone() for n, v in m.grad_views().items()}
    unread = O.unread_params(native, doms, mode)
    assert sorted(m._unused_params) == unread and (len(unread) > 0) == (mode == 'lstm' or len(set(doms)) == 1)
    for n, v in native.items():
        assert torch.isfinite(v).all() and (v.any().item() != (n in unread)), n
    m.grad_flat().zero_()
    m.zero_grad()
    l2 = m.loss(x.cuda(), lengths, tags.cuda(), doms)
    assert l2.requires_grad and l2.item() == loss.item()
    l2.backward()
    for n, prm in m.named_parameters():
        if n in unread:
            assert prm.grad is None, n
        else:
            assert torch.equal(prm.grad, native[n]), n
    with torch.no_grad():
        assert m.loss(x.cuda(), lengths, tags.cuda(), doms).item() == loss.item()
    with pytest.raises(NotImplementedError):
        m.loss(x.cuda(), lengths, tags.cuda(), doms, segments=[])


def test_padded_input_rows_do_not_reach_the_loss_or_the_gradients():
    """rows at or past a document's length: whatever they hold, the loss, the scores and every gradient are the same bits -- also where a
    document is scored from a SHORTER one (domains [0, 1, 1, 0]: document 3, 22 sentences, reads document 1, 12), whose rows past its
    length are 0 and take no gradient"""
    from multimodaltopicsegmentation_amd import SwitchBiLSTM
    x, lengths, tags = _small_batch()
    doms = [0, 1, 1, 0]
    m = SwitchBiLSTM(2, 64, 32, 2, loss_fn='BinaryCrossEntropy', switch_dense_adapt=True, compute_dtype='fp32', seed=6).cuda()
    x0, x1 = x.clone(), x.clone()
    for b, n in enumerate(lengths.tolist()):
        x0[b, n:] = 0.0
        x1[b, n:] = 3.0 + torch.arange(x.shape[1] - n).view(-1, 1)
    l0, s0 = m.loss_and_grad(x0.cuda(), lengths, tags.cuda(), doms, True)
    l0, s0 = l0.item(), s0.clone()
    g0 = {n: v.clone() for n, v in m.grad_views().items()}
    l1, s1 = m.loss_and_grad(x1.cuda(), lengths, tags.cuda(), doms, True)
    assert l1.item() == l0 and torch.equal(s1, s0)
    for n, v in m.grad_views().items():
        assert torch.equal(v, g0[n]), n
    assert float(g0['model.rnn.weight_ih_l0'].abs().max()) > 0 and float(g0['classification_2.weight'].abs().max()) > 0
    bias = m.state_dict()['classification_2.bias'].item()                  # document 3 past its source's 12 sentences: the bias
    assert (s0[3, 12:, 0] == bias).all()


def test_lstm_mode_mixed_batch_raises_as_upstream():
    from multimodaltopicsegmentation_amd import SwitchBiLSTM
    g = load('g20_switch_bilstm')
    x, lengths, tags = _small_batch()
    m = SwitchBiLSTM(2, 64, 12, 1, loss_fn='FocalLoss', switch_lstm_adapt=True, compute_dtype='fp32', seed=2).cuda()
    for call in (lambda: m.loss(x.cuda(), lengths, tags.cuda(), [1, 0, 1, 1]), lambda: m(x.cuda(), lengths, [1, 0, 1, 1]),
                 lambda: m.loss_and_grad(x.cuda(), lengths, tags.cuda(), [0, 0, 0, 1])):
        with pytest.raises(AttributeError) as e:
            call()
        assert type(e.value).__name__ == str(g['lstm_mixed_loss_type']) and str(e.value) == str(g['lstm_mixed_loss_msg'])


@pytest.mark.parametrize('switch', ['dense', 'lstm'])
def test_text_segmenter_steps(switch):
    from multimodaltopicsegmentation_amd import AudioPortionDataset, SwitchBiLSTM, TextSegmenter
    torch.manual_seed(11)
    ts = TextSegmenter(2, 64, 32, num_layers=2, architecture='SwitchBiLSTM', switch=switch, loss_fn='FocalLoss', threshold=0.45,
                       compute_dtype='fp32').cuda()
    assert isinstance(ts.model, SwitchBiLSTM) and ts.domain
    x, lengths, tags = _small_batch()
    doms = [1, 0, 0, 1] if switch == 'dense' else [0, 0, 0, 0]
    # a collated batch: the dataset's own collater with domain_adapt (a file name that starts with a digit is domain 1)
    lines = [(x[i, :n], tags[i, :n].tolist(), f'{7 if doms[i] else "a"}_doc{i}') for i, n in enumerate(lengths.tolist())]
    ds = AudioPortionDataset(lines, {}, CRF=False, truncate=False, domain_adapt=True)
    batch = ds.collater([ds[i] for i in range(len(lines))])
    assert torch.equal(batch['tgt_tokens'], tags) and batch['src_lengths'].tolist() == lengths.tolist()      # src_tokens: x, zero past each length
    assert batch['domain'] == doms
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) and k != 'src_lengths' else v) for k, v in batch.items()}
    loss = ts.training_step(batch, 0)
    assert loss.requires_grad and np.isfinite(loss.item())
    loss.backward()
    unread = set(O.unread_params(dict(ts.model.named_parameters()), doms, switch))
    for n, p in ts.model.named_parameters():
        assert (p.grad is None) == (n in unread), n
        assert p.grad is None or torch.isfinite(p.grad).all()
    val = ts.validation_step(batch, 0)
    want, _ = ts.model.loss_and_grad(batch['src_tokens'], batch['src_lengths'], batch['tgt_tokens'], doms, False)
    assert val.item() == want.item()
    res = ts.test_step(batch, 0)
    assert ts.model.th == 0.45 and all(np.isfinite(float(v)) for v in res.values())
    pred = ts.predict_step(batch, 0)                                       # served when the batch carries 'domain' (upstream: TypeError)
    sc, lists = ts.model(batch['src_tokens'], batch['src_lengths'], doms)
    assert pred == lists and [len(t) for t in pred] == lengths.tolist()
    with pytest.raises(TypeError):
        ts.predict_step({k: v for k, v in batch.items() if k != 'domain'}, 0)


def test_native_trainer_plain_mode_steps_like_bilstm():
    from multimodaltopicsegmentation_amd import BiLSTM, SwitchBiLSTM
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    x, lengths, tags = _small_batch()
    ref = BiLSTM(2, 64, 32, 2, loss_fn='FocalLoss', compute_dtype='bf16', seed=5).cuda()
    m = SwitchBiLSTM(2, 64, 32, 2, loss_fn='FocalLoss', compute_dtype='bf16', seed=5).cuda()
    assert torch.equal(m.flat, ref.flat)
    ta, tb = NativeTrainer(ref, lr=1e-3, optimizer='Adam'), NativeTrainer(m, lr=1e-3, optimizer='Adam')
    batch = {'src_tokens': x.cuda(), 'src_lengths': lengths, 'tgt_tokens': tags.cuda(), 'domain': [1, 0, 0, 1]}
    for _ in range(2):
        la, lb = ta.step(batch), tb.step(batch)
        assert la.item() == lb.item()
    torch.cuda.synchronize()
    assert torch.equal(m.flat, ref.flat) and torch.equal(m._wcopy, ref._wcopy)


def test_native_trainer_first_adam_step_leaves_the_unread_head_alone():
    from multimodaltopicsegmentation_amd import SwitchBiLSTM
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    x, lengths, tags = _small_batch()
    m = SwitchBiLSTM(2, 64, 32, 2, loss_fn='FocalLoss', switch_dense_adapt=True, compute_dtype='fp32', seed=5).cuda()
    before = {n: t.clone() for n, t in m.state_dict().items()}
    tr = NativeTrainer(m, lr=1e-2, optimizer='Adam')
    loss = tr.step({'src_tokens': x.cuda(), 'src_lengths': lengths, 'tgt_tokens': tags.cuda(), 'domain': [1, 1, 1, 1]})
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
    after = m.state_dict()
    for n in before:
        same = torch.equal(after[n], before[n])
        assert same == n.startswith('classification_2.'), n
