"""GPU tests of the gated late-fusion merge: mts_gate_merge_fwd / _bwd against fp64 on their own operands, BiLSTMLateFusion(merge='gate')
against the fp64 oracle (tests/gated_fusion_oracle.py), the two front ends, the gradient-ready spans, TextSegmenter(fusion_merge='gate'),
and the trainer, the fit loop and the data-parallel step around it."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import gated_fusion_oracle as O
from tests.test_gpu_recurrent_longt5 import _check

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD_ROWS, GUARD_COLS = 7, 8
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}
# (rows, W, column offset of the views): one vector row; an odd W / 16; rows that are no multiple of the block's; W = 528 (no power of two:
# a partial last column block) on a base 4 elements into the buffer, which is 8-byte aligned in bf16: the 4-element path; the bench width
KERNEL_CASES = [(1, 16, 0), (2, 48, 0), (115, 64, 0), (771, 528, 4), (16384, 512, 0)]
PLANTED = (30.0, -30.0, 88.0, -88.0, 1e4, -1e4)


def _planted_positions(n):
    return [(i * n) // 6 + (i % 2) for i in range(6)]


def _buffer(rows, W, dt, fill=None, gen=None, scale=1.0):
    """a [rows + 7, W + 8] buffer: random where an input, 7.0 where an output"""
    if fill is None:
        return (torch.randn(rows + GUARD_ROWS, W + GUARD_COLS, generator=gen) * scale).to(dt).to(DEV)
    return torch.full((rows + GUARD_ROWS, W + GUARD_COLS), fill, dtype=dt, device=DEV)


def _guards_intact(buf, rows, W, off):
    b = buf.float().clone()
    b[:rows, off:off + W] = 7.0
    return bool((b == 7.0).all())


@functools.lru_cache(maxsize=2)
def _kernel_reference(rows, W, dtype):
    """the inputs of a case (on the host, as the kernels will read them) and the fp64 results -- computed once, shared, never changed"""
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(rows * 1000 + W)
    a = (torch.randn(rows, W, generator=g) * 2.0)
    pos = _planted_positions(rows * W)
    a.view(-1)[pos] = torch.tensor(PLANTED)
    a = a.to(dt)
    h1, h2, dm = ((torch.randn(rows, W, generator=g) * s).to(dt) for s in (0.5, 0.5, 1.0))
    a64, p, q, d = a.double(), h1.double(), h2.double(), dm.double()
    z = torch.sigmoid(a64)
    ref = dict(m=z * p + (1 - z) * q, da=d * (p - q) * z * (1 - z), dh1=d * z, dh2=d * (1 - z))
    return dict(a=a, h1=h1, h2=h2, dm=dm), ref, pos


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', KERNEL_CASES, ids=[f'{c[0]}x{c[1]}' for c in KERNEL_CASES])
def test_gate_merge_kernels_against_fp64(case, dtype):
    from multimodaltopicsegmentation_amd import ops
    rows, W, off = case
    dt = DTYPES[dtype]
    host, ref, pos = _kernel_reference(rows, W, dtype)
    bufs, views = {}, {}
    for k, t in host.items():
        bufs[k] = _buffer(rows, W, dt, fill=7.0)
        views[k] = bufs[k][:rows, off:off + W]
        views[k].copy_(t)
    keep = {k: b.clone() for k, b in bufs.items()}
    if off:
        assert views['a'].data_ptr() % 16 == (8 if dt == torch.bfloat16 else 0)          # bf16: no 16-byte vectors from this base
    runs = []
    for _ in range(2):
        out = {k: _buffer(rows, W, dt, fill=7.0) for k in ('m', 'da', 'dh1', 'dh2')}
        ov = {k: b[:rows, off:off + W] for k, b in out.items()}
        ops.gate_merge_fwd(views['a'], views['h1'], views['h2'], ov['m'])
        ops.gate_merge_bwd(views['a'], views['h1'], views['h2'], views['dm'], ov['da'], ov['dh1'], ov['dh2'])
        runs.append((out, ov))
    torch.cuda.synchronize()
    out, ov = runs[0]
    for k in bufs:
        assert torch.equal(bufs[k], keep[k]), f'input {k} was modified'
    for k in out:
        assert _guards_intact(out[k], rows, W, off), f'{k}: written outside [0:rows, 0:W]'
        assert torch.equal(out[k], runs[1][0][k]), f'{k}: differs between two identical calls'
        assert torch.isfinite(ov[k].float()).all(), f'{k}: not finite'
        _check(ov[k], ref[k], dt, f'{k} {rows}x{W} {dtype}')
    # |a| = 1e4: the gate is saturated -- z is exactly 1 | 0, m is h1 | h2 bit for bit, da an exact 0, and dh1 | dh2 is dm | 0 bit for bit
    flat = {k: v.reshape(-1) for k, v in {**views, **ov}.items()}
    hi, lo = pos[4], pos[5]
    assert float(flat['a'][hi]) > 9e3 and float(flat['a'][lo]) < -9e3
    assert torch.equal(flat['m'][hi], flat['h1'][hi]) and torch.equal(flat['m'][lo], flat['h2'][lo])
    assert float(flat['da'][hi]) == 0.0 and float(flat['da'][lo]) == 0.0
    assert torch.equal(flat['dh1'][hi], flat['dm'][hi]) and float(flat['dh2'][hi]) == 0.0
    assert torch.equal(flat['dh2'][lo], flat['dm'][lo]) and float(flat['dh1'][lo]) == 0.0


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_weight_gradient_into_a_column_half_at_split_k_depth(dtype):
    """dW_g is two TN mts_gemm calls into the column halves of the gradient view (ldc = 4H).  At the training shapes K = all sentences, where
    mts_gemm splits K: the strided fp32 C must come out of the split path too.  K = 4096 (above both split thresholds), W = 512; the bound
    is tests/gemm_epilogue_oracle.py's derived one; the other half keeps its 7.0."""
    from multimodaltopicsegmentation_amd import ops
    from tests import gemm_epilogue_oracle as G
    K, W = 4096, 512
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(5)
    da, h = (torch.randn(K, W, generator=g) * 0.2).to(dt), (torch.randn(K, W, generator=g) * 0.5).to(dt)
    ref, S = G.product('TN', da, h)
    for half in (0, 1):
        dw = torch.full((W, 2 * W), 7.0, device=DEV)
        ops.linear_wgrad(da.to(DEV), h.to(DEV), dw[:, half * W:(half + 1) * W])
        torch.cuda.synchronize()
        got = dw.cpu().double()
        assert bool((got[:, (1 - half) * W:(2 - half) * W] == 7.0).all())
        err = (got[:, half * W:(half + 1) * W] - ref).abs()
        lim = G.bound(S, K, ref)
        print(f'wgrad half {half} {dtype}: largest err / bound {float((err / lim).max()):.4f}')
        assert bool((err <= lim).all())


# ------------------------------------------------------------------------------------------------ model level
def _model(cs, dtype, loss_fn='FocalLoss', **kw):
    from multimodaltopicsegmentation_amd import BiLSTMLateFusion
    m = BiLSTMLateFusion(2, list(cs['D']), cs['H'], cs['NL'], loss_fn=loss_fn, compute_dtype=dtype, seed=0, merge='gate', **kw)
    m.load_state_dict({n: t.float() for n, t in cs['p'].items()})
    return m.cuda().eval()


def _oracle(cs, p_src, loss_fn, segments=None, tags=None):
    """-> (loss, scores, z, {name: gradient}) in fp64; p_src: name -> tensor in the reference's shapes"""
    p = {n: t.detach().cpu().double().requires_grad_(True) for n, t in p_src.items()}
    tags = cs['tags'] if tags is None else tags
    loss, s, z = O.loss(cs['x1'].double(), cs['x2'].double(), cs['lengths'], tags.double(), p, loss_fn, segments=segments)
    loss.backward()
    return loss.detach(), s.detach(), z.detach(), {n: t.grad for n, t in p.items()}


def _compare_small(m, cs, loss, out, ref, what):
    """test_gpu_taggers.py::test_late_fusion_small's fp32 bars: scores atol 1e-5 on every row, gradients rtol 2e-3 / atol 2e-6"""
    l_ref, s_ref, z, g_ref = ref
    frac = O.decided_fraction(z, cs['lengths'].tolist())
    print(f'{what}: loss {float(loss):.8f} oracle {float(l_ref):.8f}; {frac:.3f} of the valid gates outside [0.25, 0.75]')
    assert frac >= 0.2                                                      # the gate matters: a merge that ignored it could not pass
    assert abs(float(loss) - float(l_ref)) < 2e-6 * max(1.0, abs(float(l_ref)))
    got = out.detach().cpu().double()
    assert got.shape == s_ref.shape
    err = float((got - s_ref).abs().max())
    print(f'{what}: scores max err {err:.3e}')
    assert err <= 1e-5
    views = m.grad_views()
    assert set(views) == set(g_ref)
    for n, gv in views.items():
        a, r = m.logical_view(views, n).detach().cpu().double(), g_ref[n]
        assert a.shape == r.shape, n
        d = (a - r).abs()
        assert bool((d <= 2e-6 + 2e-3 * r.abs()).all()), (what, n, float(d.max()), float(r.abs().max()))
    for n in ('gate.weight', 'gate.bias', 'model1.rnn.weight_ih_l0', 'model2.rnn.weight_hh_l1_reverse'):
        assert float(g_ref[n].abs().max()) > 1e-6, n


def _bias_at_padded_rows(m, cs, out):
    bias = m.state_dict()['classification.bias'].to(out.device)
    for b, n in enumerate(cs['lengths'].tolist()):
        assert (out[b, n:] == bias).all(), b                                # rows at or past the length: m = 0 exactly, the score is the bias


@pytest.mark.parametrize('loss_fn', ['FocalLoss', 'BinaryCrossEntropy', 'CrossEntropy'])
def test_small_fp32_against_the_oracle(loss_fn):
    cs = O.small_case(32, n_out=2 if loss_fn == 'CrossEntropy' else 1)
    m = _model(cs, 'fp32', loss_fn)
    loss, out = m.loss_and_grad(cs['x1'].cuda(), cs['x2'].cuda(), cs['lengths'], cs['tags'].cuda(), True)
    torch.cuda.synchronize()
    _compare_small(m, cs, loss, out, _oracle(cs, m.state_dict(), loss_fn), f'gate H=32 {loss_fn}')
    _bias_at_padded_rows(m, cs, out)
    assert out.shape[1] == 30                                               # max(lengths) of an input of 33 rows


def _pad_mask(m):
    """True at the pad entries of the flat vectors (padded units; alignment gaps are not parameters)"""
    from multimodaltopicsegmentation_amd.flat import pad_blocks
    mask = torch.zeros(m._layout.numel, dtype=torch.bool)
    sd = m.state_dict()
    for name, spec in m._layout.pads.items():
        real = pad_blocks(torch.ones(tuple(sd[name].shape)), spec)
        m._layout.view(mask, name).copy_(real == 0)
    return mask


def test_padded_hidden_size_and_inert_pads():
    """H = 25 (stored as 32): the same comparison, and after one NativeTrainer Adam step every pad entry of the parameters and of the
    gradient is exactly 0 -- the padded units are inert through the gate, shown and not assumed."""
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    cs = O.small_case(25)
    m = _model(cs, 'fp32')
    loss, out = m.loss_and_grad(cs['x1'].cuda(), cs['x2'].cuda(), cs['lengths'], cs['tags'].cuda(), True)
    torch.cuda.synchronize()
    _compare_small(m, cs, loss, out, _oracle(cs, m.state_dict(), 'FocalLoss'), 'gate H=25')
    _bias_at_padded_rows(m, cs, out)
    pad = _pad_mask(m).to(DEV)
    assert int(pad.sum()) > 64 * 128 - 50 * 100 and not m.flat[pad].any() and not m.grad_flat()[pad].any()
    before = m.flat.clone()
    tr = NativeTrainer(m, lr=1e-2, optimizer='Adam')
    tr.step({'src_tokens': cs['x1'].cuda(), 'src_tokens2': cs['x2'].cuda(), 'src_lengths': cs['lengths'], 'tgt_tokens': cs['tags'].cuda()})
    torch.cuda.synchronize()
    assert not m.flat[pad].any() and not m.grad_flat()[pad].any()
    moved = (m.flat - before).abs()
    for n in ('gate.weight', 'gate.bias', 'classification.weight'):
        assert float(m._layout.view(moved, n).max()) > 1e-3, n               # ... while the real entries took the step


def test_mid_size_bf16_against_the_oracle():
    """test_gpu_parity_fullsize.py's protocol and bars, as test_gpu_switch.py::test_mid_size_bf16_against_oracle applies them: bf16-exact
    master weights and inputs on both sides; loss 2e-3 relative; scores of every row (padded ones included) max <= 3e-2 max(1, max |s_ref|),
    mean <= 3e-3; every gradient tensor max <= 2e-2 max |g_ref| and L2 <= 1e-2 ||g_ref||, none skipped."""
    from tests.test_gpu_parity_fullsize import BAR_L2, BAR_MAX, _round_to_bf16_
    cs = O.mid_case()
    m = _round_to_bf16_(_model(cs, 'bf16'))
    loss, out = m.loss_and_grad(cs['x1'].cuda(), cs['x2'].cuda(), cs['lengths'], cs['tags'].cuda(), True)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    l_ref, s_ref, z, g_ref = _oracle(cs, m.state_dict(), 'FocalLoss')
    d = (out.detach().cpu().double().view_as(s_ref) - s_ref).abs()
    scale = max(1.0, float(s_ref.abs().max()))
    views = m.grad_views()
    assert set(views) == set(g_ref)
    worst = {}
    for name, gv in views.items():
        a, r = gv.detach().cpu().double(), g_ref[name]
        worst[name] = (float((a - r).abs().max()) / float(r.abs().max()), float((a - r).norm()) / float(r.norm()))
    print('gate 8x96 bf16: loss', float(loss), 'oracle', float(l_ref), 'scores max / mean |d|', float(d.max()), float(d.mean()), 'scale', scale,
          'decided gates', O.decided_fraction(z, cs['lengths'].tolist()))
    for name, w in worst.items():
        print(f'  {name}: max-ratio {w[0]:.3e} l2-ratio {w[1]:.3e}')
    assert abs(float(loss) - float(l_ref)) <= 2e-3 * abs(float(l_ref)), (float(loss), float(l_ref))
    assert float(d.max()) <= 3e-2 * scale and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    for name, (rmax, rl2) in worst.items():
        assert rmax <= BAR_MAX and rl2 <= BAR_L2, (name, rmax, rl2)


def test_bf16_wire_inputs_and_serial_encoders_give_the_same_bits():
    """What sits in front of the merge keeps working: inputs that arrive in bf16 (DevicePrefetcher / ResidentCorpus wire_dtype='bf16') give the
    bits of the bf16-exact fp32 inputs, and the two encoders on one stream (concurrent_encoders = False) the bits of the two-stream overlap."""
    cs = O.mid_case()
    m = _model(cs, 'bf16')
    x1, x2, lengths, tags = cs['x1'].cuda(), cs['x2'].cuda(), cs['lengths'], cs['tags'].cuda()
    assert m.concurrent_encoders
    loss, out = m.loss_and_grad(x1, x2, lengths, tags, True)
    l0, s0, g0 = loss.item(), out.clone(), m.grad_flat().clone()
    loss, out = m.loss_and_grad(x1.to(torch.bfloat16), x2.to(torch.bfloat16), lengths, tags, True)
    assert loss.item() == l0 and torch.equal(out, s0) and torch.equal(m.grad_flat(), g0)
    m.concurrent_encoders = False
    loss, out = m.loss_and_grad(x1, x2, lengths, tags, True)
    assert loss.item() == l0 and torch.equal(out, s0) and torch.equal(m.grad_flat(), g0)
    assert np.isfinite(l0) and float(g0.abs().max()) > 0


@pytest.mark.parametrize('kw', [dict(), dict(dropout_in=0.2, dropout_out=0.3)], ids=['plain', 'dropout'])
def test_front_ends_agree_bitwise_and_padded_input_rows_reach_nothing(kw):
    """loss_and_grad and the autograd front end (loss() under grad mode) give the same bits; want_grad=False and loss() under no_grad give the
    same loss; garbage in the input rows at or past each length changes no bit of the loss, the valid scores or the gradients."""
    cs = O.small_case(32)
    m = _model(cs, 'fp32', **kw)
    x1, x2, lengths, tags = cs['x1'].cuda(), cs['x2'].cuda(), cs['lengths'], cs['tags'].cuda()

    def native(a, b):
        torch.manual_seed(3)
        m._drop_calls = 0                                                    # the same dropout masks in every run
        m.grad_flat().fill_(7.0)                                             # stale values: every span is overwritten
        loss, out = m.loss_and_grad(a, b, lengths, tags, True)
        return loss.item(), out.clone(), {n: v.clone() for n, v in m.grad_views().items()}

    l0, s0, g0 = native(x1, x2)
    assert all(torch.isfinite(v).all() and v.any() for v in g0.values())
    torch.manual_seed(3)
    m._drop_calls = 0
    m.zero_grad()
    l1 = m.loss(x1, x2, lengths, tags)
    assert l1.requires_grad and l1.item() == l0
    l1.backward()
    for n, prm in m.named_parameters():
        assert torch.equal(prm.grad, g0[n]), n
    torch.manual_seed(3)
    m._drop_calls = 0
    assert m.loss_and_grad(x1, x2, lengths, tags, False)[0].item() == l0
    torch.manual_seed(3)
    m._drop_calls = 0
    with torch.no_grad():
        assert m.loss(x1, x2, lengths, tags).item() == l0
    y1, y2 = x1.clone(), x2.clone()
    for b, n in enumerate(lengths.tolist()):
        y1[b, n:] = 3.0 + torch.arange(x1.shape[1] - n, device=DEV).view(-1, 1)
        y2[b, n:] = -5.0
    l2, s2, g2 = native(y1, y2)
    assert l2 == l0
    for b, n in enumerate(lengths.tolist()):
        assert torch.equal(s2[b, :n], s0[b, :n]), b
    for n in g0:
        assert torch.equal(g2[n], g0[n]), n


def test_segments_with_the_gate_against_the_oracle():
    """`segments=`: 0.1 x the cosine loss over m (width 2H) + the unmasked main loss; loss and gradients against the oracle, fp32."""
    cs = O.small_case(32)
    m = _model(cs, 'fp32')
    tags = cs['tags'][:, :30]                                               # the segments branch wants targets of exactly max(lengths) positions
    loss, out = m.loss_and_grad(cs['x1'].cuda(), cs['x2'].cuda(), cs['lengths'], tags.cuda(), True, segments=cs['segments'])
    torch.cuda.synchronize()
    ref = _oracle(cs, m.state_dict(), 'FocalLoss', segments=cs['segments'], tags=tags)
    plain = _oracle(cs, m.state_dict(), 'FocalLoss')
    assert abs(float(ref[0]) - float(plain[0])) > 1e-3                      # the auxiliary term is there
    _compare_small(m, cs, loss, out, ref, 'gate H=32 segments')
    l2 = m.loss(cs['x1'].cuda(), cs['x2'].cuda(), cs['lengths'], tags.cuda(), segments=cs['segments'])
    assert l2.item() == loss.item()


def test_gradient_ready_spans_cover_every_parameter_once():
    """tests/test_gpu_hooks.py for the gate: every span handed to the hook holds its final value, every parameter entry of the flat gradient
    lies in exactly one span, no entry in two, and what no span covers (the alignment gaps between parameter groups) is zero.  The gate's
    and the head's spans are announced before any encoder span."""
    cs = O.small_case(32)
    m = _model(cs, 'fp32')
    assert m.grad_hooks_cover_all
    seen = []
    m._grad_hook = lambda a, b: seen.append((a, b, m.grad_flat()[a:b].clone()))
    m.loss_and_grad(cs['x1'].cuda(), cs['x2'].cuda(), cs['lengths'], cs['tags'].cuda(), True)
    m._grad_hook = None
    torch.cuda.synchronize()
    final = m.grad_flat().clone()
    covered = torch.zeros(final.numel(), dtype=torch.int32)
    for a, b, snap in seen:
        assert torch.equal(snap, final[a:b]), (a, b)
        covered[a:b] += 1
    assert int(covered.max()) == 1
    is_param = torch.zeros(final.numel(), dtype=torch.bool)
    for name, (off, shape) in m._layout.entries.items():
        is_param[off:off + int(np.prod(shape))] = True
    assert bool((covered[is_param] == 1).all())
    assert torch.count_nonzero(final.cpu()[covered == 0]) == 0
    lay = m._layout
    head = (lay.entries['classification.weight'][0], sum(lay.span('classification.bias', 'classification.bias')))
    gate = (lay.entries['gate.weight'][0], sum(lay.span('gate.bias', 'gate.bias')))
    assert [(a, b) for a, b, _ in seen[:2]] == [head, gate]
    assert all(float(snap.abs().max()) > 0 for _, _, snap in seen)


def test_text_segmenter_steps_and_checkpoint(tmp_path):
    from multimodaltopicsegmentation_amd import BiLSTMLateFusion, TextSegmenter
    torch.manual_seed(11)
    kw = dict(tagset_size=2, embedding_dim=[40, 24], hidden_dim=25, num_layers=2, architecture='BiLSTMLateFusion', loss_fn='FocalLoss',
              threshold=0.45, compute_dtype='fp32')
    ts = TextSegmenter(fusion_merge='gate', **kw).cuda()
    concat = TextSegmenter(**kw)
    assert isinstance(ts.model, BiLSTMLateFusion) and ts.double_input and ts.model.merge == 'gate'
    assert set(ts.state_dict()) == set(concat.state_dict()) | {'model.gate.weight', 'model.gate.bias'}
    cs = O.small_case(25)
    batch = {'src_tokens': cs['x1'].cuda(), 'src_tokens2': cs['x2'].cuda(), 'src_lengths': cs['lengths'], 'tgt_tokens': cs['tags'].cuda()}
    loss = ts.training_step(batch, 0)
    assert loss.requires_grad and np.isfinite(loss.item())
    loss.backward()
    for n, p in ts.model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.any(), n
    val = ts.validation_step(batch, 0)
    want, _ = ts.model.loss_and_grad(batch['src_tokens'], batch['src_tokens2'], batch['src_lengths'], batch['tgt_tokens'], False)
    assert val.item() == want.item()
    res = ts.test_step(batch, 0)
    assert ts.model.th == 0.45 and all(np.isfinite(float(v)) for v in res.values())
    pred = ts.predict_step(batch, 0)
    scores, lists = ts.model(batch['src_tokens'], batch['src_tokens2'], batch['src_lengths'])
    assert pred == lists and [len(t) for t in pred] == cs['lengths'].tolist()
    path = tmp_path / 'gate.ckpt'
    torch.save({'state_dict': {k: v.cpu() for k, v in ts.state_dict().items()}}, path)
    back =TextSegmenter.load_from_checkpoint(str(path), fusion_merge='gate', **kw).cuda()
    for (ka, va), (kb, vb) in zip(ts.state_dict().items(), back.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    back.model.th = 0.45
    scores2, lists2 = back.model(batch['src_tokens'], batch['src_tokens2'], batch['src_lengths'])
    assert torch.equal(scores2, scores) and lists2 == lists


def _batch_of(cs):
    return {'src_tokens': cs['x1'].cuda(), 'src_tokens2': cs['x2'].cuda(), 'src_lengths': cs['lengths'], 'tgt_tokens': cs['tags'].cuda()}


def test_native_trainer_three_steps():
    """NativeTrainer.step x 3 (fused Adam on the flat buffers, bf16 mirror written by the optimizer): every tensor moves, the mirror is the
    master rounded once, and in fp32 the result is that of the autograd front end under torch.optim.Adam(eps=1e-7) -- identical gradients
    (test_front_ends_agree_bitwise...), so only the two Adam implementations differ: test_gpu_dp_step.py's absolute criterion, 2e-5 max and
    1e-7 mean at lr = 1e-3."""
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    cs = O.small_case(32)
    batch = _batch_of(cs)
    m = _model(cs, 'bf16')
    before = {n: t.clone() for n, t in m.state_dict().items()}
    tr = NativeTrainer(m, lr=1e-3, optimizer='Adam')
    losses = [tr.step(batch).item() for _ in range(3)]
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in losses) and len(set(losses)) == 3
    for n, t in m.state_dict().items():
        assert not torch.equal(t, before[n]) and torch.isfinite(t).all(), n
    assert torch.equal(m._wcopy, m.flat.to(torch.bfloat16))

    a, b = _model(cs, 'fp32'), _model(cs, 'fp32')
    tr = NativeTrainer(a, lr=1e-3, optimizer='Adam')
    opt = torch.optim.Adam(b.parameters(), lr=1e-3, eps=1e-7)
    for _ in range(3):
        la = tr.step(batch)
        opt.zero_grad()
        lb = b.loss(batch['src_tokens'], batch['src_tokens2'], batch['src_lengths'], batch['tgt_tokens'])
        lb.backward()
        opt.step()
        assert abs(la.item() - lb.item()) <= 1e-5 * max(1.0, abs(lb.item()))
    torch.cuda.synchronize()
    diff = (a.flat - b.flat).abs()
    print('gate trainer vs torch Adam: max', float(diff.max()), 'mean', float(diff.mean()))
    assert float(diff.max()) <= 2e-5 and float(diff.mean()) <= 1e-7


def _build_gate():
    from multimodaltopicsegmentation_amd import BiLSTMLateFusion
    return BiLSTMLateFusion(2, [40, 24], 32, num_layers=2, loss_fn='FocalLoss', compute_dtype='fp32', seed=11, merge='gate').to(DEV)


def test_fit_on_a_resident_corpus_is_the_hand_written_loop():
    """fit for 2 epochs on a small ResidentCorpus with a second input, validation with the device threshold sweep in between: the
    parameters are those of the hand-written loop (sampler + corpus.batch + trainer.step), bit for bit -- ResidentCorpus, fit and
    ThresholdSweep dispatch on the second input, not on the merge."""
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    from tests.test_gpu_fit import BATCH, SEED, TRAIN_LENGTHS, VAL_LENGTHS, _corpus
    train, val = _corpus('latefusion', TRAIN_LENGTHS, 2), _corpus('latefusion', VAL_LENGTHS, 4)
    want = _build_gate()
    tr = NativeTrainer(want, lr=1e-3)
    sampler = train.sampler(BATCH, rank=0, world=1, shuffle=True, seed=SEED)
    means = []
    for epoch in range(2):
        sampler.set_epoch(epoch)
        losses = [tr.step(train.batch(*item)) for item in sampler]
        means.append(float(torch.stack([v.detach() for v in losses]).to(torch.float64).sum()) / len(losses))
    model = _build_gate()
    init = model.flat.detach().clone()
    out = NativeTrainer(model, lr=1e-3).fit(train, val, batch_size=BATCH, max_epochs=2, seed=SEED, search_threshold=True, metric='Pk',
                                            restore_best=False)
    torch.cuda.synchronize()
    assert torch.equal(model.flat, want.flat) and float((model.flat - init).abs().max()) > 1e-3
    assert [r['train_loss'] for r in out['epochs']] == means
    assert all(r['threshold'] is not None for r in out['epochs']) and out['threshold'] is not None


def _dp_run(rank, world):
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer, shard_batch
    from tests.test_gpu_dp_step import _batches, _to_dev
    model = _build_gate()
    tr = NativeTrainer(model, lr=1e-3, optimizer='Adam')
    losses = [float(tr.step(_to_dev(shard_batch(batch, rank, world)))) for batch in _batches('latefusion', False)]
    torch.cuda.synchronize()
    return model.flat.detach().cpu().clone(), losses, tr


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), MTS_DP_SCHEDULE='allreduce')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    flat, losses, tr = _dp_run(rank, world)
    assert tr.world == world
    # the overlapped path ran: hooks installed (grad_hooks_cover_all), nothing left pending
    assert getattr(tr.model, 'grad_hooks_cover_all', False) and tr._pending == [] and tr.model._grad_hook is not None
    torch.save({'flat': flat, 'losses': losses}, os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_native_step_equals_the_single_process_step(tmp_path):
    """tests/test_gpu_dp_step.py's late-fusion case with the gate, under that file's criterion: two gloo ranks on one GPU, each on its
    shard, hold identical parameters after two steps, equal to the one-process run on the global batch within 2e-5 max / 1e-7 mean."""
    import torch.multiprocessing as mp
    from tests.test_gpu_dp_step import _batches, _free_port
    world = 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(os.path.join(tmp_path, 'r0.pt'))
    r1 = torch.load(os.path.join(tmp_path, 'r1.pt'))
    assert torch.equal(r0['flat'], r1['flat'])
    single, losses, _ = _dp_run(0, 1)
    init = _build_gate().flat.detach().cpu().clone()
    assert float((single - init).abs().max()) > 1e-3
    diff = (r0['flat'] - single).abs()
    assert float(diff.max()) <= 2e-5, (float(diff.max()), int(diff.argmax()))
    assert float(diff.mean()) <= 1e-7, float(diff.mean())
    assert abs(0.5 * r0['losses'][0] + 0.5 * r1['losses'][0] - losses[0]) <= 2e-6 * max(1.0, abs(losses[0]))
    assert len(_batches('latefusion', False)) == 2
