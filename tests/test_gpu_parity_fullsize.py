"""Parity AT THE BENCHMARKED SIZES: every BASELINE.json per-GPU shape goes through the code path
bench.py / NativeTrainer run -- `loss_and_grad` in bf16 with the default planner -- and is compared with the CPU oracle on the SAME
numbers:

  * the model's fp32 master weights and the inputs are first rounded to bf16-representable values, so the product's bf16 GEMM
    operands and the oracle's operands are identical; what is left between the two is the product's bf16 storage of activations and
    its accumulation order -- not the 2^-9 operand rounding that forced the 0.1-0.12 bars of the earlier model-level tests;
  * the oracle runs in fp64 (fp32 for the 64 x 512 late-fusion case, whose 2 x 2 x 2 x 512 dependent steps take minutes in fp64; an
    fp32 evaluation is within ~1e-5 of the fp64 one, three orders below the bars);
  * bars: per tensor, max |g - g_ref| <= BAR_MAX * max |g_ref| and ||g - g_ref|| <= BAR_L2 * ||g_ref|| -- no tensor skipped.  A
    wrong scale on any tensor (x2, x0.5, a missing 1/sqrt(hd)) moves the L2 ratio to >= 0.5.

Decode (round 4): at every shape the greedy boundary lists (th 0.4 and 0.5; Viterbi paths for the CRF head) are compared with the oracle's.  In bf16 a
sentence may differ only where the oracle's probability lies within DECODE_MARGIN of the threshold -- the 3e-2 score bar times the largest slope
of the sigmoid (1/4), rounded up; in fp32 parity mode (the drop-in classes' default, north_star's "bit-exact boundary indices under greedy
decode") the lists of the 64 x 256 x 1792 transformer and BiLSTM must be IDENTICAL.  Ragged batches (len ~ U{L/4..L}, the packed path for the
transformer -- asserted from the shape of the scores it returns) run at full size too.

Shapes: configs[1]/[3] 64 x 256 x 1792 restricted-window transformer (16 384 rows: 256x224 GEMM tile, fused feed-forward block,
split-K weight gradients -- asserted from the launches that actually ran); configs[2] 64 x 256 x 1792 BiLSTM 2 x 256 with the focal
head and with the CRF head; configs[4] 64 x 512 late fusion 1024 + 768.  Reference: models/CRF.py:574-595, :319-356, :130-146, :420-461.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

BAR_MAX, BAR_L2 = 2e-2, 1e-2


def _round_to_bf16_(model):
    with torch.no_grad():
        model.flat.copy_(model.flat.to(torch.bfloat16).to(torch.float32))
    return model


def _bf16_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _oracle_params(model, dtype):
    return {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in model.state_dict().items()}


def _compare_grads(model, p, exact_zero=()):
    """every parameter tensor of the model against the oracle's autograd gradient"""
    views = model.grad_views()
    assert set(views) == set(p), set(views) ^ set(p)
    worst = {}
    for name, gv in views.items():
        a = gv.detach().cpu().double()
        r = p[name].grad
        r = torch.zeros_like(a) if r is None else r.double()
        rmax, rl2 = float(r.abs().max()), float(r.norm())
        if name in exact_zero:
            # the exact gradient is 0 (see the caller): the oracle's own value is rounding noise, the bar is absolute, on the scale
            # of the sibling tensor named by the caller
            sib = p[exact_zero[name]].grad.double()
            assert rmax <= 1e-9 * float(sib.abs().max()), (name, rmax)
            assert float(a.abs().max()) <= BAR_MAX * float(sib.abs().max()), (name, float(a.abs().max()), float(sib.abs().max()))
            continue
        assert rmax > 0, name
        dmax, dl2 = float((a - r).abs().max()), float((a - r).norm())
        worst[name] = (dmax / rmax, dl2 / rl2)
        assert dmax <= BAR_MAX * rmax, (name, dmax, rmax)
        assert dl2 <= BAR_L2 * rl2, (name, dl2, rl2)
    return worst


def _full_batch(B, L, D, seed, D2=None):
    g = torch.Generator().manual_seed(seed)
    x = _bf16_exact(torch.randn(B, L, D, generator=g))
    y = (torch.rand(B, L, generator=g) < 0.05).float()
    y[:, -1] = 0.0
    x2 = _bf16_exact(torch.randn(B, L, D2, generator=g)) if D2 else None
    return x, x2, y, torch.full((B,), L, dtype=torch.int64)


DECODE_MARGIN = 1e-2


def _ragged_batch(B, L, D, seed, D2=None, crf=False):
    """len ~ U{L/4..L}, one full-length and one shortest document; padded inputs are zero, padded targets -1 (0 for the CRF collater:
    EncoderDataset.py:20-27)"""
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(L // 4, L + 1, (B,), generator=g)
    lengths[0], lengths[B // 2] = L, L // 4
    x = _bf16_exact(torch.randn(B, L, D, generator=g))
    x2 = _bf16_exact(torch.randn(B, L, D2, generator=g)) if D2 else None
    y = (torch.rand(B, L, generator=g) < 0.05).float()
    for b, n in enumerate(lengths.tolist()):
        x[b, n:] = 0.0
        if x2 is not None:
            x2[b, n:] = 0.0
        y[b, n - 1] = 0.0
        y[b, n:] = 0.0 if crf else -1.0
    return x, x2, y, lengths


def _check_greedy_lists(model, args, lengths, ref_scores, exact):
    """boundary lists of `model.forward` at th 0.4 / 0.5 against the oracle's (models/CRF.py:358-369, :597-610)"""
    from oracle import restatement as R
    lens = lengths.tolist()
    flips = 0
    for th in (0.4, 0.5):
        model.th = th
        _, got = model(*args, lengths)
        ref = R.greedy_decode(ref_scores.detach(), lengths, th, True)
        assert [len(t) for t in got] == lens
        if exact:
            assert got == ref, th
            continue
        prob = torch.sigmoid(ref_scores.detach()[:, :, 0].double())
        for b, n in enumerate(lens):
            for i in range(n):
                if got[b][i] != ref[b][i]:
                    flips += 1
                    assert abs(float(prob[b, i]) - th) < DECODE_MARGIN, (th, b, i, float(prob[b, i]))
    model.th = None
    return flips


def _crf_path_score(feats, trans, path, start, stop):
    s, prev = 0.0, start
    for t, tag in enumerate(path):
        s += float(trans[tag, prev]) + float(feats[t, tag])
        prev = tag
    return s + float(trans[stop, prev])


def _check_viterbi(model, xd, lengths, hcpu, p, exact):
    """Viterbi paths (models/CRF.py:172-216): identical in fp32; in bf16 the path found must score within 2e-2 rel of the oracle's best UNDER THE
    ORACLE'S features and at least 97 % of the tags agree"""
    from oracle import restatement as R
    Lq = hcpu.shape[1]
    score, paths = model(xd, lengths)
    with torch.no_grad():
        w, b, tr = p['crf.fc.weight'].detach(), p['crf.fc.bias'].detach(), p['crf.transitions'].detach()
        ref_score, ref_paths = R.crf_viterbi(hcpu.detach(), R.create_mask(Lq, lengths), w, b, tr)
        feats = hcpu.detach() @ w.t() + b
    assert [len(q) for q in paths] == lengths.tolist()
    agree = total = 0
    for bi, n in enumerate(lengths.tolist()):
        if exact:
            assert paths[bi] == ref_paths[bi], bi
            continue
        assert all(0 <= t < 2 for t in paths[bi])
        s_here = _crf_path_score(feats[bi], tr, paths[bi], model.start_idx, model.stop_idx)
        assert s_here <= float(ref_score[bi]) + 1e-3 and float(ref_score[bi]) - s_here < 2e-2 * max(1.0, abs(float(ref_score[bi]))), bi
        agree += sum(int(a == r) for a, r in zip(paths[bi], ref_paths[bi]))
        total += n
    if not exact:
        assert agree >= 0.97 * total, (agree, total)


def test_transformer_64x256x1792_bf16_against_the_oracle():
    from oracle import restatement as R
    from multimodaltopicsegmentation_amd import _lib as L, ops
    from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter
    B, Lq, D, FF, HEADS = 64, 256, 1792, 256, 8
    m = _round_to_bf16_(Transformer_segmenter(2, D, FF, num_layers=1, nheads=HEADS, loss_fn='FocalLoss', window_size=30,
                                               compute_dtype='bf16', max_position_embedding=Lq + 2, seed=21).to(DEV))
    x, _, y, lengths = _full_batch(B, Lq, D, 22)
    xd, yd = x.to(DEV), y.to(DEV)
    ops._plan_cache.clear()                                  # timer labels = the plan of a shape's FIRST launch in this process: forget those
                                                             # of earlier tests that forced a tile through mts_set_option
    m.loss_and_grad(xd, lengths, yd, True)                   # first call: the planner's choice per shape is recorded (timer labels)
    timer = ops.KernelTimer()
    ops.TIMER = timer
    try:
        loss, scores = m.loss_and_grad(xd, lengths, yd, True)
    finally:
        ops.TIMER = None
    torch.cuda.synchronize()
    ran = timer.summary()
    N = B * Lq
    tiles = {(t[1], t[4], t[5], t[6]): t[7] for t in ran if t[0] == 'gemm'}          # (layout, M, N, K) -> tile the planner chose
    assert tiles[(L.NT, N, 3 * D, D)] == 224 and tiles[(L.NT, N, D, D)] == 226          # q|k|v (persistent kernel) and attention-output projection (residual: one tile per workgroup, 226)
    assert tiles[(L.NN, N, D, 3 * D)] == 225 and tiles[(L.NN, N, D, D)] == 225          # their data gradients (225: the 224-wide tile on the four-wave kernel of gemm224n.hip)
    assert tiles[(L.TN, 3 * D, D, N)] == 224                                             # q|k|v weight gradient (split-K)
    assert any(t[0] == 'ffn_fwd' and t[1] == N for t in ran) and any(t[0] == 'ffn_bwd' and t[1] == N for t in ran)   # fused block ran
    assert not any(t[0] == 'gemm' and t[1] in (L.NT, L.NN) and FF in (t[5], t[6]) for t in ran)   # ... instead of its four data GEMMs

    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = _oracle_params(m, torch.float64)
    ref_scores = R.transformer_scores(x.double(), lengths, p, HEADS, R.pyramidal_radii(1, 30), attention=R.band_attention_blocked)
    ref_loss = R.tagger_loss(ref_scores, lengths, y.double(), 'FocalLoss')
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    d = (scores.detach().cpu().double().view(B, Lq, 1) - ref_scores.detach()).abs()
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    # key.bias: the softmax over a window is invariant to a shift common to all its keys, so d loss / d key.bias is exactly 0
    kb = 'model.model.encoder.layer.0.attention.self.key.bias'
    worst = _compare_grads(m, p, exact_zero={kb: 'model.model.encoder.layer.0.attention.self.query.bias'})
    flips = _check_greedy_lists(m, (xd,), lengths, ref_scores, exact=False)
    print('transformer 64x256x1792 worst (max-ratio, l2-ratio):', max(v[0] for v in worst.values()), max(v[1] for v in worst.values()), 'decode flips inside the margin:', flips)


@pytest.mark.parametrize('head', ['focal', 'crf'])
def test_bilstm_64x256x1792_bf16_against_the_oracle(head):
    from oracle import restatement as R
    from multimodaltopicsegmentation_amd import BiLSTM, BiRnnCrf
    B, Lq, D, H, NL = 64, 256, 1792, 256, 2
    if head == 'focal':
        m = BiLSTM(2, D, H, num_layers=NL, loss_fn='FocalLoss', compute_dtype='bf16', seed=31)
    else:
        m = BiRnnCrf(2, D, H, num_layers=NL, compute_dtype='bf16', seed=31)
    m = _round_to_bf16_(m.to(DEV))
    x, _, y, lengths = _full_batch(B, Lq, D, 32)
    loss, out = m.loss_and_grad(x.to(DEV), lengths, y.to(DEV), True)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = _oracle_params(m, torch.float64)
    if head == 'focal':
        ref_out = R.bilstm_scores(x.double(), lengths, p, NL, batched=True)
        ref_loss = R.tagger_loss(ref_out, lengths, y.double(), 'FocalLoss')
    else:
        hcpu = R.rnn_forward(x.double(), lengths, p, 'model.', NL, True, batched=True)
        ref_loss = R.crf_nll(hcpu, y.double(), R.create_mask(Lq, lengths), p['crf.fc.weight'], p['crf.fc.bias'], p['crf.transitions'])
        ref_out = hcpu @ p['crf.fc.weight'].t() + p['crf.fc.bias']
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * max(1.0, abs(float(ref_loss))), (float(loss), float(ref_loss))
    d = (out.detach().cpu().double().view_as(ref_out) - ref_out.detach()).abs()
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    worst = _compare_grads(m, p)
    if head == 'focal':
        _check_greedy_lists(m, (x.to(DEV),), lengths, ref_out, exact=False)
    else:
        _check_viterbi(m, x.to(DEV), lengths, hcpu, p, exact=False)
    print(f'bilstm ({head}) 64x256x1792 worst (max-ratio, l2-ratio):', max(v[0] for v in worst.values()), max(v[1] for v in worst.values()))


def test_late_fusion_64x512_bf16_against_the_oracle():
    from oracle import restatement as R
    from multimodaltopicsegmentation_amd import BiLSTMLateFusion
    B, Lq, D1, D2, H, NL = 64, 512, 1024, 768, 256, 2
    m = _round_to_bf16_(BiLSTMLateFusion(2, [D1, D2], H, num_layers=NL, loss_fn='FocalLoss', compute_dtype='bf16', seed=41).to(DEV))
    # The GPU runs the full 64 x 512 batch; its second half repeats the first 32 documents, so loss and gradients (means over the
    # batch) equal those of the 32-document batch and the CPU oracle -- 2 x 2 x 2 x 512 dependent steps, the slowest item of the
    # suite -- evaluates 32 documents.  Every one of the 64 score rows is still compared (a document group handled wrongly shows).
    h1, h2, hy, hl = _full_batch(B // 2, Lq, D1, 42, D2)
    x1, x2, y, lengths = torch.cat([h1, h1]), torch.cat([h2, h2]), torch.cat([hy, hy]), torch.cat([hl, hl])
    loss, scores = m.loss_and_grad(x1.to(DEV), x2.to(DEV), lengths, y.to(DEV), True)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = _oracle_params(m, torch.float32)
    half_scores = R.late_fusion_scores(h1, h2, hl, p, NL, batched=True)
    ref_loss = R.tagger_loss(half_scores, hl, hy, 'FocalLoss')
    ref_loss.backward()
    ref_scores = torch.cat([half_scores, half_scores])
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    d = (scores.detach().cpu().view(B, Lq, 1) - ref_scores.detach()).abs()
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    worst = _compare_grads(m, p)
    _check_greedy_lists(m, (x1.to(DEV), x2.to(DEV)), lengths, ref_scores, exact=False)
    print('late fusion 64x512 worst (max-ratio, l2-ratio):', max(v[0] for v in worst.values()), max(v[1] for v in worst.values()))


# ------------------------------------------------------------------------------------------------ fp32 parity mode: bit-exact boundary lists
@pytest.mark.parametrize('arch', ['transformer', 'transformer_w120', 'bilstm', 'bilstm_crf'])
def test_fp32_parity_mode_64x256x1792_boundary_lists_are_bit_exact(arch):
    """north_star: "outputs match the reference CPU path ... (bit-exact boundary indices under greedy decode)".  The drop-in classes' default
    arithmetic (fp32) at the BASELINE shape against the fp64 oracle on the same fp32 weights and inputs: scores 5e-5 abs, loss 1e-5 rel, and
    every one of the 16 384 greedy decisions at th 0.4 and 0.5 (every Viterbi tag for the CRF head) identical."""
    from oracle import restatement as R
    from multimodaltopicsegmentation_amd import BiLSTM, BiRnnCrf
    from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter
    B, Lq, D = 64, 256, 1792
    x, _, y, lengths = _ragged_batch(B, Lq, D, 52, crf=arch == 'bilstm_crf')
    if arch == 'transformer':
        m = Transformer_segmenter(2, D, 256, num_layers=1, nheads=8, loss_fn='FocalLoss', window_size=30, compute_dtype='fp32',
                                  max_position_embedding=Lq + 2, seed=51).to(DEV)
    elif arch == 'transformer_w120':
        # the drop-in class as users build it: TextSegmenter's default attention_window 120 (radius 60: the generic fp32 kernels)
        from multimodaltopicsegmentation_amd import TextSegmenter
        torch.manual_seed(51)
        m = TextSegmenter(2, D, 256, architecture='Transformer', nheads=8, loss_fn='FocalLoss', compute_dtype='fp32').to(DEV).model
        assert m.radii == [60]
    elif arch == 'bilstm':
        m = BiLSTM(2, D, 256, num_layers=2, loss_fn='FocalLoss', compute_dtype='fp32', seed=51).to(DEV)
    else:
        m = BiRnnCrf(2, D, 256, num_layers=2, compute_dtype='fp32', seed=51).to(DEV)
    xd, yd = x.to(DEV), y.to(DEV)
    loss, out = m.loss_and_grad(xd, lengths, yd, False)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    with torch.no_grad():
        if arch in ('transformer', 'transformer_w120'):
            radii = R.pyramidal_radii(1, 120 if arch == 'transformer_w120' else 30)
            ref = R.transformer_scores(x.double(), lengths, p, 8, radii, attention=R.band_attention_blocked)
            ref_loss = R.tagger_loss(ref, lengths, y.double(), 'FocalLoss')
        elif arch == 'bilstm':
            ref = R.bilstm_scores(x.double(), lengths, p, 2, batched=True)
            ref_loss = R.tagger_loss(ref, lengths, y.double(), 'FocalLoss')
        else:
            hcpu = R.rnn_forward(x.double(), lengths, p, 'model.', 2, True, batched=True)
            ref_loss = R.crf_nll(hcpu, y.double(), R.create_mask(Lq, lengths), p['crf.fc.weight'], p['crf.fc.bias'], p['crf.transitions'])
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss))), (float(loss), float(ref_loss))
    if arch == 'bilstm_crf':
        _check_viterbi(m, xd, lengths, hcpu, p, exact=True)
        return
    scores, _ = m(xd, lengths)
    valid = R.create_mask(Lq, lengths)
    d = (scores.cpu().double() - ref)[valid].abs()
    assert float(d.max()) <= 5e-5, float(d.max())
    _check_greedy_lists(m, (xd,), lengths, ref, exact=True)


# ------------------------------------------------------------------------------------------------ ragged batches at full size
def test_transformer_64x256x1792_ragged_packed_bf16_against_the_oracle():
    """What real documents take (train_fit.py:104-106 pads every batch; the training path keeps the valid sentences only): len ~ U{L/4..L},
    the packed path must be the one that ran (scores come back as [n_valid, 1]), loss / scores / every gradient against the fp64 oracle."""
    from oracle import restatement as R
    from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter
    B, Lq, D, FF, HEADS = 64, 256, 1792, 256, 8
    m = _round_to_bf16_(Transformer_segmenter(2, D, FF, num_layers=1, nheads=HEADS, loss_fn='FocalLoss', window_size=30,
                                               compute_dtype='bf16', max_position_embedding=Lq + 2, seed=61).to(DEV))
    x, _, y, lengths = _ragged_batch(B, Lq, D, 62)
    n_valid = int(lengths.sum())
    assert n_valid < 0.9 * B * Lq
    loss, scores = m.loss_and_grad(x.to(DEV), lengths, y.to(DEV), True)
    torch.cuda.synchronize()
    assert tuple(scores.shape) == (n_valid, 1), scores.shape          # pack_rows = 'auto' packed the batch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = _oracle_params(m, torch.float64)
    ref_scores = R.transformer_scores(x.double(), lengths, p, HEADS, R.pyramidal_radii(1, 30), attention=R.band_attention_blocked)
    ref_loss = R.tagger_loss(ref_scores, lengths, y.double(), 'FocalLoss')
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    valid = R.create_mask(Lq, lengths)
    d = (scores.detach().cpu().double().view(-1) - ref_scores.detach()[valid].view(-1)).abs()        # packed rows = valid sentences, document after document
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    kb = 'model.model.encoder.layer.0.attention.self.key.bias'
    worst = _compare_grads(m, p, exact_zero={kb: 'model.model.encoder.layer.0.attention.self.query.bias'})
    flips = _check_greedy_lists(m, (x.to(DEV),), lengths, ref_scores, exact=False)
    print('transformer ragged/packed worst:', max(v[0] for v in worst.values()), max(v[1] for v in worst.values()), 'flips', flips)


def _band_radii_that_ran(run):
    """run() under a KernelTimer: the radii of the band-attention forward and backward launches (('band_fwd', B, L, D, heads, radius))"""
    from multimodaltopicsegmentation_amd import ops
    timer = ops.KernelTimer()
    ops.TIMER = timer
    try:
        out = run()
    finally:
        ops.TIMER = None
    torch.cuda.synchronize()
    ran = timer.summary()
    return out, {t[5] for t in ran if t[0] == 'band_fwd'}, {t[5] for t in ran if t[0] == 'band_bwd'}


def _transformer_bf16_against_the_oracle(m, radii, x, y, lengths, packed):
    """loss_and_grad of a bf16 Transformer_segmenter (weights and inputs bf16-exact) against the fp64 oracle at every radius: loss, scores,
    every gradient (key.bias of every layer: exactly 0), greedy lists inside DECODE_MARGIN"""
    from oracle import restatement as R
    B, Lq, _ = x.shape
    n_valid = int(lengths.sum())
    (loss, scores), fwd_radii, bwd_radii = _band_radii_that_ran(lambda: m.loss_and_grad(x.to(DEV), lengths, y.to(DEV), True))
    assert m.radii == list(radii) and fwd_radii == set(radii) and bwd_radii == set(radii), (m.radii, fwd_radii, bwd_radii)
    if packed:
        assert n_valid < 0.9 * B * Lq
        assert tuple(scores.shape) == (n_valid, 1), scores.shape      # pack_rows = 'auto' packed the batch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = _oracle_params(m, torch.float64)
    ref_scores = R.transformer_scores(x.double(), lengths, p, m.nheads, radii, attention=R.band_attention_blocked)
    ref_loss = R.tagger_loss(ref_scores, lengths, y.double(), 'FocalLoss')
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    valid = R.create_mask(Lq, lengths)
    d = (scores.detach().cpu().double().view(-1) - ref_scores.detach()[valid].view(-1)).abs()      # packed: valid rows document after document
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    # key.bias: the softmax over a window is invariant to a shift common to all its keys -- in every layer
    lay = 'model.model.encoder.layer.{}.attention.self.'
    worst = _compare_grads(m, p, exact_zero={lay.format(li) + 'key.bias': lay.format(li) + 'query.bias' for li in range(len(radii))})
    flips = _check_greedy_lists(m, (x.to(DEV),), lengths, ref_scores, exact=False)
    return worst, flips


@pytest.mark.parametrize('batch', ['equal', 'ragged'])
def test_transformer_2layer_pyramidal_64x256x1792_bf16_against_the_oracle(batch):
    """-nl 2 at window 30 (models/CRF.py:529): layer 0 at radius 30 (MFMA 6 key blocks, two-kernel backward), layer 1 at radius 15 (4 key
    blocks, one-pass backward), both at head dim 224, equal lengths and ragged (packed rows)"""
    from oracle import restatement as R
    from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter
    B, Lq, D, FF, HEADS = 64, 256, 1792, 256, 8
    m = _round_to_bf16_(Transformer_segmenter(2, D, FF, num_layers=2, nheads=HEADS, loss_fn='FocalLoss', window_size=30,
                                               compute_dtype='bf16', max_position_embedding=Lq + 2, seed=91).to(DEV))
    x, _, y, lengths = _full_batch(B, Lq, D, 92) if batch == 'equal' else _ragged_batch(B, Lq, D, 93)
    worst, flips = _transformer_bf16_against_the_oracle(m, R.pyramidal_radii(2, 30), x, y, lengths, packed=batch == 'ragged')
    print(f'transformer 2-layer ({batch}) worst (max-ratio, l2-ratio):', max(v[0] for v in worst.values()), max(v[1] for v in worst.values()),
          'flips', flips)


def test_transformer_default_window_64x256x1792_bf16_against_the_oracle():
    """The drop-in class as users build it: TextSegmenter without attention_window -> window 120, radius 60 (MFMA 10 key blocks at head dim
    224), ragged documents on the packed path"""
    from oracle import restatement as R
    from multimodaltopicsegmentation_amd import TextSegmenter
    B, Lq, D = 64, 256, 1792
    torch.manual_seed(95)
    m = _round_to_bf16_(TextSegmenter(2, D, 256, architecture='Transformer', nheads=8, loss_fn='FocalLoss', compute_dtype='bf16').to(DEV).model)
    assert m.radii == [60]
    x, _, y, lengths = _ragged_batch(B, Lq, D, 96)
    worst, flips = _transformer_bf16_against_the_oracle(m, R.pyramidal_radii(1, 120), x, y, lengths, packed=True)
    print('transformer default window (radius 60) worst (max-ratio, l2-ratio):', max(v[0] for v in worst.values()),
          max(v[1] for v in worst.values()), 'flips', flips)


@pytest.mark.parametrize('head', ['focal', 'crf'])
def test_bilstm_64x256x1792_ragged_bf16_against_the_oracle(head):
    from oracle import restatement as R
    from multimodaltopicsegmentation_amd import BiLSTM, BiRnnCrf
    B, Lq, D, H, NL = 64, 256, 1792, 256, 2
    if head == 'focal':
        m = BiLSTM(2, D, H, num_layers=NL, loss_fn='FocalLoss', compute_dtype='bf16', seed=71)
    else:
        m = BiRnnCrf(2, D, H, num_layers=NL, compute_dtype='bf16', seed=71)
    m = _round_to_bf16_(m.to(DEV))
    x, _, y, lengths = _ragged_batch(B, Lq, D, 72, crf=head == 'crf')
    loss, out = m.loss_and_grad(x.to(DEV), lengths, y.to(DEV), True)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = _oracle_params(m, torch.float64)
    valid = R.create_mask(Lq, lengths)
    if head == 'focal':
        ref_out = R.bilstm_scores(x.double(), lengths, p, NL, batched=True)
        ref_loss = R.tagger_loss(ref_out, lengths, y.double(), 'FocalLoss')
    else:
        hcpu = R.rnn_forward(x.double(), lengths, p, 'model.', NL, True, batched=True)
        ref_loss = R.crf_nll(hcpu, y.double(), valid, p['crf.fc.weight'], p['crf.fc.bias'], p['crf.transitions'])
        ref_out = hcpu @ p['crf.fc.weight'].t() + p['crf.fc.bias']
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * max(1.0, abs(float(ref_loss))), (float(loss), float(ref_loss))
    d = (out.detach().cpu().double().view_as(ref_out) - ref_out.detach())[valid].abs()
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    worst = _compare_grads(m, p)
    if head == 'focal':
        _check_greedy_lists(m, (x.to(DEV),), lengths, ref_out, exact=False)
    else:
        _check_viterbi(m, x.to(DEV), lengths, hcpu, p, exact=False)
    print(f'bilstm ({head}) ragged worst:', max(v[0] for v in worst.values()), max(v[1] for v in worst.values()))


def test_late_fusion_32x512_ragged_bf16_against_the_oracle():
    """configs[4] per-GPU shape class with ragged documents (32 of them: the CPU oracle's 2 x 2 x 2 x 512 dependent steps are the slowest
    item of the suite; two document groups of the CU-quad recurrences, both encoders on their own streams)"""
    from oracle import restatement as R
    from multimodaltopicsegmentation_amd import BiLSTMLateFusion
    B, Lq, D1, D2, H, NL = 32, 512, 1024, 768, 256, 2
    m = _round_to_bf16_(BiLSTMLateFusion(2, [D1, D2], H, num_layers=NL, loss_fn='FocalLoss', compute_dtype='bf16', seed=81).to(DEV))
    x1, x2, y, lengths = _ragged_batch(B, Lq, D1, 82, D2)
    loss, scores = m.loss_and_grad(x1.to(DEV), x2.to(DEV), lengths, y.to(DEV), True)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = _oracle_params(m, torch.float32)
    ref_scores = R.late_fusion_scores(x1, x2, lengths, p, NL, batched=True)
    ref_loss = R.tagger_loss(ref_scores, lengths, y, 'FocalLoss')
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    valid = R.create_mask(Lq, lengths)
    d = (scores.detach().cpu().view(B, Lq, 1) - ref_scores.detach())[valid].abs()
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    worst = _compare_grads(m, p)
    _check_greedy_lists(m, (x1.to(DEV), x2.to(DEV)), lengths, ref_scores, exact=False)
    print('late fusion ragged worst:', max(v[0] for v in worst.values()), max(v[1] for v in worst.values()))
