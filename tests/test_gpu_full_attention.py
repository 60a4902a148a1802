"""Full self-attention (csrc/full_attn.hip) and Transformer_segmenter(restricted=False) on a real MI355X, against the fp64 oracle
of tests/full_attention_oracle.py and the reference's fixture tests/golden/g17_full_attention.npz.

Kernel level, bf16 and fp32, head dims 16 / 32 / 64 / 96 / 128 / 160 / 192 / 224 / 256 / 264 / 300 / 512 (every instantiation the
dispatcher can select, and both refusals), L from 1 to 2437 plus one 4096-row document, equal / ragged / packed lengths, attention dropout 0.1 (keep mask rebuilt on the host from include/mts.h's rule), each checked on the operands the
kernel got, widened to fp64:
  * ctx, lse, dq / dk / dv: the elementwise bars and L2 ratio of test_gpu_band_hd224.py; padded query rows equal to the oracle (not
    zero); dk / dv of padded keys exactly 0;
  * the fused q/k/v bias gradient = column sums of dqkv as stored;
  * guard rows past every buffer untouched; a second backward bitwise equal to the first.
Model level: g17 in fp32 and bf16; 64 x 256 x 1792 with 1 and 2 layers, equal and ragged (packed) batches, bf16 against the fp64
oracle at the full-size bars of test_gpu_parity_fullsize.py; fp32 boundary lists identical to the oracle's; one NativeTrainer step
equal to Adam (eps 1e-7) on the oracle's gradients; hipGraph inference bitwise equal to eager.
"""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.full_attention_oracle import full_attention, full_encoder, full_scores, keep_mask, tagger_loss

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 96

# name: (B, Lq, D, heads, lengths or None, packed, dropout p)
CASES = {
    'hd16_ragged':    (3, 37, 64, 4, [37, 1, 20], False, 0.0),
    'hd16_packed':    (3, 37, 64, 4, [37, 1, 20], True, 0.1),
    'hd32_equal':     (2, 100, 128, 4, None, False, 0.0),
    'hd64_drop':      (2, 130, 256, 4, [130, 65], False, 0.1),
    'hd224_ragged':   (2, 300, 448, 2, [300, 131], False, 0.0),
    'hd224_packed':   (4, 385, 448, 2, [385, 1, 129, 30], True, 0.0),
    'hd224_d1792':    (2, 256, 1792, 8, [256, 173], False, 0.1),
    'hd256_ragged':   (2, 200, 512, 2, [200, 77], False, 0.0),
    'L1':             (1, 1, 448, 2, None, False, 0.0),
    'L2437':          (1, 2437, 448, 2, None, False, 0.0),
    'L4096':          (1, 4096, 64, 2, [4096], True, 0.0),
    # the instantiations no case above selects (tests/test_instantiation_cover_cpu.py keeps the list): KK = 3 .. 6 of the matrix-core
    # kernels at 64 + 6 query rows (two query tiles), 2 x 32 + 6 keys (a ragged last key step) and a short document; MAXU = 16 of the
    # generic kernels (head dims above 256); both sides of the two refusals.  An 8th field names the modes that must refuse the case.
    'hd96':            (2, 70, 192, 2, [70, 33], False, 0.0),
    'hd128_packed':    (2, 70, 256, 2, [70, 33], True, 0.1),
    'hd160_drop':      (2, 70, 320, 2, [70, 33], False, 0.1),
    'hd192':           (2, 70, 384, 2, [70, 1], False, 0.0),
    'hd264':           (2, 70, 528, 2, [70, 33], False, 0.0),                        # 264 % 32 != 0: bf16 'mfma' runs the generic kernels
    'hd300_fp32_edge': (2, 70, 600, 2, [70, 33], False, 0.1, ('mfma', 'generic')),   # fp32: 162304 B of LDS; bf16: 300 % 8 != 0
    'hd512':           (2, 40, 1024, 2, [40, 9], False, 0.0, ('fp32',)),             # bf16: 141824 B of LDS; fp32: 272896 B
}
MODES = ('mfma', 'generic', 'fp32')     # mfma: bf16, matrix-core kernels where hd % 32 == 0; generic: bf16 with full_mfma 0


def _seed(name):
    return 104729 * (1 + list(CASES).index(name))


def _case(name):
    return CASES[name][:7]


def _refused_in(name):
    return CASES[name][7] if len(CASES[name]) > 7 else ()


def _inputs(name, dtype):
    B, Lq, D, heads, lengths, packed, p = _case(name)
    g = torch.Generator().manual_seed(2000 + list(CASES).index(name))
    qkv = torch.randn(B, Lq, 3, D, generator=g) * 0.7
    qkv[:, :, 0] /= math.sqrt(D // heads) / 2.0               # q as the model feeds it (pre-scaled), a little sharper than uniform
    dctx = torch.randn(B, Lq, D, generator=g)
    return qkv.reshape(B, Lq, 3 * D).to(dtype), dctx.to(dtype)


def _ratios(got, ref):
    return float((got - ref).abs().max()) / float(ref.abs().max()), float((got - ref).norm()) / float(ref.norm())


def _check(got, ref, rtol, atol, bar_l2, msg):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f'{msg}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e})'
    if float(ref.abs().max()) == 0.0:                  # e.g. dq / dk of a one-sentence document: the softmax of one key is 1 whatever q, k
        return 0.0, 0.0
    mr, l2 = _ratios(got, ref)
    assert l2 <= bar_l2, f'{msg}: L2 ratio {l2:.3e} > {bar_l2:.0e}'
    return mr, l2


def _guarded(rows, cols, dtype):
    buf = torch.full((rows + GUARD, cols), float('nan'), dtype=dtype, device=DEV)
    return buf, buf[:rows]


@pytest.mark.parametrize('name,mode', [(c, m) for c in CASES for m in MODES])
def test_full_attention_against_the_oracle(name, mode):
    from multimodaltopicsegmentation_amd import _lib as L, ops
    B, Lq, D, heads, lengths, packed, p = _case(name)
    hd = D // heads
    dtype = torch.float32 if mode == 'fp32' else torch.bfloat16
    qkv, dctx = _inputs(name, dtype)
    lens = lengths if lengths is not None else [Lq] * B
    len_t = torch.tensor(lens)
    valid = torch.arange(Lq).view(1, Lq) < len_t.view(B, 1)
    if packed:
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int).tolist()
        n_rows = sum(lens)
        row0 = torch.tensor(starts, dtype=torch.int32, device=DEV)
        row_of = torch.zeros((B, Lq), dtype=torch.long)
        for b, (s, n) in enumerate(zip(starts, lens)):
            row_of[b, :n] = torch.arange(s, s + n)
        sel = valid.view(-1)
    else:
        n_rows, row0 = B * Lq, None
        row_of = torch.arange(B * Lq).view(B, Lq)
        sel = torch.ones(B * Lq, dtype=torch.bool)
    li32 = torch.tensor(lens, dtype=torch.int32, device=DEV) if lengths is not None else None

    qbuf, qd = _guarded(n_rows, 3 * D, dtype)
    qd.copy_(qkv.view(B * Lq, 3 * D)[sel].to(DEV))
    dbuf, dd = _guarded(n_rows, D, dtype)
    dd.copy_(dctx.view(B * Lq, D)[sel].to(DEV))
    cbuf, ctx = _guarded(n_rows, D, dtype)
    lbuf, lse = _guarded(n_rows, heads, torch.float32)
    gbuf, dqkv = _guarded(n_rows, 3 * D, dtype)
    dbias = torch.full((3 * D,), float('nan'), device=DEV)
    seed = _seed(name)
    if mode in _refused_in(name):                          # outside the entry points' contract: refused before any launch, nothing written
        try:
            L.check(L.lib.mts_set_option(b'full_mfma', 0 if mode == 'generic' else 1))
            with pytest.raises(NotImplementedError):
                ops.full_attn_fwd(qd, li32, B, Lq, D, heads, ctx, lse, row0=row0, drop_p=p, drop_seed=seed)
            with pytest.raises(NotImplementedError):
                ops.full_attn_bwd(qd, li32, lse, ctx, dd, B, Lq, D, heads, dqkv, dbias=dbias, row0=row0, drop_p=p, drop_seed=seed)
            torch.cuda.synchronize()
        finally:
            L.check(L.lib.mts_set_option(b'full_mfma', 1))
        for buf, what in ((cbuf, 'ctx'), (lbuf, 'lse'), (gbuf, 'dqkv'), (dbias, 'dbias')):
            assert torch.isnan(buf.float()).all(), f'{what}: written by a refused call'
        return
    try:
        L.check(L.lib.mts_set_option(b'full_mfma', 0 if mode == 'generic' else 1))
        ops.full_attn_fwd(qd, li32, B, Lq, D, heads, ctx, lse, row0=row0, drop_p=p, drop_seed=seed)
        ops.full_attn_bwd(qd, li32, lse, ctx, dd, B, Lq, D, heads, dqkv, dbias=dbias, row0=row0, drop_p=p, drop_seed=seed)
        first = dqkv.clone()
        ops.full_attn_bwd(qd, li32, lse, ctx, dd, B, Lq, D, heads, dqkv, dbias=dbias, row0=row0, drop_p=p, drop_seed=seed)
        torch.cuda.synchronize()
    finally:
        L.check(L.lib.mts_set_option(b'full_mfma', 1))
    assert torch.equal(first.view(torch.int16) if dtype == torch.bfloat16 else first.view(torch.int32),
                       dqkv.view(torch.int16) if dtype == torch.bfloat16 else dqkv.view(torch.int32)), 'backward not bitwise reproducible'
    for buf, rows, what in ((cbuf, n_rows, 'ctx'), (lbuf, n_rows, 'lse'), (gbuf, n_rows, 'dqkv')):
        assert torch.isnan(buf[rows:].float()).all(), f'{what}: a kernel wrote past the end of its buffer'

    # fp64 oracle on exactly the operands the kernels got
    keep = None
    if p > 0:
        k = torch.from_numpy(keep_mask(n_rows * heads * Lq, p, seed).reshape(n_rows, heads, Lq)).double()
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        keep = k[row_of.view(-1)].view(B, Lq, heads, Lq) * scale
        assert (keep == 0).any()
    x64 = qkv.double().view(B, Lq, 3, heads, hd)
    q, k_, v = (x64[:, :, i].clone().requires_grad_(True) for i in range(3))
    rctx, rlse = full_attention(q, k_, v, len_t, keep=keep, return_lse=True)
    dref = dctx.double().view(B, Lq, heads, hd)
    if packed:
        dref = dref * valid.view(B, Lq, 1, 1)              # padded query rows do not exist in a packed batch: they contribute nothing
    rctx.backward(dref)
    fp32 = dtype == torch.float32
    tol = dict(rtol=2e-5, atol=2e-5, bar_l2=1e-5) if fp32 else dict(rtol=1e-2, atol=1e-2, bar_l2=1e-2)
    tolb = dict(rtol=1e-4, atol=1e-4, bar_l2=1e-4) if fp32 else dict(rtol=3e-2, atol=3e-2, bar_l2=1e-2)
    worst = {}
    got_ctx = ctx.cpu().double()
    worst['ctx'] = _check(got_ctx, rctx.detach().reshape(B * Lq, D)[sel], msg='ctx', **tol)
    vrow = valid.view(-1)[sel]
    if (~vrow).any():                                      # padded query rows: BERT's values, not zeros
        assert float(got_ctx[~vrow].abs().max()) > 0
    worst['lse'] = _check(lse.cpu(), rlse.detach().reshape(B * Lq, heads)[sel], rtol=1e-5, atol=1e-5 if fp32 else 1e-4, bar_l2=1e-5,
                          msg='lse')
    got = dqkv.cpu().double()
    assert not torch.isnan(got).any()
    colsum = got.sum(0)
    assert float(((dbias.cpu().double() - colsum).abs() - 1e-5 * colsum.abs()).max()) <= 1e-5 * n_rows, 'dbias'
    g5 = got.view(n_rows, 3, heads, hd)
    if (~vrow).any():
        assert float(g5[~vrow][:, 1:].abs().max()) == 0.0, 'dk / dv on a padded key'
    for kk, (what, ref) in enumerate((('dq', q.grad / math.sqrt(hd)), ('dk', k_.grad), ('dv', v.grad))):
        worst[what] = _check(g5[:, kk], ref.reshape(B * Lq, heads, hd)[sel], msg=what, **tolb)
    print(f'\nfull attention {name} [{mode}] worst (max-ratio, L2 ratio): ' + ', '.join(f'{k} {a:.2e} / {b:.2e}' for k, (a, b) in worst.items()))


def test_the_lds_bound_is_where_full_fill_puts_it():
    """full_fill refuses a shape whose generic kernels need more than 160 KiB of LDS (128 row strides + 8704 bytes).  In fp32 that puts
    the bound between head dims 300 (162304 bytes: accepted, case hd300_fp32_edge) and 304 (166400 bytes): 304 is refused by the forward
    and by the backward, nothing written."""
    from multimodaltopicsegmentation_amd import ops
    from tests.test_instantiation_cover_cpu import full_generic_lds
    assert full_generic_lds(300, 4) == 162304 <= 160 * 1024 < full_generic_lds(304, 4) == 166400
    assert CASES['hd300_fp32_edge'][2] // CASES['hd300_fp32_edge'][3] == 300 and 'fp32' not in _refused_in('hd300_fp32_edge')
    B, Lq, D, heads = 1, 8, 608, 2
    qbuf, qd = _guarded(B * Lq, 3 * D, torch.float32)
    qd.copy_(torch.randn(B * Lq, 3 * D))
    dbuf, dd = _guarded(B * Lq, D, torch.float32)
    dd.copy_(torch.randn(B * Lq, D))
    cbuf, ctx = _guarded(B * Lq, D, torch.float32)
    lbuf, lse = _guarded(B * Lq, heads, torch.float32)
    gbuf, dqkv = _guarded(B * Lq, 3 * D, torch.float32)
    dbias = torch.full((3 * D,), float('nan'), device=DEV)
    with pytest.raises(NotImplementedError, match='LDS'):
        ops.full_attn_fwd(qd, None, B, Lq, D, heads, ctx, lse)
    with pytest.raises(NotImplementedError, match='LDS'):
        ops.full_attn_bwd(qd, None, lse, ctx, dd, B, Lq, D, heads, dqkv, dbias=dbias)
    torch.cuda.synchronize()
    for buf, what in ((cbuf, 'ctx'), (lbuf, 'lse'), (gbuf, 'dqkv'), (dbias, 'dbias')):
        assert torch.isnan(buf).all(), f'{what}: written by a refused call'


# ------------------------------------------------------------------------------------------------ model level
def _g17(k):
    g17 = H.load('g17_full_attention')
    g = {n[len(k) + 1:]: v for n, v in g17.items() if n.startswith(k + '_')}
    D, heads, ff, NL = (int(v) for v in g['cfg'])
    return g, D, heads, ff, NL


def _g17_model(k, dtype):
    from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter
    g, D, heads, ff, NL = _g17(k)
    n_out = g['scores'].shape[-1]
    loss_fn = 'FocalLoss' if n_out == 1 else 'CrossEntropy'
    m = Transformer_segmenter(2, D, ff, num_layers=NL, nheads=heads, loss_fn=loss_fn, restricted=False, compute_dtype=dtype)
    w = {n: torch.from_numpy(H.seeded_param(n, s, int(g['seed']))) for n, s in H.band_param_shapes(D, ff, NL, n_out).items()}
    m.load_state_dict(w)
    return m.to(DEV).eval(), g, loss_fn


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('k', ['a', 'b'])
def test_g17_reference_fixture(k, dtype):
    m, g, loss_fn = _g17_model(k, dtype)
    f32 = dtype == 'fp32'
    x, lengths, tags = torch.from_numpy(g['x']).to(DEV), torch.from_numpy(g['lengths']), torch.from_numpy(g['tags']).to(DEV)
    loss = m.loss(x, lengths, tags)
    loss.backward()
    assert abs(loss.item() - float(g['loss'])) < (2e-6 if f32 else 2e-2) * max(1.0, abs(float(g['loss']))), (loss.item(), float(g['loss']))
    m.th = 0.5
    scores, got = m(x, lengths)
    np.testing.assert_allclose(scores.cpu().numpy(), g['scores'], atol=2e-5 if f32 else 5e-2, rtol=0)    # every row, padded ones too
    if f32:
        assert got == H.split_tags(g['tags0.5'], g['lengths'].tolist())
    rtol, atol = (2e-3, 2e-6) if f32 else (8e-2, 3e-3)
    Lq = g['x'].shape[1]
    for n, prm in m.named_parameters():
        gv = m.logical_view({n: prm.grad}, n).detach().float().cpu().numpy()
        if 'position_embeddings' in n:
            assert not gv[Lq:].any()
            gv = gv[:Lq]
        if 'key.bias' in n:
            continue            # exactly 0 in theory (softmax shift invariance): both sides hold rounding noise
        if 'g.' + n in g:
            ref = g['g.' + n]
            assert (np.abs(gv - ref) <= atol + rtol * np.abs(ref)).all(), (n, float(np.abs(gv - ref).max()), float(np.abs(ref).max()))
        else:
            ref = g['ghead.' + n]
            head = gv.ravel()[:32]
            assert (np.abs(head - ref) <= atol + rtol * np.abs(ref) + (0 if f32 else 2e-2 * np.abs(ref).max())).all(), n
            np.testing.assert_allclose(H.checksum(gv)[1:], g['gsum.' + n][1:], rtol=1e-3 if f32 else 5e-2)


BAR_MAX, BAR_L2 = 2e-2, 1e-2        # test_gpu_parity_fullsize.py


def _full_size_model(NL, dtype, seed):
    from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter
    m = Transformer_segmenter(2, 1792, 256, num_layers=NL, nheads=8, loss_fn='FocalLoss', restricted=False, compute_dtype=dtype,
                              max_position_embedding=256, seed=seed).to(DEV)
    with torch.no_grad():
        m.flat.copy_(m.flat.to(torch.bfloat16).to(torch.float32))     # bf16-exact weights: oracle and product see the same operands
    return m.eval()


def _batch(ragged, seed, B=64, L=256, D=1792):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, D, generator=g).to(torch.bfloat16).to(torch.float32)
    y = (torch.rand(B, L, generator=g) < 0.05).float()
    lengths = torch.full((B,), L, dtype=torch.int64)
    if ragged:
        lengths = torch.randint(L // 4, L + 1, (B,), generator=g)
        lengths[0], lengths[B // 2] = L, L // 4
        for b, n in enumerate(lengths.tolist()):
            x[b, n:] = 0.0
            y[b, n - 1] = 0.0
            y[b, n:] = -1.0
    y[:, -1] = torch.where(y[:, -1] < 0, y[:, -1], torch.zeros_like(y[:, -1]))
    return x, y, lengths


@pytest.mark.timeout(900)
@pytest.mark.parametrize('NL,ragged', [(1, False), (1, True), (2, False), (2, True)])
def test_full_size_bf16_against_the_oracle(NL, ragged):
    m = _full_size_model(NL, 'bf16', 31 + NL)
    x, y, lengths = _batch(ragged, 41 + NL)
    loss, scores = m.loss_and_grad(x.to(DEV), lengths, y.to(DEV), True)
    torch.cuda.synchronize()
    B, Lq = x.shape[:2]
    if ragged:
        assert scores.shape[0] == int(lengths.sum())         # the packed path ran
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    ref_scores = full_scores(x.double(), lengths, p, 8, NL)
    ref_loss = tagger_loss(ref_scores, lengths, y.double(), 'FocalLoss')
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 2e-3 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    valid = torch.arange(Lq).view(1, Lq) < lengths.view(B, 1)
    got = scores.detach().cpu().double().view(-1)
    ref = ref_scores.detach()[..., 0][valid] if ragged else ref_scores.detach().view(-1)
    d = (got - ref).abs()
    assert float(d.max()) <= 3e-2 and float(d.mean()) <= 3e-3, (float(d.max()), float(d.mean()))
    worst = 0.0
    for name, gv in m.grad_views().items():
        a = gv.detach().cpu().double()
        r = p[name].grad
        r = torch.zeros_like(a) if r is None else r.double()
        if 'key.bias' in name:       # exactly 0 (a shift common to all keys of a softmax): both sides are rounding noise
            qb = p[name.replace('key.bias', 'query.bias')].grad.double()
            assert float(a.abs().max()) <= BAR_MAX * float(qb.abs().max()), name
            continue
        rmax, rl2 = float(r.abs().max()), float(r.norm())
        assert rmax > 0, name
        dmax, dl2 = float((a - r).abs().max()), float((a - r).norm())
        assert dmax <= BAR_MAX * rmax, (name, dmax, rmax)
        assert dl2 <= BAR_L2 * rl2, (name, dl2, rl2)
        worst = max(worst, dl2 / rl2)
    print(f'\nfull attention {NL} layer(s) ragged={ragged}: worst L2 ratio {worst:.2e}')


@pytest.mark.timeout(900)
def test_fp32_boundary_lists_identical_to_the_oracle():
    from oracle import restatement as R
    m = _full_size_model(1, 'fp32', 51)
    x, y, lengths = _batch(True, 52)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref_scores = full_scores(x.double(), lengths, p, 8, 1)
    for th in (0.4, 0.5):
        m.th = th
        _, got = m(x.to(DEV), lengths)
        assert got == R.greedy_decode(ref_scores, lengths, th, True), th


def test_native_trainer_step_is_adam_on_the_oracle_gradients():
    from multimodaltopicsegmentation_amd.trainer import NativeTrainer
    m, g, loss_fn = _g17_model('a', 'fp32')          # eval mode: no dropout, so the step's gradient is the fixture's
    init = m.flat.detach().clone()
    p = {n: torch.from_numpy(np.asarray(v)).double().requires_grad_(True) for n, v in
         ((n, H.seeded_param(n, s, int(g['seed']))) for n, s in H.band_param_shapes(64, 32, 2, 1).items())}
    x, lengths, tags = torch.from_numpy(g['x']), torch.from_numpy(g['lengths']), torch.from_numpy(g['tags'])
    tagger_loss(full_scores(x.double(), lengths, p, 4, 2), lengths, tags.double(), 'FocalLoss').backward()
    tr = NativeTrainer(m, lr=1e-3, optimizer='Adam')
    tr.step({'src_tokens': x.to(DEV), 'src_lengths': lengths, 'tgt_tokens': tags.to(DEV)})
    torch.cuda.synchronize()
    lr, eps = 1e-3, 1e-7
    sd_new = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    m.flat.data.copy_(init)
    sd_old = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    moved = 0
    for n, prm in p.items():
        gr = prm.grad
        if gr is None:
            gr = torch.zeros_like(prm)
        step = (sd_new[n].double().cpu() - sd_old[n].double().cpu())
        # step 1 of Adam (bias-corrected): -lr * g / (|g| + eps)
        want = -lr * gr / (gr.abs() + eps)
        sure = gr.abs() > 1e-4                 # where |g| >> eps the update is -lr * sign(g) whatever the summation order
        assert torch.allclose(step[sure], want[sure], rtol=0, atol=2e-6), n
        assert float(step.abs().max()) <= lr * (1 + 1e-5), n
        moved += int(sure.sum())
    assert moved > 1000


def test_hipgraph_inference_is_bitwise_eager():
    m, g, _ = _g17_model('a', 'bf16')
    x, lengths = torch.from_numpy(g['x']).to(DEV), torch.from_numpy(g['lengths'])
    s_eager, t_eager = m(x, lengths)
    m.inference_graphs = True
    s1, t1 = m(x, lengths)          # capture
    s2, t2 = m(x, lengths)          # replay
    torch.cuda.synchronize()
    assert torch.equal(s_eager, s1) and torch.equal(s_eager, s2) and t_eager == t1 == t2
    assert len(m._graphs) == 1


def test_training_mode_attention_dropout_against_the_oracle():
    """restricted=False in training mode: attention dropout 0.1 on every layer (packed batch), against the fp64 oracle with the keep
    masks rebuilt from include/mts.h's rule and the seeds the tagger draws (taggers._drop_seed)."""
    m, g, loss_fn = _g17_model('a', 'fp32')
    D, heads, NL = 64, 4, 2
    x, lengths, tags = torch.from_numpy(g['x']), torch.from_numpy(g['lengths']), torch.from_numpy(g['tags'])
    B, Lq = x.shape[:2]
    m.train()
    c0 = m._drop_calls
    loss, scores = m.loss_and_grad(x.to(DEV), lengths, tags.to(DEV), True)
    torch.cuda.synchronize()
    assert m._drop_calls == c0 + NL                               # one attention-dropout seed per layer, nothing else (dropout_in = 0)
    lens = lengths.tolist()
    assert scores.shape[0] == sum(lens)                           # packed: the keep index runs over packed rows
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int)
    row_of = torch.zeros((B, Lq), dtype=torch.long)
    for b, (s0, n) in enumerate(zip(starts, lens)):
        row_of[b, :n] = torch.arange(s0, s0 + n)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1)))
    keeps = []
    for li in range(NL):
        seed = (torch.initial_seed() * 1000003 + (c0 + 1 + li) * 7919) & 0x7FFFFFFFFFFFFFFF
        k = torch.from_numpy(keep_mask(sum(lens) * heads * Lq, 0.1, seed).reshape(sum(lens), heads, Lq)).double()
        keeps.append(k[row_of.view(-1)].view(B, Lq, heads, Lq) * scale)
    p = {n: torch.from_numpy(H.seeded_param(n, s, int(g['seed']))).double().requires_grad_(True)
         for n, s in H.band_param_shapes(D, 32, NL, 1).items()}
    ref_scores = full_scores(x.double(), lengths, p, heads, NL, keeps=keeps)
    ref_loss = tagger_loss(ref_scores, lengths, tags.double(), 'FocalLoss')
    ref_loss.backward()
    valid = torch.arange(Lq).view(1, Lq) < lengths.view(B, 1)
    got = scores.detach().cpu().double().view(-1)
    assert float((got - torch.from_numpy(g['scores'][..., 0])[valid].double()).abs().max()) > 1e-3     # the dropout changed the scores ...
    assert float((got - ref_scores.detach()[..., 0][valid]).abs().max()) < 2e-5                          # ... as the oracle says
    assert abs(float(loss) - float(ref_loss)) < 2e-6 * max(1.0, abs(float(ref_loss))), (float(loss), float(ref_loss))   # ... as the oracle says
    views = m.grad_views()
    for n, prm in p.items():
        if 'key.bias' in n:
            continue
        a = views[n].detach().cpu().double()
        r = prm.grad.double()
        if 'position_embeddings' in n:
            a, r = a[:Lq], r[:Lq]
        assert float((a - r).norm()) <= 1e-4 * float(r.norm()), (n, float((a - r).norm()), float(r.norm()))
