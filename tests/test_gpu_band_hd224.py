"""Band attention at head dim 224 (d = 1792 / 8 heads, the BASELINE width) for every window the models reach, against the fp64 oracle.

The one-sided radius decides which kernel runs (csrc/band_attn_mfma.hip ``band_slots`` / ``pick_nkb`` / ``mts_band_mfma_bwd``; the
generic kernels of csrc/band_attn.hip otherwise):

  radius <= 15   32 slots        bf16: MFMA, 4 key blocks, one-pass fused backward   (window 30: BASELINE configs[1], layer 1 of -nl 2)
  radius 16-31   64 slots        bf16: MFMA, 6 key blocks, two-kernel backward      (layer 0 of -nl 2 at window 30)
  radius 32-63   96 / 128 slots  bf16: MFMA, 10 key blocks, two-kernel backward     (TextSegmenter's default attention_window 120)
  radius >= 64   >= 160 slots    generic VALU kernels                               (layer 0 of -nl 2 at window 120)

fp32 (the drop-in classes' default) always takes the generic kernels; mts_set_option("band_mfma", 0) sends bf16 there too, and
mts_set_option("band_fused_bwd", 0) the radius <= 15 backward to the two-kernel path.  Every case runs in each of those modes and is
checked on the operands the kernel got (bf16-rounded where the kernel reads bf16), widened to fp64:

  * ctx, dq / dk / dv against oracle.restatement.band_attention and its autograd gradients: elementwise bars of
    test_gpu_kernels.py::test_band_attention_fwd_bwd plus a per-tensor L2 ratio;
  * the saved probabilities slot by slot (slot c <-> key i - radius + c); slots whose key lies outside [0, len_b), pad slots
    c >= 2r + 1 and rows of padded queries exactly 0; ctx and dq / dk / dv rows of padded positions exactly 0;
  * the fused q/k/v bias gradient = column sums of dqkv as stored;
  * attention dropout (p = 0.1) against the oracle with the keep mask rebuilt on the host from the kernels' hash
    (common.h mts_hash32 at index (global_row * heads + h) * slots + c, threshold of band_set_dropout);
  * guard rows past the buffers the kernels were given stay untouched.
"""
import math

import numpy as np
import pytest
import torch

from oracle import restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 160          # rows past every buffer: input guard rows are NaN (never read), output guard rows must stay NaN (never written)

# name: (B, Lq, D, heads, radius, lengths or None, packed, q pre-scaled by 1/sqrt(hd), dropout p)
CASES = {
    'r15':        (2, 300, 448, 2, 15, [300, 131], False, False, 0.0),
    'r15_drop':   (2, 300, 448, 2, 15, [300, 17], False, True, 0.1),
    'r16':        (2, 300, 448, 2, 16, [300, 17], False, False, 0.0),           # first 6-block radius; a document of r + 1 rows
    'r30':        (3, 385, 448, 2, 30, [385, 129, 30], False, True, 0.0),       # tile seams at 128, 256, 384; a document as long as r
    'r30_drop':   (3, 385, 448, 2, 30, [385, 129, 30], False, False, 0.1),
    'r31':        (2, 256, 448, 2, 31, None, False, False, 0.0),                # W = 63 of 64 slots, equal lengths
    'r32':        (2, 300, 448, 2, 32, [300, 33], False, True, 0.0),            # first 10-block radius
    'r60':        (2, 520, 448, 2, 60, [520, 61], False, False, 0.0),           # TextSegmenter's default window 120
    'r60_drop':   (2, 520, 448, 2, 60, [520, 61], False, True, 0.1),
    'r63':        (1, 257, 448, 2, 63, [257], False, True, 0.0),                # the last MFMA radius
    'r64':        (2, 300, 448, 2, 64, [300, 64], False, False, 0.0),           # the first generic radius
    'r120':       (2, 600, 448, 2, 120, [600, 121], False, True, 0.0),          # layer 0 of -nl 2 at window 120
    'r120_drop':  (2, 600, 448, 2, 120, [600, 121], False, False, 0.1),
    'r60_d1792':  (2, 200, 1792, 8, 60, [200, 61], False, True, 0.0),           # the real row stride 3 * 1792 and 8 heads
    'r30_packed': (4, 385, 448, 2, 30, [385, 1, 129, 30], True, False, 0.0),    # row0: documents back to back, a 1-row document
    'r60_packed': (4, 520, 448, 2, 60, [200, 1, 520, 61], True, True, 0.1),
}
MODES = ('mfma', 'generic', 'fp32', 'two_kernel')       # two_kernel: bf16 MFMA with band_fused_bwd 0 (radius <= 15 only)
RUNS = [(c, m) for c in CASES for m in MODES if m != 'two_kernel' or CASES[c][4] <= 15]


# ------------------------------------------------------------------------------------------------ mirror of the dispatch rule
def _band_slots(r):
    return (2 * r + 1 + 31) // 32 * 32


def _kernel_class(mode, hd, r):
    """which kernel pair runs (band_attn.hip mts_band_attn_fwd / _bwd; band_attn_mfma.hip pick_nkb, covered, mts_band_mfma_bwd)"""
    if mode in ('fp32', 'generic') or hd % 32 != 0 or hd > 256:
        return 'generic'
    need = 2 + _band_slots(r) // 16
    nkb = 4 if need <= 4 else 6 if need <= 6 else 10 if need <= 10 else 0
    if nkb == 0:
        return 'generic'
    if nkb == 4:
        return 'fused' if mode == 'mfma' and hd <= 224 else 'mfma4'
    return f'mfma{nkb}'


def test_cases_cover_every_dispatch_class_at_hd224():
    from multimodaltopicsegmentation_amd import ops
    for r in (1, 15, 16, 31, 32, 47, 48, 63, 64, 120, 200):
        assert ops.band_slots(r) == _band_slots(r), r
    got = {}
    for c, m in RUNS:
        B, Lq, D, heads, r = CASES[c][:5]
        assert D // heads == 224, c
        got.setdefault(m, set()).add((_kernel_class(m, D // heads, r), _band_slots(r) // 32))
    assert {k for k, _ in got['mfma']} == {'fused', 'mfma6', 'mfma10', 'generic'}
    assert {k for k, _ in got['two_kernel']} == {'mfma4'}
    assert {s for k, s in got['mfma'] if k == 'mfma10'} == {3, 4}                     # 96 and 128 slots
    for m in ('generic', 'fp32'):
        assert {k for k, _ in got[m]} == {'generic'}
        assert {min(s, 5) for _, s in got[m]} == {1, 2, 3, 4, 5}, m                  # 32, 64, 96, 128 and >= 160 slots
    for m in ('mfma', 'generic', 'fp32'):                                              # dropout in every slot class
        drop = {_band_slots(CASES[c][4]) // 32 for c, mm in RUNS if mm == m and CASES[c][8] > 0}
        assert {min(s, 5) for s in drop} >= {1, 2, 4, 5}, (m, drop)


# ------------------------------------------------------------------------------------------------ host replica of the keep mask
def _keep(n, p, seed):
    """mts_hash32(seed, idx) >= drop_thr for idx 0..n-1; drop_thr as band_set_dropout forms it from the float32 p"""
    idx = np.arange(1, n + 1, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * idx
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    thr = int(max(1.0, min(4294967295.0, float(np.float32(p)) * 4294967296.0)))
    return (z >> np.uint64(32)) >= np.uint64(thr)


def _inputs(name, dtype):
    B, Lq, D, heads, r, lengths, packed, prescale, p = CASES[name]
    hd = D // heads
    g = torch.Generator().manual_seed(1000 + list(CASES).index(name))
    qkv = torch.randn(B, Lq, 3, D, generator=g) * 0.7
    if prescale:
        qkv[:, :, 0] /= math.sqrt(hd)                      # q as the model feeds it: near-uniform softmax
    dctx = torch.randn(B, Lq, D, generator=g)
    return qkv.reshape(B, Lq, 3 * D).to(dtype), dctx.to(dtype)


_oracle_cache = {}


def _oracle(name, dtype, row_of):
    """fp64 ctx, probabilities [B, Lq, heads, slots] and gradients on exactly the operands the kernels get"""
    key = (name, dtype)
    if key in _oracle_cache:
        return _oracle_cache[key]
    B, Lq, D, heads, r, lengths, packed, prescale, p = CASES[name]
    hd, slots, W = D // heads, _band_slots(r), 2 * r + 1
    qkv, dctx = _inputs(name, dtype)
    len_t = torch.tensor(lengths if lengths is not None else [Lq] * B)
    keep = None
    if p > 0:
        k = torch.from_numpy(_keep(B * Lq * heads * slots, p, _seed(name)).reshape(B * Lq, heads, slots)).double()
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        keep = k[row_of.view(-1)].view(B, Lq, heads, slots)[..., :W] * scale
        assert (keep == 0).any()
    x64 = qkv.double().view(B, Lq, 3, heads, hd)
    q, k_, v = (x64[:, :, i].clone().requires_grad_(True) for i in range(3))
    ctx, pr = R.band_attention(q, k_, v, len_t, r, return_probs=True, keep=keep)
    ctx.backward(dctx.double().view(B, Lq, heads, hd))
    pr = torch.nn.functional.pad(pr.detach(), (0, slots - W))
    out = (ctx.detach().reshape(B, Lq, D), pr, q.grad / math.sqrt(hd), k_.grad, v.grad)
    for kk in [kk for kk in _oracle_cache if kk[0] != name]:
        del _oracle_cache[kk]                              # the runs of a case are adjacent: keep that case's (two dtypes) only
    _oracle_cache[key] = out
    return out


def _seed(name):
    return 7919 * (1 + list(CASES).index(name))


def _ratios(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max()) / float(ref.abs().max()), float((got - ref).norm()) / float(ref.norm())


def _check(got, ref, rtol, atol, bar_l2, msg):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f'{msg}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e})'
    mr, l2 = _ratios(got, ref)
    assert l2 <= bar_l2, f'{msg}: L2 ratio {l2:.3e} > {bar_l2:.0e}'
    return mr, l2


def _guarded(rows, cols, dtype, fill=float('nan')):
    buf = torch.full((rows + GUARD, cols), fill, dtype=dtype, device=DEV)
    return buf, buf[:rows]


def _guard_intact(buf, rows, msg):
    assert torch.isnan(buf[rows:].float()).all(), f'{msg}: a kernel wrote past the end of its buffer'


@pytest.mark.parametrize('name,mode', RUNS)
def test_band_attention_hd224_against_the_oracle(name, mode):
    from multimodaltopicsegmentation_amd import _lib as L, ops
    B, Lq, D, heads, r, lengths, packed, prescale, p = CASES[name]
    hd, slots, W = D // heads, ops.band_slots(r), 2 * r + 1
    assert slots == _band_slots(r)
    dtype = torch.float32 if mode == 'fp32' else torch.bfloat16
    qkv, dctx = _inputs(name, dtype)
    lens = lengths if lengths is not None else [Lq] * B
    len_t = torch.tensor(lens)
    valid = torch.arange(Lq).view(1, Lq) < len_t.view(B, 1)                           # [B, Lq]
    if packed:
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
        n_rows = sum(lens)
        row0 = torch.tensor(starts, dtype=torch.int32, device=DEV)
        row_of = torch.full((B, Lq), -1, dtype=torch.long)                             # global (packed) row of each valid (b, i)
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
    pbuf, probs = _guarded(n_rows, heads * slots, torch.float32)
    gbuf, dqkv = _guarded(n_rows, 3 * D, dtype)
    sbuf, dsc = _guarded(n_rows, heads * slots, torch.float32)
    dbias = torch.full((3 * D,), float('nan'), device=DEV)
    seed = _seed(name)
    try:
        L.check(L.lib.mts_set_option(b'band_mfma', 0 if mode == 'generic' else 1))
        L.check(L.lib.mts_set_option(b'band_fused_bwd', 0 if mode == 'two_kernel' else 1))
        ops.band_attn_fwd(qd, li32, B, Lq, D, heads, r, ctx, probs, row0=row0, drop_p=p, drop_seed=seed)
        ops.band_attn_bwd(qd, li32, probs, dd, B, Lq, D, heads, r, dqkv, dsc, dbias=dbias, row0=row0, drop_p=p, drop_seed=seed)
        torch.cuda.synchronize()
    finally:
        L.check(L.lib.mts_set_option(b'band_mfma', 1))
        L.check(L.lib.mts_set_option(b'band_fused_bwd', 1))
    for buf, rows, what in ((cbuf, n_rows, 'ctx'), (pbuf, n_rows, 'probs'), (gbuf, n_rows, 'dqkv'), (sbuf, n_rows, 'dscores')):
        _guard_intact(buf, rows, what)

    ref_ctx, ref_pr, ref_dq, ref_dk, ref_dv = _oracle(name, dtype, row_of)
    fp32 = dtype == torch.float32
    tol = dict(rtol=2e-5, atol=2e-5, bar_l2=1e-5) if fp32 else dict(rtol=1e-2, atol=1e-2, bar_l2=1e-2)
    tolb = dict(rtol=1e-4, atol=1e-4, bar_l2=1e-4) if fp32 else dict(rtol=3e-2, atol=3e-2, bar_l2=1e-2)
    worst = {}

    # the saved probabilities, slot by slot; exact zeros where no key (or no query) is
    pr = probs.cpu().view(n_rows, heads, slots)
    rp = ref_pr.reshape(B * Lq, heads, slots)[sel]
    i = torch.arange(Lq).view(1, Lq, 1)
    j = i - r + torch.arange(slots).view(1, 1, slots)
    zero = (j < 0) | (j >= len_t.view(B, 1, 1)) | (torch.arange(slots) >= W).view(1, 1, slots) | ~valid.view(B, Lq, 1)
    zero = zero.view(B * Lq, 1, slots).expand(B * Lq, heads, slots)[sel]
    assert not torch.isnan(pr).any()
    assert float(pr[zero].abs().max()) == 0.0, 'probability outside the window, in a pad slot or on a padded query'
    worst['probs'] = _check(pr[~zero], rp[~zero], rtol=1e-4, atol=1e-5, bar_l2=1e-5, msg='probs')

    vrow = valid.view(-1)[sel]                                                         # rows of real queries / keys
    got_ctx = ctx.cpu().double()
    if (~vrow).any():
        assert float(got_ctx[~vrow].abs().max()) == 0.0, 'context on a padded query'
    worst['ctx'] = _check(got_ctx, ref_ctx.reshape(B * Lq, D)[sel], msg='ctx', **tol)

    # q/k/v bias gradient fused into the backward = column sums of dqkv as stored
    got = dqkv.cpu().double()
    assert not torch.isnan(got).any()
    colsum = got.sum(0)
    assert float(((dbias.cpu().double() - colsum).abs() - 1e-5 * colsum.abs()).max()) <= 1e-5 * n_rows, 'dbias'
    if (~vrow).any():
        assert float(got[~vrow].abs().max()) == 0.0, 'gradient on a padded row'
    g5 = got.view(n_rows, 3, heads, hd)
    for k, (what, ref) in enumerate((('dq', ref_dq), ('dk', ref_dk), ('dv', ref_dv))):
        worst[what] = _check(g5[:, k], ref.reshape(B * Lq, heads, hd)[sel], msg=f'{what}', **tolb)
    print(f'\nhd224 {name} [{mode}] worst (max-ratio, L2 ratio): ' + ', '.join(f'{k} {a:.2e} / {b:.2e}' for k, (a, b) in worst.items()))
