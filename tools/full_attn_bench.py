#!/usr/bin/env python3
"""Time the full-attention kernels (csrc/full_attn.hip) and the full-attention training step against the restricted one.

  * mts_full_attn_fwd / _bwd at 64 x 256 x 1792 (8 heads, head dim 224) and on one 2437-sentence document, bf16;
    each with its fraction of 6.3 TB/s (algorithmic bytes: q|k|v, ctx, lse once; the backward also dCtx in and dq|dk|dv out)
    and of the 2.5 PF bf16 MFMA peak (QK^T and PV in the forward; QK^T, dP, dQ, dK, dV in the backward);
  * one loss_and_grad of Transformer_segmenter (1 layer, bf16, 64 x 256 x 1792, F 256): restricted (window 30, radius 15)
    against restricted=False, in the same process.
Prints one line per measurement (median of 5 repetitions of 20 back-to-back calls)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import ops  # noqa: E402
from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter  # noqa: E402

DEV = 'cuda'
HBM, MFMA = 6.3e12, 2.5e15


def timed(fn, reps=5, inner=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(inner):
            fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3 / inner)
    return sorted(ts)[len(ts) // 2]


def kernels(B, Lq, D, heads, label):
    hd, N = D // heads, B * Lq
    g = torch.Generator(device=DEV).manual_seed(1)
    qkv = (torch.randn(N, 3 * D, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
    qkv[:, :D] /= hd ** 0.5
    dctx = torch.randn(N, D, device=DEV, generator=g).to(torch.bfloat16)
    ctx = torch.empty(N, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(N, heads, device=DEV)
    dqkv = torch.empty_like(qkv)
    dbias = torch.empty(3 * D, device=DEV)
    fwd = lambda: ops.full_attn_fwd(qkv, None, B, Lq, D, heads, ctx, lse)
    bwd = lambda: ops.full_attn_bwd(qkv, None, lse, ctx, dctx, B, Lq, D, heads, dqkv, dbias=dbias)
    pairs = B * heads * Lq * Lq
    for name, fn, nbytes, flops in (
            ('fwd', fwd, N * 3 * D * 2 + N * D * 2 + N * heads * 4, 4.0 * pairs * hd),
            ('bwd', bwd, N * 3 * D * 2 + 2 * N * D * 2 + N * heads * 4 + N * 3 * D * 2, 10.0 * pairs * hd)):
        us = timed(fn)
        print(f'full_attn_{name} {label}: {us:8.1f} us   {nbytes / 1e6:6.1f} MB -> {nbytes / (us * 1e-6) / HBM * 100:5.1f} % of 6.3 TB/s   '
              f'{flops / 1e9:6.1f} GFLOP -> {flops / (us * 1e-6) / MFMA * 100:5.1f} % of the bf16 MFMA peak')


def step(B=64, Lq=256, D=1792):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, Lq, D, generator=g).to(DEV)
    y = (torch.rand(B, Lq, generator=g) < 0.05).float().to(DEV)
    lengths = torch.full((B,), Lq, dtype=torch.int64)
    out = {}
    for name, kw in (('restricted (radius 15)', dict(window_size=30)), ('full', dict(restricted=False))):
        m = Transformer_segmenter(2, D, 256, num_layers=1, nheads=8, loss_fn='FocalLoss', compute_dtype='bf16',
                                  max_position_embedding=Lq + 2, seed=3, **kw).to(DEV)
        out[name] = timed(lambda: m.loss_and_grad(x, lengths, y, True), inner=10)
        print(f'training step 1 layer {B} x {Lq} x {D}, {name}: {out[name]:8.1f} us')
    r = out['full'] / out['restricted (radius 15)']
    print(f'full / restricted step: {r:.2f}x')


if __name__ == '__main__':
    kernels(64, 256, 1792, 8, '64 x 256 x 1792 (hd 224)')
    kernels(1, 2437, 1792, 8, '1 x 2437 x 1792 (hd 224)')
    step()
