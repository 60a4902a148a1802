#!/usr/bin/env python3
"""Time the LongT5 local-attention kernels (csrc/t5_local_attn.hip) and the RecurrentLongT5 training step against BiLSTM.

  * mts_t5_local_attn_fwd / _bwd at 64 x 256, 8 heads x 64, radius 120 (TextSegmenter's default window), bf16 (matrix-core and
    generic kernels) and fp32; each with
    its fraction of 6.3 TB/s (algorithmic bytes: q|k|v, ctx, lse once; the backward also dCtx in and dq|dk|dv out) and the FLOPs
    of the band it computes (QK^T and PV over 2r + 1 keys per row in the forward; QK^T, dP, dQ, dK, dV in the backward);
  * one fwd + bwd + Adam step (NativeTrainer) of RecurrentLongT5(512, 256, NL, 8 heads, window 120, FocalLoss) at 64 x 256 for
    NL 1 and 2, bf16 and fp32, against BiLSTM(512, 256, NL) in the same process.
Prints one line per measurement (median of 5 repetitions of back-to-back calls).  Kernel times per symbol come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/recurrent_longt5_bench.py --step-only` run."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import _lib as L, ops  # noqa: E402
from multimodaltopicsegmentation_amd.rnn_taggers import BiLSTM  # noqa: E402
from multimodaltopicsegmentation_amd.t5_taggers import RecurrentLongT5, num_buckets, relative_position_buckets  # noqa: E402
from multimodaltopicsegmentation_amd.trainer import NativeTrainer  # noqa: E402

DEV = 'cuda'
HBM, PEAK = 6.3e12, 2.5e15


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


def kernels(B=64, Lq=256, heads=8, radius=120, dtype=torch.bfloat16, mfma=True):
    inner, N = heads * 64, B * Lq
    es = 2 if dtype == torch.bfloat16 else 4
    g = torch.Generator(device=DEV).manual_seed(1)
    qkv = (torch.randn(N, 3 * inner, device=DEV, generator=g) * 0.5).to(dtype)
    dctx = torch.randn(N, inner, device=DEV, generator=g).to(dtype)
    table = torch.randn(num_buckets(radius), heads, device=DEV, generator=g) * 0.5
    bkt = relative_position_buckets(radius).to(device=DEV, dtype=torch.int32)
    ctx = torch.empty(N, inner, device=DEV, dtype=dtype)
    lse = torch.empty(N, heads, device=DEV)
    dqkv = torch.empty_like(qkv)
    dtable = torch.empty_like(table)
    fwd = lambda: ops.t5_local_attn_fwd(qkv, None, B, Lq, heads, radius, table, bkt, ctx, lse)                     # noqa: E731
    bwd = lambda: ops.t5_local_attn_bwd(qkv, None, B, Lq, heads, radius, table, bkt, lse, ctx, dctx, dqkv, dtable)  # noqa: E731
    keys = sum(min(Lq, i + radius + 1) - max(0, i - radius) for i in range(Lq))                                    # band pairs per (doc, head)
    pairs = B * heads * keys
    label = f'{B} x {Lq}, {heads} x 64, r {radius}, {("bf16 matrix-core" if mfma else "bf16 generic") if es == 2 else "fp32"}'
    L.lib.mts_set_option(b't5_mfma', int(mfma))
    for name, fn, nbytes, flops in (
            ('fwd', fwd, N * 3 * inner * es + N * inner * es + N * heads * 4, 4.0 * pairs * 64),
            ('bwd', bwd, N * 3 * inner * es + 2 * N * inner * es + N * heads * 4 + N * 3 * inner * es, 10.0 * pairs * 64)):
        us = timed(fn)
        print(f't5_local_attn_{name} {label}: {us:8.1f} us   {nbytes / 1e6:6.1f} MB -> {nbytes / (us * 1e-6) / HBM * 100:5.1f} % of 6.3 TB/s   '
              f'{flops / 1e9:6.1f} GFLOP -> {flops / (us * 1e-6) / 1e12:6.1f} TFLOP/s')
    L.lib.mts_set_option(b't5_mfma', 1)


def steps(B=64, Lq=256, D=512, H=256):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, Lq, D, generator=g).to(DEV)
    y = (torch.rand(B, Lq, generator=g) < 0.05).float().to(DEV)
    y[:, -1] = 0
    lengths = torch.full((B,), Lq, dtype=torch.int64)
    batch = {'src_tokens': x, 'src_lengths': lengths, 'tgt_tokens': y}
    for dt in ('bf16', 'fp32'):
        for NL in (1, 2):
            out = {}
            for name, m in (('BiLSTM', BiLSTM(2, D, H, num_layers=NL, loss_fn='FocalLoss', compute_dtype=dt, seed=3)),
                            ('RecurrentLongT5', RecurrentLongT5(2, D, H, num_layers=NL, nheads=8, loss_fn='FocalLoss', window_size=120,
                                                                compute_dtype=dt, seed=3))):
                m = m.to(DEV)
                tr = NativeTrainer(m, lr=1e-4, optimizer='Adam')
                out[name] = timed(lambda: tr.step(batch), inner=10)
                print(f'training step {dt} NL {NL} {B} x {Lq} x {D}, H {H}, {name}: {out[name] / 1e3:7.3f} ms')
            print(f'RecurrentLongT5 / BiLSTM step, {dt} NL {NL}: {out["RecurrentLongT5"] / out["BiLSTM"]:.2f}x')


if __name__ == '__main__':
    if '--step-only' not in sys.argv:
        kernels(dtype=torch.bfloat16)
        kernels(dtype=torch.bfloat16, mfma=False)
        kernels(dtype=torch.float32)
    steps()
