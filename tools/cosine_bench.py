#!/usr/bin/env python3
"""Time the cosine auxiliary segment loss (csrc/segment_cosine.hip) and the BiLSTM training step with and without it.

  * mts_segment_cosine_fwd / _bwd at 64 x 256, W = 512 (H = 256), bf16 and fp32, a boundary about every 10 rows; the forward reads
    N W e bytes of x once (N = B L rows, element size e), the backward reads and writes dx (accumulate = 1): 2 N W e; both with their
    fraction of 6.3 TB/s on these algorithmic bytes;
  * the host side of a step: ops.segment_table for that batch (built and uploaded on every call: the timed steps include it);
  * one fwd + bwd + Adam step (NativeTrainer) of BiLSTM(1792, 256, 2, FocalLoss) at 64 x 256, bf16 and fp32, with
    cosine_loss=True (boundary-derived segments, the collater's rule) against the same model without, the two alternating.
Prints one line per measurement (median of 5 repetitions of back-to-back calls).  Kernel times per symbol come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/cosine_bench.py --step-only` run."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import ops  # noqa: E402
from multimodaltopicsegmentation_amd.rnn_taggers import BiLSTM  # noqa: E402
from multimodaltopicsegmentation_amd.trainer import NativeTrainer  # noqa: E402

DEV = 'cuda'
HBM = 6.3e12


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


def boundary_batch(B, Lq, rate=0.1, seed=2):
    """tags with a boundary about every 1 / rate rows and the segments the collater derives from them"""
    rng = np.random.default_rng(seed)
    y = (rng.random((B, Lq)) < rate).astype(np.float32)
    y[:, -1] = 0
    return torch.from_numpy(y), [(np.flatnonzero(y[b] == 1) + 1).tolist() for b in range(B)]


def kernels(B=64, Lq=256, W=512, dtype=torch.bfloat16):
    N = B * Lq
    es = 2 if dtype == torch.bfloat16 else 4
    g = torch.Generator(device=DEV).manual_seed(1)
    x = (torch.randn(N, W, device=DEV, generator=g) * 0.5).to(dtype)
    dx = torch.zeros_like(x)
    _, segments = boundary_batch(B, Lq)
    lengths = torch.full((B,), Lq, dtype=torch.int64)
    t0 = time.perf_counter()
    tab_h = ops.segment_table(segments, lengths, B, Lq)
    host_ms = (time.perf_counter() - t0) * 1e3
    tab = ops.segment_tables(segments, lengths, B, Lq, DEV)
    out = torch.empty(2, device=DEV)
    ws = ops.segment_cosine_fwd(x, tab, out)
    fwd = lambda: ops.segment_cosine_fwd(x, tab, out)                                           # noqa: E731
    bwd = lambda: ops.segment_cosine_bwd(tab, 0.1 / tab.n_pair, dx, ws, accumulate=True)        # noqa: E731
    label = f'{B} x {Lq}, W {W}, {"bf16" if es == 2 else "fp32"}, {tab.n_seg} segments, {tab.n_pair} pairs'
    for name, fn, nbytes in (('fwd', fwd, N * W * es), ('bwd', bwd, 2 * N * W * es)):
        us = timed(fn, inner=50)
        print(f'segment_cosine_{name} {label}: {us:8.1f} us   {nbytes / 1e6:6.1f} MB -> {nbytes / (us * 1e-6) / HBM * 100:5.1f} % of 6.3 TB/s')
    print(f'ops.segment_table (host, {tab_h.n_seg} segments): {host_ms:.2f} ms; workspace {ws.numel() / 1e6:.1f} MB')


def steps(B=64, Lq=256, D=1792, H=256, NL=2):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, Lq, D, generator=g).to(DEV)
    y, segments = boundary_batch(B, Lq)
    lengths = torch.full((B,), Lq, dtype=torch.int64)
    batch = {'src_tokens': x, 'src_lengths': lengths, 'tgt_tokens': y.to(DEV), 'src_segments': segments}
    for dt in ('bf16', 'fp32'):
        trainers = {name: NativeTrainer(BiLSTM(2, D, H, num_layers=NL, loss_fn='FocalLoss', compute_dtype=dt, seed=3).to(DEV), lr=1e-4,
                                        optimizer='Adam', cosine_loss=cos) for name, cos in (('plain', False), ('cosine', True))}
        out = {name: [] for name in trainers}
        for _ in range(3):                                               # the two alternate: a drift of the box hits both
            for name, tr in trainers.items():
                out[name].append(timed(lambda: tr.step(batch), reps=3, inner=10))
        med = {name: sorted(v)[1] for name, v in out.items()}
        for name in trainers:
            print(f'training step {dt} {B} x {Lq} x {D}, H {H}, NL {NL}, {name}: {med[name] / 1e3:7.3f} ms   '
                  f'(rounds: {", ".join(f"{v / 1e3:.3f}" for v in out[name])})')
        print(f'cosine - plain step, {dt}: {(med["cosine"] - med["plain"]):+.1f} us ({med["cosine"] / med["plain"]:.3f}x)')


if __name__ == '__main__':
    if '--step-only' not in sys.argv:
        kernels(dtype=torch.bfloat16)
        kernels(dtype=torch.float32)
    steps()
