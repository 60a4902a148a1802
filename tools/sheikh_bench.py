#!/usr/bin/env python3
"""Time the adjacent-pair score kernels (csrc/pair_score.hip) and the SheikhBiLSTM training step against BiLSTM.

  * mts_pair_score_fwd / _bwd at 64 x 256, H = 256, bf16 and fp32, F and G the two halves of one [N, 2H] buffer as the tagger passes
    them; each with its fraction of 6.3 TB/s on the algorithmic bytes (N = B L rows, element size e):
    forward 2 N H e + 4 N, backward 4 N H e + 4 N;
  * one fwd + bwd + Adam step (NativeTrainer) of SheikhBiLSTM(1792, 256, 2) at 64 x 256, bf16 and fp32, against BiLSTM(1792, 256, 2,
    BinaryCrossEntropy) in the same process, the two alternating; dropout_in 0.5 (what TextSegmenter builds) and 0.
Prints one line per measurement (median of 5 repetitions of back-to-back calls).  Kernel times per symbol come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/sheikh_bench.py --step-only` run."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import ops  # noqa: E402
from multimodaltopicsegmentation_amd.rnn_taggers import BiLSTM, SheikhBiLSTM  # noqa: E402
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


def kernels(B=64, Lq=256, H=256, dtype=torch.bfloat16):
    N = B * Lq
    es = 2 if dtype == torch.bfloat16 else 4
    g = torch.Generator(device=DEV).manual_seed(1)
    FG = (torch.randn(N, 2 * H, device=DEV, generator=g) * 0.5).to(dtype)
    ds = torch.randn(B, Lq, device=DEV, generator=g)
    dFG = torch.empty_like(FG)
    scores = torch.empty(N, device=DEV)
    fwd = lambda: ops.pair_score_fwd(FG[:, :H], FG[:, H:], B, Lq, scores)                              # noqa: E731
    bwd = lambda: ops.pair_score_bwd(FG[:, :H], FG[:, H:], ds, B, Lq, dFG[:, :H], dFG[:, H:])          # noqa: E731
    label = f'{B} x {Lq}, H {H}, {"bf16" if es == 2 else "fp32"}'
    for name, fn, nbytes in (('fwd', fwd, 2 * N * H * es + 4 * N), ('bwd', bwd, 4 * N * H * es + 4 * N)):
        us = timed(fn, inner=50)
        print(f'pair_score_{name} {label}: {us:8.1f} us   {nbytes / 1e6:6.1f} MB -> {nbytes / (us * 1e-6) / HBM * 100:5.1f} % of 6.3 TB/s')


def steps(B=64, Lq=256, D=1792, H=256, NL=2):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, Lq, D, generator=g).to(DEV)
    y = (torch.rand(B, Lq, generator=g) < 0.05).float().to(DEV)
    y[:, -1] = 0
    lengths = torch.full((B,), Lq, dtype=torch.int64)
    batch = {'src_tokens': x, 'src_lengths': lengths, 'tgt_tokens': y}
    for dt in ('bf16', 'fp32'):
        for p_in in (0.5, 0.0):
            models = (('BiLSTM', BiLSTM(2, D, H, num_layers=NL, loss_fn='BinaryCrossEntropy', dropout_in=p_in, compute_dtype=dt, seed=3)),
                      ('SheikhBiLSTM', SheikhBiLSTM(2, D, H, NL, dropout_in=p_in, compute_dtype=dt, seed=3)))
            trainers = {name: NativeTrainer(m.to(DEV), lr=1e-4, optimizer='Adam') for name, m in models}
            out = {name: [] for name in trainers}
            for _ in range(3):                                           # the two alternate: a drift of the box hits both
                for name, tr in trainers.items():
                    out[name].append(timed(lambda: tr.step(batch), reps=3, inner=10))
            med = {name: sorted(v)[1] for name, v in out.items()}
            for name in trainers:
                print(f'training step {dt} dropout_in {p_in} {B} x {Lq} x {D}, H {H}, NL {NL}, {name}: {med[name] / 1e3:7.3f} ms   '
                      f'(rounds: {", ".join(f"{v / 1e3:.3f}" for v in out[name])})')
            print(f'SheikhBiLSTM - BiLSTM step, {dt} dropout_in {p_in}: {(med["SheikhBiLSTM"] - med["BiLSTM"]):+.1f} us '
                  f'({med["SheikhBiLSTM"] / med["BiLSTM"]:.3f}x)')


if __name__ == '__main__':
    if '--step-only' not in sys.argv:
        kernels(dtype=torch.bfloat16)
        kernels(dtype=torch.float32)
    steps()
