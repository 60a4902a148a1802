#!/usr/bin/env python3
"""Cost of gradient clipping on the native training step (NativeTrainer(gradient_clip_val=...); DESIGN.md §3 "Gradient clipping").

Shape: BASELINE configs[1] -- the one-layer restricted-window transformer at 64 x 256 x 1792 in bf16.  Two trainers over two models of
the same seed, one unclipped and one clipping by norm with max_norm = 1e-8 of the first step's gradient norm (the coefficient is checked to
be below 1 on every timed step), take steps IN TURN in one process: a drift of the machine hits both.  Every step sits between two device events;
nothing synchronises until the last step is queued.  Prints both medians, their difference and one JSON line.

  python tools/grad_clip_bench.py [--steps 60] [--warmup 10]
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o tr -- python tools/grad_clip_bench.py --trace     (a run of its own)
  python tools/grad_clip_bench.py --stats <dir>/.../tr_kernel_stats.csv       (no GPU needed)

--stats turns the trace's per-kernel totals into bytes per second on the ALGORITHMIC bytes of the spans the optimizer steps (n live
elements): grad_sumsq_kernel reads 4 n; adam_kernel reads p, g, m, v and writes p, m, v and the bf16 mirror = 30 n.  A pure read
stream should reach at least 0.7 of adam_kernel's rate."""
import argparse
import csv
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd.taggers import Transformer_segmenter  # noqa: E402
from multimodaltopicsegmentation_amd.trainer import NativeTrainer  # noqa: E402

B, L, D = 64, 256, 1792
SUMSQ_BYTES, ADAM_BYTES = 4, 30                                  # per live element
# max_norm / the first step's norm.  The same batch is stepped on and on and its gradient shrinks by orders of magnitude; this far down
# Adam's eps dominates the clipped gradient, the parameters all but stand still and the coefficient stays below 1 for any number of
# steps.  The launches and the bytes they move do not depend on the coefficient.
CLIP_FRACTION = 1e-8


def model():
    return Transformer_segmenter(2, D, 256, num_layers=1, nheads=8, loss_fn='FocalLoss', window_size=30, compute_dtype='bf16', seed=1234)


def live_elements():
    """elements of the flat buffer the optimizer (and so the norm) covers at this batch length"""
    tr = NativeTrainer(model())
    tr._last_L = L
    spans = tr._adam_spans()
    return sum(b - a for a, b in spans), len(spans)


def batch(dev):
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(B, L, D, generator=g)
    y = (torch.rand(B, L, generator=g) < 0.05).float()
    y[:, -1] = 0.0
    return {'src_tokens': x.to(dev), 'src_lengths': torch.full((B,), L, dtype=torch.int64), 'tgt_tokens': y.to(dev), 'src_tokens2': None}


def run(steps, warmup, trace):
    dev = 'cuda'
    bt = batch(dev)
    plain = NativeTrainer(model().to(dev), lr=1e-3, optimizer='Adam')
    plain.step(bt)
    norm0 = float(plain.model.grad_flat().double().norm())
    clipped = NativeTrainer(model().to(dev), lr=1e-3, optimizer='Adam', gradient_clip_val=CLIP_FRACTION * norm0)
    clipped.step(bt)
    trainers = {'unclipped': plain, 'clipped': clipped}
    for _ in range(warmup):
        for tr in trainers.values():
            tr.step(bt)
    torch.cuda.synchronize()
    events = {name: [] for name in trainers}
    coefs = []
    for _ in range(steps):
        for name, tr in trainers.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            tr.step(bt)
            e.record()
            events[name].append((s, e))
        coefs.append(clipped.last_clip_coef.clone())
    torch.cuda.synchronize()
    coefs = torch.stack(coefs).cpu()
    assert bool((coefs < 1.0).all()), 'clipping was not active on every timed step'
    n = sum(b - a for a, b in clipped._adam_spans())
    if trace:
        print(f'traced {steps + warmup + 1} steps per trainer; live elements {n} ({n * SUMSQ_BYTES / 1e6:.1f} MB read by the norm)')
        return
    ms = {name: sorted(s.elapsed_time(e) for s, e in ev)[len(ev) // 2] for name, ev in events.items()}
    for name, v in ms.items():
        print(f'{name:9s} step {B} x {L} x {D} bf16: {v:.4f} ms (median of {steps}, the two in turn)')
    print(f'clipped - unclipped: {(ms["clipped"] - ms["unclipped"]) * 1e3:+.1f} us   ({ms["clipped"] / ms["unclipped"]:.4f}x); '
          f'coefficient {float(coefs.min()):.3e} .. {float(coefs.max()):.3e}; norm reads {n * SUMSQ_BYTES / 1e6:.1f} MB')
    print(json.dumps({'shape': [B, L, D], 'dtype': 'bf16', 'steps': steps, 'warmup': warmup, 'live_elements': n,
                      'ms_per_step': {'unclipped': round(ms['unclipped'], 4), 'clipped': round(ms['clipped'], 4)},
                      'overhead_us': round((ms['clipped'] - ms['unclipped']) * 1e3, 1), 'max_norm': CLIP_FRACTION * norm0,
                      'clip_coef': [float(coefs.min()), float(coefs.max())]}))


def stats(path):
    rows = list(csv.DictReader(open(path)))
    n, n_spans = live_elements()                                 # spans: in front of and behind the position table's untouched rows

    def pick(sub):
        r = [x for x in rows if sub in x['Name']]
        return (sum(int(x['Calls']) for x in r), sum(float(x['TotalDurationNs']) for x in r)) if r else (0, 0.0)

    out = {}
    for label, sub, nbytes, per_step in (('adam_kernel', 'adam_kernel', ADAM_BYTES * n, n_spans),
                                         ('adam_clip_kernel', 'adam_clip_kernel', ADAM_BYTES * n, n_spans),
                                         ('grad_sumsq_kernel', 'grad_sumsq_kernel', SUMSQ_BYTES * n, 1),
                                         ('grad_norm_finalize_kernel', 'grad_norm_finalize_kernel', 0, 1)):
        calls, ns = pick(sub)
        if not calls:
            print(f'{label}: not in the trace')
            continue
        us = ns / (calls / per_step) / 1e3
        out[label] = nbytes / (us * 1e-6) if nbytes else None
        rate = f'{nbytes / 1e6:7.1f} MB -> {out[label] / 1e12:.3f} TB/s' if nbytes else ''
        print(f'{label:26s} {calls:5d} launches, {us:8.2f} us per step   {rate}')
    if out.get('adam_kernel') and out.get('grad_sumsq_kernel'):
        print(f'grad_sumsq_kernel / adam_kernel byte rate: {out["grad_sumsq_kernel"] / out["adam_kernel"]:.3f}   (live elements {n})')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--trace', action='store_true', help='the program to put behind rocprofv3 --kernel-trace --stats --: fewer steps, no report')
    ap.add_argument('--stats', metavar='KERNEL_STATS_CSV', help='byte rates from a trace taken with --trace (no GPU)')
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
    else:
        run(20 if a.trace else a.steps, 5 if a.trace else a.warmup, a.trace)
