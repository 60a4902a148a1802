#!/usr/bin/env python3
"""Cost of one validation epoch's decision-threshold sweep (ThresholdSweep; DESIGN.md §3 "Decision-threshold search").

Workload: 55 documents in batches of 8, lengths drawn by a fixed seed from the RadioNews statistics of SURVEY §5 (84 .. 2 437 sentences,
log-normal around the median 359, the two extremes present), 19 thresholds, 1-wide scores.  In ONE process:

  (a) the host loop: the tags of every threshold are decoded beforehand (not timed); timed is metrics.py per document and threshold in
      test_step's order plus the sums -- what the reference's disabled hook does, on this machine's CPU;
  (b) the device path: wall clock from the first ``add`` to the returned ``table()``, so the seven launches, the one copy and its
      synchronise are inside; warmed, repeated, median and spread reported;
  (c) the seven launches alone between two device events.

The two tables are compared for equality.  Prints one JSON line.

--metric scaiano: the same three legs for the WinPR sweep (ThresholdSweep(metric='scaiano'), mts_winpr_sweep) on the same documents;
the host loop is metrics.WinPR(tags, target) per document and threshold on integer lists, with the sweep's (0, 0, 0) where it raises
ZeroDivisionError.  The Pk / WindowDiff / F1 sweep is timed in the same process as the yardstick ('pk_yardstick').

  python tools/threshold_sweep_bench.py [--reps 50] [--metric Pk|scaiano]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import DEFAULT_THRESHOLDS, ThresholdSweep, metrics, ops  # noqa: E402
from multimodaltopicsegmentation_amd.threshold_search import host_metrics  # noqa: E402

DOCS, BATCH = 55, 8


def workload():
    rng = np.random.default_rng(55)
    lengths = np.clip(np.round(np.exp(rng.normal(np.log(359.0), 0.75, size=DOCS))), 84, 2437).astype(int)
    lengths[0], lengths[1] = 2437, 84
    g = torch.Generator().manual_seed(55)
    batches = []
    for s in range(0, DOCS, BATCH):
        ls = [int(v) for v in lengths[s:s + BATCH]]
        sc = (2 * torch.randn(len(ls), max(ls), 1, generator=g)).cuda()
        tg = (torch.rand(len(ls), max(ls), generator=g) < 0.05).float().cuda()
        batches.append((sc, tg, torch.tensor(ls, dtype=torch.int32, device='cuda'), ls))
    return lengths, batches


def device_path(batches, metric=None):
    s = ThresholdSweep(metric=metric)
    for sc, tg, li, _ in batches:
        s.add(sc, tg, li)
    return s.table()


def time_device(batches, reps, metric=None):
    """-> (table, sorted wall ms of first add .. table(), sorted ms of the launches alone)"""
    for _ in range(5):
        tab = device_path(batches, metric)
    wall = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tab = device_path(batches, metric)
        wall.append(1e3 * (time.perf_counter() - t0))
    wall.sort()
    winpr = metric is not None
    outs = [torch.empty(sc.shape[0], len(DEFAULT_THRESHOLDS), 3 if winpr else 6, dtype=torch.int32, device='cuda') for sc, _, _, _ in batches]
    ths = torch.from_numpy(DEFAULT_THRESHOLDS.astype(np.float32)).cuda()
    launches = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for (sc, tg, li, _), o in zip(batches, outs):
            if winpr:
                ops.winpr_sweep(sc, tg, li, ths, o)
            else:
                ops.threshold_sweep(sc, tg, li, ths, o)
        b.record()
        torch.cuda.synchronize()
        launches.append(a.elapsed_time(b))
    launches.sort()
    return tab, wall, launches


def _stats(wall, reps):
    return {'median': statistics.median(wall), 'min': wall[0], 'p90': wall[int(0.9 * len(wall)) - 1], 'max': wall[-1], 'reps': reps}


def winpr_host(tags, target):
    """metrics.WinPR as test_step calls it, on integer lists; the sweep's zeros where it divides by zero"""
    try:
        return [float(v) for v in metrics.WinPR([int(v) for v in tags], [int(v == 1) for v in target])]
    except ZeroDivisionError:
        return [0.0, 0.0, 0.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--metric', choices=['Pk', 'scaiano'], default='Pk')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('threshold_sweep_bench: needs the GPU (a CPU run says nothing about it)')
    lengths, batches = workload()
    winpr = args.metric == 'scaiano'
    tab, wall, launches = time_device(batches, args.reps, 'scaiano' if winpr else None)
    if winpr:
        _, pk_wall, pk_launches = time_device(batches, args.reps)

    decoded = []
    for sc, tg, li, ls in batches:
        tags = torch.empty(sc.shape[0], sc.shape[1], dtype=torch.uint8, device='cuda')
        per_th = []
        for th in DEFAULT_THRESHOLDS:
            ops.greedy_decode(sc, li, float(th), tags)
            per_th.append(tags.cpu().numpy())
        decoded.append((per_th, tg.cpu().numpy(), ls))
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        acc = np.zeros((len(DEFAULT_THRESHOLDS), 3))
        for per_th, tgt, ls in decoded:
            for b, n in enumerate(ls):
                one = winpr_host if winpr else host_metrics
                acc = acc + np.array([one(per_th[j][b, :n], tgt[b, :n]) for j in range(len(DEFAULT_THRESHOLDS))])
        acc = acc / DOCS
        host.append(time.perf_counter() - t0)
    keys = ('b_precision', 'b_recall', 'b_f1') if winpr else ('Pk_loss', 'WD_loss', 'F1_loss')
    equal = all(list(tab[k]) == list(acc[:, c]) for c, k in enumerate(keys))
    res = {'metric': args.metric, 'docs': DOCS, 'sentences': int(lengths.sum()), 'median_length': int(np.median(lengths)),
           'thresholds': len(DEFAULT_THRESHOLDS), 'device_wall_ms': _stats(wall, args.reps),
           'launches_ms': {'median': statistics.median(launches), 'min': launches[0], 'max': launches[-1]},
           'host_loop_s': sorted(host), 'tables_equal': equal}
    if winpr:
        res['pk_yardstick'] = {'device_wall_ms': _stats(pk_wall, args.reps),
                               'launches_ms': {'median': statistics.median(pk_launches), 'min': pk_launches[0], 'max': pk_launches[-1]}}
    print(json.dumps(res))
    if not equal:
        raise SystemExit('threshold_sweep_bench: the device table differs from the host loop')


if __name__ == '__main__':
    main()
