#!/usr/bin/env python3
"""Cost of the test pass and of the bootstrap behind it (evaluate.py; DESIGN.md "Test pass and bootstrap intervals").

Workload: 55 synthetic documents, lengths drawn by a fixed seed from the RadioNews statistics of SURVEY §5 (84 .. 2 437 sentences,
log-normal around the median 359, the two extremes present; the lengths of tools/threshold_sweep_bench.py), 768-wide embeddings in a
ResidentCorpus, a one-layer BiLSTM tagger (hidden 256) inside a TextSegmenter.  In ONE process, warmed, wall clock, medians:

  (a) ``evaluate(model, corpus, batch_size=8)`` and ``batch_size=1`` against ``TextSegmenter.test_step`` at batch size 1 over the same
      documents and model (``corpus.batch([i])`` inside the timed region on both sides), metric 'Pk' and metric 'scaiano' -- test_step
      reports one family per call, evaluate both;
  (b) ``bootstrap_ci`` of the six per-document metrics x 10 000 samples (host table in, host intervals out: upload, launch, copy, percentiles)
      against the reference's expression -- a loop of 10 000 resample-and-mean calls (train_fit.py:540-562), numpy standing in for pandas
      -- and against one vectorised numpy draw of all 10 000 x n indices.

The means of (a) are compared for equality where they are equal by construction (Pk, WD, F1).  Prints one JSON line.

  python tools/evaluate_bench.py [--reps 5]
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
from multimodaltopicsegmentation_amd import AudioPortionDataset, ResidentCorpus, TextSegmenter, bootstrap_ci, evaluate  # noqa: E402

DOCS, D, HIDDEN, SAMPLES = 55, 768, 256, 10000


def workload():
    rng = np.random.default_rng(55)
    lengths = np.clip(np.round(np.exp(rng.normal(np.log(359.0), 0.75, size=DOCS))), 84, 2437).astype(int)
    lengths[0], lengths[1] = 2437, 84
    g = torch.Generator().manual_seed(55)
    lines = [(torch.randn(int(n), D, generator=g), (torch.rand(int(n), generator=g) < 0.05).float().tolist(), f'doc{k}.wav')
             for k, n in enumerate(lengths)]
    return lengths, ResidentCorpus(AudioPortionDataset(lines, {}, CRF=False, truncate=False), 'cuda')


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return res, {'median_s': statistics.median(out), 'min_s': min(out), 'max_s': max(out), 'reps': reps}


def test_pass(ts, corpus, metric):
    """the product's own hook, one document per call; the mean over documents of its per-call results"""
    ts.metric = metric
    rows = [ts.test_step(corpus.batch([i]), i) for i in range(len(corpus))]
    return {k: sum(float(r[k]) for r in rows) / len(rows) for k in rows[0]}


def numpy_loop(values, rng):
    n = values.shape[1]
    means = np.empty((values.shape[0], SAMPLES))
    for s in range(SAMPLES):
        means[:, s] = values[:, rng.integers(0, n, n)].mean(axis=1)
    return np.percentile(means, 2.5, axis=1), np.percentile(means, 97.5, axis=1)


def numpy_vectorised(values, rng):
    n = values.shape[1]
    means = values[:, rng.integers(0, n, (SAMPLES, n))].mean(axis=2)
    return np.percentile(means, 2.5, axis=1), np.percentile(means, 97.5, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('evaluate_bench: needs the GPU (a CPU run says nothing about it)')
    lengths, corpus = workload()
    torch.manual_seed(3)
    ts = TextSegmenter(2, D, HIDDEN, architecture='BiLSTM', loss_fn='FocalLoss', threshold=0.5, metric='Pk').cuda().eval()
    ev8, t_ev8 = timed(lambda: evaluate(ts, corpus, batch_size=8, threshold=0.5), args.reps)
    ev1, t_ev1 = timed(lambda: evaluate(ts, corpus, batch_size=1, threshold=0.5), args.reps)
    pk, t_pk = timed(lambda: test_pass(ts, corpus, 'Pk'), max(1, args.reps // 2))
    try:
        _, t_sc = timed(lambda: test_pass(ts, corpus, 'scaiano'), max(1, args.reps // 2))
    except ZeroDivisionError:                               # metrics.WinPR on a document without a common boundary window
        t_sc = None
    # batch size 1 pads nothing, so the per-document integers are those of test_step's calls; the mean of its per-call values is summed here
    # as evaluate sums (one document after the other)
    equal = (ev1['mean']['Pk'], ev1['mean']['WD'], ev1['mean']['F1']) == (pk['test_loss'], pk['WD_loss'], pk['F1_loss'])
    table = np.stack([ev8['per_document'][k] for k in ev8['per_document']])
    ci, t_ci = timed(lambda: bootstrap_ci(table, samples=SAMPLES, seed=0), args.reps)
    rng = np.random.default_rng(0)
    _, t_loop = timed(lambda: numpy_loop(table, rng), max(1, args.reps // 2))
    (vlo, vhi), t_vec = timed(lambda: numpy_vectorised(table, rng), args.reps)
    res = {'docs': DOCS, 'sentences': int(lengths.sum()), 'median_length': int(np.median(lengths)), 'embedding': D, 'hidden': HIDDEN,
           'evaluate_batch8': t_ev8, 'evaluate_batch1': t_ev1, 'test_step_batch1_pk': t_pk, 'test_step_batch1_scaiano': t_sc,
           'means_equal_test_step': equal, 'bootstrap_samples': SAMPLES, 'metrics': int(table.shape[0]), 'bootstrap_ci': t_ci,
           'numpy_loop': t_loop, 'numpy_vectorised': t_vec,
           'half_width_kernel': ((ci['hi'] - ci['lo']) / 2).tolist(), 'half_width_numpy': ((vhi - vlo) / 2).tolist()}
    print(json.dumps(res))
    if not equal:
        raise SystemExit('evaluate_bench: evaluate at batch size 1 and test_step disagree on Pk / WD / F1')


if __name__ == '__main__':
    main()
