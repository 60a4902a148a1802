#!/usr/bin/env python3
"""Cost of the prediction pass and of the decode kernel behind it (predict.py; DESIGN.md "Prediction pass and minimum-length decode").

Workload (a): 55 synthetic documents, lengths drawn by a fixed seed from the RadioNews statistics of SURVEY §5 (the lengths of
tools/evaluate_bench.py: 84 .. 2 437 sentences, 33 179 in all), 768-wide embeddings in an UNLABELLED ResidentCorpus, a one-layer BiLSTM
tagger (hidden 256) inside a TextSegmenter.  In ONE process, warmed, wall clock, medians:

  ``predict(model, corpus, batch_size=8)`` at min_segment 1 and 5, against the host path it replaces -- per batch the tagger's own forward
  (scores, then python tag lists: one ``.tolist()`` per document) and ``metrics.get_boundaries`` per document, cumulated to segment ends.
  The segment ends of the two are compared for equality at min_segment 1.

Workload (b): the kernel alone on ONE document of 65 536 sentences (the longest the ABI takes), random scores, min_segment in
{1, 2, 64, 1024}: HIP events around 20 launches, the median.  min_segment = 2 is the worst case of the recurrence: 32 768 runs of two
positions walked by one wave, and the densest walk back.

Prints one JSON line.

  python tools/predict_bench.py [--reps 5]
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
from multimodaltopicsegmentation_amd import ResidentCorpus, TextSegmenter, ops, predict  # noqa: E402
from multimodaltopicsegmentation_amd.metrics import get_boundaries  # noqa: E402

DOCS, D, HIDDEN, LONG = 55, 768, 256, 65536


def workload():
    rng = np.random.default_rng(55)
    lengths = np.clip(np.round(np.exp(rng.normal(np.log(359.0), 0.75, size=DOCS))), 84, 2437).astype(int)
    lengths[0], lengths[1] = 2437, 84
    g = torch.Generator().manual_seed(55)
    return lengths, ResidentCorpus.from_documents([torch.randn(int(n), D, generator=g) for n in lengths], 'cuda',
                                                  names=[f'doc{k}.npy' for k in range(DOCS)])


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


def host_path(model, corpus, batch_size):
    """forward, tag lists, get_boundaries per document -> segment ends per document (the tail closed, as predict's close_last)"""
    ends = []
    for s in range(0, len(corpus), batch_size):
        batch = corpus.batch(list(range(s, min(s + batch_size, len(corpus)))))
        tags = model(batch['src_tokens'], batch['src_lengths'])[1]
        for t in tags:
            e = np.cumsum(get_boundaries(t)).tolist()
            if not t[-1]:
                e.append(len(t))
            ends.append(e)
    return ends


def kernel_alone(m, launches=20):
    g = torch.Generator().manual_seed(m)
    scores = torch.randn(1, LONG, 1, generator=g).cuda()
    seg_end = torch.empty((1, LONG), dtype=torch.int32, device='cuda')
    n_seg = torch.empty(1, dtype=torch.int32, device='cuda')
    tags = torch.empty((1, LONG), dtype=torch.uint8, device='cuda')
    ms = []
    for k in range(launches + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.segment_decode(scores, None, 0.5, seg_end, n_seg, min_segment=m, tags=tags)
        b.record()
        torch.cuda.synchronize()
        if k >= 2:
            ms.append(a.elapsed_time(b))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'segments': int(n_seg.item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('predict_bench: needs the GPU (a CPU run says nothing about it)')
    lengths, corpus = workload()
    torch.manual_seed(3)
    ts = TextSegmenter(2, D, HIDDEN, architecture='BiLSTM', loss_fn='FocalLoss', threshold=0.5, metric='Pk').cuda().eval()
    model = ts.model
    model.th = 0.5
    p1, t_p1 = timed(lambda: predict(model, corpus, batch_size=8, threshold=0.5), args.reps)
    p5, t_p5 = timed(lambda: predict(model, corpus, batch_size=8, threshold=0.5, min_segment=5), args.reps)
    host, t_host = timed(lambda: host_path(model, corpus, 8), args.reps)
    equal = [e.tolist() for e in p1.segment_ends] == host
    res = {'docs': DOCS, 'sentences': int(lengths.sum()), 'embedding': D, 'hidden': HIDDEN, 'predict_m1': t_p1, 'predict_m5': t_p5,
           'host_path': t_host, 'segments_m1': int(p1.n_segments.sum()), 'segments_m5': int(p5.n_segments.sum()),
           'segment_ends_equal_host_path': equal, 'kernel_65536': {str(m): kernel_alone(m) for m in (1, 2, 64, 1024)}}
    print(json.dumps(res))
    if not equal:
        raise SystemExit('predict_bench: predict at min_segment 1 and the host path disagree on the segment ends')


if __name__ == '__main__':
    main()
