#!/usr/bin/env python3
"""What on-device sentence pooling costs (frames.py, csrc/frame_pool.hip; DESIGN.md "Sentence pooling of frame-level features") next to the
host route a user had before it.  One process, every leg warmed, the legs taken in turn, REPS repetitions, each repetition reported.

The corpus is seeded and RadioNews-shaped: 55 documents, 33 179 sentences, frames per sentence from a seeded skewed (log-normal)
distribution cut to 1 .. 3000.  The default (width 512, median 42 frames) is about 3.9 GB in fp32; --width / --median-frames change it.

(a) every mode on the device between device events, for fp32 and for bf16 storage (output in the storage dtype).  For the four
    reductions the rate is computed from the bytes the algorithm needs -- the frames read ONCE plus the output written -- and given as a
    share of the 6.3 TB/s a streaming kernel reaches on this card; the re-read of the second pass is the kernel's own cost, not counted;
(b) the host route: the reference's NumPy expressions over the per-sentence list, plus the upload of the result (--host-reps, default 1:
    it takes seconds per mode);
(c) ``corpus.with_frames(frames, 'mean_std', 'append')`` end to end on a bf16 text corpus of width 768: a host clock round work that ends
    in a device synchronise.

  python tools/frame_pool_bench.py [--out profiles/frame_pool_bench.json] [--reps 3] [--width 512] [--median-frames 42]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import POOL_MODES, AudioPortionDataset, ResidentCorpus, ResidentFrames  # noqa: E402

DEV = 'cuda'
N_DOCS, N_SENT = 55, 33179
STREAM_TBS = 6.3


def corpus_shape(median_frames, seed=0):
    """-> (sentences per document [N_DOCS], frames per sentence [N_SENT])"""
    g = np.random.default_rng([53, seed])
    cut = np.rint(np.linspace(0, N_SENT, N_DOCS + 1)).astype(np.int64)
    cut[1:-1] += g.integers(-100, 101, size=N_DOCS - 1)
    counts = np.clip(np.rint(g.lognormal(np.log(median_frames), 0.8, size=N_SENT)), 1, 3000).astype(np.int64)
    return np.diff(cut), counts


def make_docs(sentences, counts, D, seed=0):
    """per-sentence matrices as VIEWS into one seeded block of 8192 frames (a sentence starts at a seeded offset): the values repeat
    between sentences, which no leg can tell, and the list costs no memory"""
    g = np.random.default_rng([59, seed])
    block = (g.standard_normal((8192, D)) * 0.3 + 2.0 * g.standard_normal(D)[None, :]).astype(np.float32)
    at = g.integers(0, 8192 - 3000, size=counts.size)
    flat = [block[a:a + n] for a, n in zip(at.tolist(), counts.tolist())]
    ends = np.cumsum(sentences)
    return [flat[a:b] for a, b in zip((ends - sentences).tolist(), ends.tolist())]


HOST = {
    'mean': lambda es: np.array([e.mean(axis=0) for e in es]),
    'max': lambda es: np.array([np.max(e, axis=0) for e in es]),
    'mean_std': lambda es: np.array([np.concatenate((e.mean(axis=0), np.std(e, axis=0))) for e in es]),
    'max_std': lambda es: np.array([np.concatenate((np.max(e, axis=0), np.std(e, axis=0))) for e in es]),
    'last': lambda es: np.array([e[-1] for e in es]),
}


def host_delta_gap(es):
    out = []
    for i, e in enumerate(es):
        out.append(es[i + 1][0] - e[-1] if i + 1 < len(es) else e[-1])
    return np.array(out)


def host_pool(docs, mode):
    fn = host_delta_gap if mode == 'delta_gap' else HOST[mode]
    return np.concatenate([fn(doc) for doc in docs])


def device_time(fn, inner=3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def host_time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=1)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--median-frames', type=float, default=42.0)
    ap.add_argument('--text-width', type=int, default=768)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('frame_pool_bench: no GPU visible; nothing is measured on the CPU')
    sentences, counts = corpus_shape(a.median_frames)
    docs = make_docs(sentences, counts, a.width)
    total = int(counts.sum())
    report = {'device': torch.cuda.get_device_name(0), 'documents': N_DOCS, 'sentences': N_SENT, 'width': a.width, 'frames': total,
              'frames per sentence': {'median': float(np.median(counts)), 'mean': float(counts.mean()), 'max': int(counts.max()),
                                      'share of sentences of at most 32 frames (read once)': float((counts <= 32).mean())},
              'fp32 GB': total * a.width * 4 / 1e9}
    t, f32 = host_time(lambda: ResidentFrames(docs, DEV, wire_dtype='fp32'))
    report['upload fp32 ms (concatenate, copy, finiteness check)'] = t
    frames = {'fp32': f32, 'bf16': ResidentFrames(docs, DEV, wire_dtype='bf16')}
    g = torch.Generator().manual_seed(1)
    lines = []
    for k, n in enumerate(sentences.tolist()):
        y = (torch.rand(n, generator=g) < 0.05).float()
        y[-1] = 0.0
        lines.append((torch.randn(n, a.text_width, generator=g), y.tolist(), f'doc{k}.wav'))
    corpus = ResidentCorpus(AudioPortionDataset(lines, {'O': 0, 'B': 1}, CRF=False, truncate=False), DEV, wire_dtype='bf16')
    outs = {(w, m): torch.empty((N_SENT, f.width(m)), dtype=f.wire, device=DEV) for w, f in frames.items() for m in POOL_MODES}

    device = {w: {m: [] for m in POOL_MODES} for w in frames}
    append = []
    for (w, m), o in outs.items():                                                      # warm every leg
        frames[w].pool(m, out=o)
    corpus.with_frames(frames['bf16'], 'mean_std', field='append')
    torch.cuda.synchronize()
    for _ in range(a.reps):                                                              # the legs in turn
        for (w, m), o in outs.items():
            device[w][m].append(device_time(lambda: frames[w].pool(m, out=o)))
        append.append(host_time(lambda: corpus.with_frames(frames['bf16'], 'mean_std', field='append'))[0])
    report['device ms'] = device
    rate = {}
    for w, f in frames.items():
        esize = f.frames.element_size()
        for m in ('mean', 'max', 'mean_std', 'max_std'):
            need = (total * a.width + N_SENT * f.width(m)) * esize
            tbs = [need / (t * 1e-3) / 1e12 for t in device[w][m]]
            rate[f'{w} {m}'] = {'bytes needed': need, 'TB/s': tbs, 'share of 6.3 TB/s': [x / STREAM_TBS for x in tbs]}
    report['reduce kernel rate (frames read once + output, over kernel time)'] = rate
    report["with_frames('mean_std', 'append') on a bf16 text corpus of width %d, bf16 frames: ms" % a.text_width] = append

    host = {m: {'pool ms': [], 'upload ms': []} for m in POOL_MODES}
    for _ in range(a.host_reps):
        for m in POOL_MODES:
            t = time.perf_counter()
            y = host_pool(docs, m)
            host[m]['pool ms'].append((time.perf_counter() - t) * 1e3)
            yt = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
            host[m]['upload ms'].append(host_time(lambda: yt.to(DEV))[0])
    report['host route (NumPy per sentence, fp32; threads %s)' % os.environ.get('OMP_NUM_THREADS', 'unset')] = host
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
