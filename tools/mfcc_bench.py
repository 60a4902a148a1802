#!/usr/bin/env python3
"""What on-device MFCC sentence features cost (audio.py, csrc/mfcc.hip; DESIGN.md "MFCC sentence features from resident waveforms") next
to the host route a user had before it.  One process, every leg warmed, REPS repetitions, each repetition reported.

The corpus is seeded and synthetic: 55 documents, about 30 000 sentences of 2 .. 10 s at 16 kHz that tile their document without gaps
(about 2.9 G samples, 11.5 GB in fp32; --sentences scales it).  A document's waveform is a seeded 60 s block of modulated noise plus two
tones, repeated: no leg can tell.

(a) ``ops.mel_frames`` and ``ops.mfcc_frames`` between device events: ms, frames/s, and the bytes of waveform the first needs -- every
    sample ONCE -- per second as a share of the 6.3 TB/s a streaming kernel reaches on this card (the 4-fold overlap of the frames is
    the kernel's own cost and L2's to serve, not counted);
(b) ``audio.mfcc()`` and ``audio.mfcc_stats()`` end to end: a host clock round work that ends in a device synchronise (tables cached,
    allocations, the finiteness check of the adopted frames, the pooling launch);
(c) the host route: the NumPy restatement of tests/mfcc_oracle.py in fp32 on --host-sentences sentences, scaled up to the corpus by
    samples (--host-sentences 0 skips it).

  python tools/mfcc_bench.py [--out profiles/mfcc_bench.json] [--reps 3] [--sentences 30000] [--host-sentences 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import ResidentAudio, ops  # noqa: E402

DEV = 'cuda'
SR, N_DOCS, HOP = 16000, 55, 512
STREAM_TBS = 6.3


def make_corpus(n_sent, seed=0):
    """-> (waves, spans in samples): sentences of 2 .. 10 s, each document the run of its sentences"""
    g = np.random.default_rng([61, seed])
    t = np.arange(60 * SR) / SR
    block = (0.3 * g.standard_normal(t.size) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.2 * np.sin(2 * np.pi * 220.0 * t)
             + 0.1 * np.sin(2 * np.pi * 1870.0 * t)).astype(np.float32)
    lens = g.integers(2 * SR, 10 * SR + 1, size=n_sent)
    cut = np.rint(np.linspace(0, n_sent, N_DOCS + 1)).astype(np.int64)
    waves, spans = [], []
    for a, b in zip(cut[:-1], cut[1:]):
        ends = np.cumsum(lens[a:b])
        waves.append(np.resize(block, int(ends[-1])))
        spans.append(list(zip((ends - lens[a:b]).tolist(), ends.tolist())))
    return waves, spans


def device_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


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
    ap.add_argument('--sentences', type=int, default=30000)
    ap.add_argument('--host-sentences', type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mfcc_bench: no GPU visible; nothing is measured on the CPU')
    waves, spans = make_corpus(a.sentences)
    t, audio = host_time(lambda: ResidentAudio(waves, spans, DEV, unit='samples'))
    report = {'device': torch.cuda.get_device_name(0), 'documents': N_DOCS, 'sentences': audio.total_sentences, 'samples': audio.total_samples,
              'hours of audio': audio.total_samples / SR / 3600, 'frames': audio.total_frames, 'waveform GB': audio.total_samples * 4 / 1e9,
              'upload ms (concatenate, copy, finiteness check)': t}
    tabs = audio._tables(50, 128, 2048)
    start = np.zeros(audio.total_sentences + 1, dtype=np.int64)
    np.cumsum(audio.frame_counts, out=start[1:])
    fs = torch.from_numpy(start).to(DEV)
    mel = torch.empty((audio.total_frames, 128), device=DEV)
    out = torch.empty((audio.total_frames, 100), device=DEV)

    def run_mel():
        return ops.mel_frames(audio.wave, audio.sent_start, audio.sent_len, fs, audio.total_frames, tabs['window'], tabs['twiddle'], tabs['mel_first'],
                              tabs['mel_ptr'], tabs['mel_w'], HOP, mel=mel)

    run_mel()                                                                            # warm every leg
    ops.mfcc_frames(mel, fs, tabs['dct'], out)
    del out
    audio.mfcc_stats()
    torch.cuda.synchronize()
    legs = {'mel_frames ms': [], 'mfcc_frames ms': [], 'audio.mfcc() ms': [], 'audio.mfcc_stats() ms': []}
    for _ in range(a.reps):                                                              # the legs in turn
        legs['mel_frames ms'].append(device_time(run_mel)[0])
        o = torch.empty((audio.total_frames, 100), device=DEV)
        legs['mfcc_frames ms'].append(device_time(lambda: ops.mfcc_frames(mel, fs, tabs['dct'], o))[0])
        del o
        legs['audio.mfcc() ms'].append(host_time(lambda: audio.mfcc().total_frames)[0])
        legs['audio.mfcc_stats() ms'].append(host_time(lambda: tuple(audio.mfcc_stats().shape))[0])
    report.update(legs)
    report['frames/s (mel_frames + mfcc_frames kernels)'] = [audio.total_frames / ((x + y) * 1e-3) for x, y in
                                                             zip(legs['mel_frames ms'], legs['mfcc_frames ms'])]
    report['x real time (audio.mfcc_stats())'] = [audio.total_samples / SR / (x * 1e-3) for x in legs['audio.mfcc_stats() ms']]
    tbs = [audio.total_samples * 4 / (x * 1e-3) / 1e12 for x in legs['mel_frames ms']]
    report['mel_frames: waveform bytes read once per second'] = {'TB/s': tbs, 'share of 6.3 TB/s': [x / STREAM_TBS for x in tbs]}
    if a.host_sentences > 0:
        from tests import mfcc_oracle as O
        pick = np.random.default_rng(7).choice(audio.total_sentences, size=min(a.host_sentences, audio.total_sentences), replace=False)
        flat = [w[s:e] for w, doc in zip(waves, spans) for s, e in doc]
        t = time.perf_counter()
        for i in pick.tolist():
            O.stats(O.mfcc_frames(flat[i], np.float32)[1])
        sec = time.perf_counter() - t
        n = int(sum(flat[i].shape[0] for i in pick.tolist()))
        report['host route (NumPy restatement, fp32; threads %s)' % os.environ.get('OMP_NUM_THREADS', 'unset')] = {
            'sentences': int(pick.size), 'samples': n, 'seconds': sec, 'seconds scaled to the corpus by samples': sec * audio.total_samples / n}
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
