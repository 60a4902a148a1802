#!/usr/bin/env python3
"""What on-device prosodic sentence features cost (audio.py, csrc/prosody.hip; DESIGN.md "Prosodic sentence features") next to the host
route.  One process, every leg warmed, REPS repetitions, each repetition reported.

The corpus is tools/mfcc_bench.py's: seeded and synthetic, 55 documents, about 30 000 sentences of 2 .. 10 s at 16 kHz (--sentences scales
it).

(a) the kernels between device events on ONE chunk of sentences, the unit ``audio.prosodic()`` works in (--chunk-sentences of them: their
    cmnd / shift / log-observations / backpointers are what the workspace budget bounds): ``ops.yin_frames``, ``ops.pyin_observe``,
    ``ops.pyin_viterbi``, ``ops.yin_pick``, and the mel / delta / pooling / statistics launches together: ms and frames/s;
(b) ``audio.pitch()``, ``audio.yin()`` and ``audio.prosodic()`` end to end over the whole corpus: a host clock round work that ends in a
    device synchronise (tables cached, the chunk loop, its allocations and its small uploads included);
(c) the host route: the NumPy restatement of tests/prosody_oracle.py in fp64 on --host-sentences sentences, scaled up to the corpus by
    samples (--host-sentences 0 skips it).

  python tools/prosody_bench.py [--out profiles/prosody_bench.json] [--reps 3] [--sentences 30000] [--chunk-sentences 600] [--host-sentences 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mfcc_bench import DEV, HOP, N_DOCS, SR, device_time, host_time, make_corpus  # noqa: E402
from multimodaltopicsegmentation_amd import ResidentAudio, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sentences', type=int, default=30000)
    ap.add_argument('--chunk-sentences', type=int, default=600)
    ap.add_argument('--host-sentences', type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('prosody_bench: no GPU visible; nothing is measured on the CPU')
    waves, spans = make_corpus(a.sentences)
    audio = ResidentAudio(waves, spans, DEV, unit='samples')
    report = {'device': torch.cuda.get_device_name(0), 'documents': N_DOCS, 'sentences': audio.total_sentences, 'samples': audio.total_samples,
              'hours of audio': audio.total_samples / SR / 3600, 'frames': audio.total_frames}
    # ---- (a) one chunk
    n = min(a.chunk_sentences, audio.total_sentences)
    tabs = audio._pitch_tables(70.0, 500.0)
    mt = audio._tables(1, 40, 2048)
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(audio.frame_counts[:n], out=start[1:])
    F = int(start[-1])
    fs = torch.from_numpy(start).to(DEV)
    first = torch.zeros(n, dtype=torch.uint8, device=DEV)
    first[0] = 1
    ss, sl = audio.sent_start[:n], audio.sent_len[:n]
    out = torch.empty((n, 167), device=DEV)

    def run_yin():
        return ops.yin_frames(audio.wave, ss, sl, fs, F, tabs['min_period'], tabs['max_period'])

    def run_rest(f0, vp, yf):
        mel = ops.mel_frames(audio.wave, ss, sl, fs, F, mt['window'], mt['twiddle'], mt['mel_first'], mt['mel_ptr'], mt['mel_w'], HOP)
        ops.frame_pool(mel, fs, out[:, 6:86], first='mean', with_std=True)
        ops.frame_pool(ops.frame_delta(mel, fs), fs, out[:, 86:166], first='mean', with_std=True)
        return ops.prosodic_stats(f0, vp, yf, fs, first, out, 166)

    cmnd, shift = run_yin()                                                              # warm every leg
    vp, logobs = ops.pyin_observe(cmnd, shift, tabs)
    _, f0, _ = ops.pyin_viterbi(logobs, fs, tabs)
    yf = ops.yin_pick(cmnd, shift, tabs['min_period'], SR)
    run_rest(f0, vp, yf)
    audio.prosodic()
    torch.cuda.synchronize()
    legs = {k: [] for k in ('yin_frames ms', 'pyin_observe ms', 'pyin_viterbi ms', 'yin_pick ms', 'mel + delta + pools + stats ms', 'audio.pitch() ms',
                            'audio.yin() ms', 'audio.prosodic() ms')}
    for _ in range(a.reps):                                                              # the legs in turn
        legs['yin_frames ms'].append(device_time(run_yin)[0])
        legs['pyin_observe ms'].append(device_time(lambda: ops.pyin_observe(cmnd, shift, tabs, voiced_prob=vp, logobs=logobs))[0])
        legs['pyin_viterbi ms'].append(device_time(lambda: ops.pyin_viterbi(logobs, fs, tabs))[0])
        legs['yin_pick ms'].append(device_time(lambda: ops.yin_pick(cmnd, shift, tabs['min_period'], SR, f0=yf))[0])
        legs['mel + delta + pools + stats ms'].append(device_time(lambda: run_rest(f0, vp, yf))[0])
        legs['audio.pitch() ms'].append(host_time(lambda: audio.pitch()[0].numel())[0])
        legs['audio.yin() ms'].append(host_time(lambda: audio.yin().numel())[0])
        legs['audio.prosodic() ms'].append(host_time(lambda: tuple(audio.prosodic().shape))[0])
    report['chunk'] = {'sentences': n, 'frames': F, 'workspace MB (cmnd, shift, log-observations, backpointers)':
                       F * (8 * tabs['n_lags'] + 20 * tabs['n_bins']) / 1e6}
    report.update(legs)
    report['chunk frames/s per kernel'] = {k[:-3]: [F / (x * 1e-3) for x in v] for k, v in legs.items() if not k.startswith('audio.')}
    report['x real time (audio.prosodic())'] = [audio.total_samples / SR / (x * 1e-3) for x in legs['audio.prosodic() ms']]
    report['Viterbi fp64 adds + compares per second (2 x 2 n_bins x 2 width per frame)'] = [
        F * 4.0 * 2 * tabs['n_bins'] * tabs['width'] / (x * 1e-3) for x in legs['pyin_viterbi ms']]
    if a.host_sentences > 0:
        from tests import prosody_oracle as PO
        pick = np.random.default_rng(7).choice(audio.total_sentences, size=min(a.host_sentences, audio.total_sentences), replace=False)
        flat = [w[s:e] for w, doc in zip(waves, spans) for s, e in doc]
        t = time.perf_counter()
        for i in pick.tolist():
            PO.prosodic_row(flat[i], flat[i - 1] if i else None)
        sec = time.perf_counter() - t
        m = int(sum(flat[i].shape[0] for i in pick.tolist()))
        report['host route (NumPy restatement, fp64, the previous sentence\'s YIN recomputed; threads %s)' % os.environ.get('OMP_NUM_THREADS', 'unset')] = {
            'sentences': int(pick.size), 'samples': m, 'seconds': sec, 'seconds scaled to the corpus by samples': sec * audio.total_samples / m}
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
