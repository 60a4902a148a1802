#!/usr/bin/env python3
"""What on-device wav2vec 2.0 sentence features cost (audio.py, wav2vec2.py, csrc/wav2vec2.hip; DESIGN.md "wav2vec 2.0 sentence
features") next to the host route a user had before.  One process, random weights at the base size (12 layers, hidden 768, conv 512 x 7),
synthetic sentences of 2 .. 10 s; every leg warmed, the legs of a repetition run one after another (interleaved), median and spread
(min .. max) over --reps repetitions.

(a) ``audio.wav2vec2()`` end to end per dtype: a host clock round work that ends in a device synchronise;
(b) one chunk per stage between device events: layer 0 (statistics + recompute), the six conv GEMMs, projection, positional convolution,
    the 12 transformer layers;
(c) the positional convolution, ``mts_w2v_pos_conv`` against its GEMM form (regroup + 16 GEMMs + rows) on the same chunk, interleaved;
(d) the host route: ``transformers``' ``Wav2Vec2Model`` on the CPU at batch size 1 for --host-sentences sentences, SCALED to the corpus by
    samples (only where ``transformers`` imports; --host-sentences 0 skips it).

FLOP counts are the multiply-adds of the matrices times two: per frame 2 * K_p * (H / G) * H for the positional convolution; per layer-l
row 2 * k * C * C for a conv GEMM; per frame and layer 2 * (4 H^2 + 2 H I) plus 4 * H * T for attention.  Shares are of the 2500 TFLOP/s
bf16 MFMA peak the project's roofline uses.

  python tools/wav2vec2_bench.py [--out profiles/wav2vec2_bench.json] [--reps 5] [--sentences 64] [--host-sentences 4]
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
from multimodaltopicsegmentation_amd import ResidentAudio, Wav2Vec2Weights  # noqa: E402
from multimodaltopicsegmentation_amd import wav2vec2 as W  # noqa: E402

DEV = 'cuda'
SR = 16000
PEAK_TFLOPS = 2500.0
BASE = dict(conv_dim=512, kernels=(10, 3, 3, 3, 3, 2, 2), strides=(5, 2, 2, 2, 2, 2, 2), hidden=768, heads=12, intermediate=3072, layers=12,
            pos_kernel=128, pos_groups=16, eps=1e-5)


def make_corpus(n_sent, seed=0, n_docs=4):
    g = np.random.default_rng([62, seed])
    lens = g.integers(2 * SR, 10 * SR + 1, size=n_sent)
    cut = np.rint(np.linspace(0, n_sent, n_docs + 1)).astype(np.int64)
    waves, spans = [], []
    for a, b in zip(cut[:-1], cut[1:]):
        ends = np.cumsum(lens[a:b])
        t = np.arange(int(ends[-1])) / SR
        waves.append((0.3 * g.standard_normal(t.size) + 0.2 * np.sin(2 * np.pi * 220.0 * t)).astype(np.float32))
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


def summary(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs), 'all': xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sentences', type=int, default=64)
    ap.add_argument('--host-sentences', type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('wav2vec2_bench: no GPU visible; nothing is measured on the CPU')
    from tests import wav2vec2_oracle as WO
    sd = WO.random_state_dict(BASE, 1)
    cfg = WO.hf_config_dict(BASE)
    waves, spans = make_corpus(a.sentences)
    audio = ResidentAudio(waves, spans, DEV, unit='samples', min_samples=400)
    seconds = audio.total_samples / SR
    report = {'device': torch.cuda.get_device_name(0), 'sentences': audio.total_sentences, 'seconds of audio': seconds, 'reps': a.reps,
              'peak TFLOP/s (bf16 MFMA, the roofline\'s)': PEAK_TFLOPS}
    C, H, I, Kp, G, L = BASE['conv_dim'], BASE['hidden'], BASE['intermediate'], BASE['pos_kernel'], BASE['pos_groups'], BASE['layers']
    weights = {d: Wav2Vec2Weights.from_state_dict(sd, cfg, device=DEV, dtype=d) for d in ('bf16', 'fp32')}
    plan = W.ChunkPlan(audio.sample_counts, weights['bf16'], audio.device)
    frames = plan.total_frames
    flops = {'conv GEMMs': float(sum(2 * k * C * C * int(plan.T[l].sum()) for l, k in enumerate(BASE['kernels']) if l)),
             'pos conv': 2.0 * Kp * (H // G) * H * frames,
             'transformer': float(L * (2 * (4 * H * H + 2 * H * I) * frames + 4 * H * int((plan.frames.astype(np.float64) ** 2).sum())))}
    flops['whole pass'] = sum(flops.values()) + 2.0 * C * H * frames + 2.0 * 10 * C * int(plan.T[0].sum()) * 2
    report.update({'frames': frames, 'GFLOP': {k: v / 1e9 for k, v in flops.items()}})

    # (a) end to end
    for d in ('bf16', 'fp32'):
        audio.wav2vec2(weights[d])
    e2e = {'bf16': [], 'fp32': []}
    for _ in range(a.reps):
        for d in ('bf16', 'fp32'):
            e2e[d].append(host_time(lambda: audio.wav2vec2(weights[d]).total_frames)[0])
    report['audio.wav2vec2() ms'] = {d: summary(v) for d, v in e2e.items()}
    med = statistics.median(e2e['bf16'])
    report['bf16: x real time'] = seconds / (med * 1e-3)
    report['bf16: whole pass TFLOP/s and share of peak'] = [flops['whole pass'] / (med * 1e-3) / 1e12, flops['whole pass'] / (med * 1e-3) / 1e12 / PEAK_TFLOPS]

    # (b), (c) one chunk per stage, bf16
    w = weights['bf16']
    wave, ss, sl = audio.wave, audio.sent_start, audio.sent_len
    x0 = torch.empty((plan.rows0 + W.SLACK, C), dtype=w.dtype, device=DEV)
    bufs = W.conv_features(w, wave, ss, sl, plan, keep=True)
    top = bufs[-1]
    h = W.project(w, top, plan)
    y = W.pos_conv_kernel(w, h, plan)
    W.pos_conv_gemm(w, h, plan)
    W.transformer(w, y, plan)
    torch.cuda.synchronize()

    def conv_gemms():
        rows, x = plan.rows0, bufs[0]
        for l in range(1, plan.n_layers):
            x = W.conv_gemm(w, l, x, rows, out=bufs[l])
            rows //= 2

    legs = {'conv layer 0 (statistics + recompute)': lambda: W.conv_layer0(w, wave, ss, sl, plan, out=x0),
            'six conv GEMMs': conv_gemms,
            'projection (LayerNorm + GEMM)': lambda: W.project(w, top, plan),
            'pos conv: mts_w2v_pos_conv': lambda: W.pos_conv_kernel(w, h, plan),
            'pos conv: regroup + 16 GEMMs + rows': lambda: W.pos_conv_gemm(w, h, plan),
            '12 transformer layers': lambda: W.transformer(w, y, plan)}
    times = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            times[k].append(device_time(fn)[0])
    report['stages, bf16, ms'] = {k: summary(v) for k, v in times.items()}
    m = {k: statistics.median(v) for k, v in times.items()}
    tf = lambda f, ms: [f / (ms * 1e-3) / 1e12, f / (ms * 1e-3) / 1e12 / PEAK_TFLOPS]
    report['TFLOP/s and share of peak'] = {'six conv GEMMs': tf(flops['conv GEMMs'], m['six conv GEMMs']),
                                           'pos conv: mts_w2v_pos_conv': tf(flops['pos conv'], m['pos conv: mts_w2v_pos_conv']),
                                           'pos conv: regroup + 16 GEMMs + rows': tf(flops['pos conv'], m['pos conv: regroup + 16 GEMMs + rows']),
                                           '12 transformer layers': tf(flops['transformer'], m['12 transformer layers'])}
    report['pos conv: kernel median / GEMM-form median'] = m['pos conv: mts_w2v_pos_conv'] / m['pos conv: regroup + 16 GEMMs + rows']

    # (d) the host route
    if a.host_sentences > 0:
        try:
            import transformers as tr
        except Exception:  # noqa: BLE001
            tr = None
        if tr is not None:
            hc = tr.Wav2Vec2Config(mask_time_prob=0.0, layerdrop=0.0)
            model = tr.Wav2Vec2Model(hc).eval()
            flat = [torch.from_numpy(wv[s:e]) for wv, doc in zip(waves, spans) for s, e in doc]
            pick = np.random.default_rng(7).choice(len(flat), size=min(a.host_sentences, len(flat)), replace=False).tolist()
            with torch.no_grad():
                model(flat[pick[0]][None][:, :SR])
                t = time.perf_counter()
                for i in pick:
                    x = flat[i]
                    model(((x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7))[None])
                sec = time.perf_counter() - t
            n = int(sum(flat[i].shape[0] for i in pick))
            report['host route (transformers %s Wav2Vec2Model, CPU fp32, batch 1; threads %s)' % (tr.__version__, torch.get_num_threads())] = {
                'sentences': len(pick), 'samples': n, 'seconds': sec, 'seconds SCALED to the corpus by samples': sec * audio.total_samples / n,
                'x real time': n / SR / sec}
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
