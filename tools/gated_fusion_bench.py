#!/usr/bin/env python3
"""What the gated late-fusion merge costs (BiLSTMLateFusion(merge='gate'), csrc/gate_merge.hip; DESIGN.md §3 "Gated late-fusion merge").
One process, every leg warmed, the legs taken IN TURN so that a drift of the machine hits all of them; REPS repetitions, the report
gives each repetition, the median and the spread.

(a) NativeTrainer.step (forward + backward + fused Adam, bf16) of BASELINE configs[4]'s per-GPU workload -- 64 documents x 512
    sentences, inputs 1024 + 768, H = 256, 2 layers, focal loss -- with merge='concat' and merge='gate', a host clock round windows of
    steps that end in a synchronise; ms per step of both and the difference.  One step of each mode is also taken under ops.KernelTimer:
    the sequence of kernel labels is reported (the concat one is the evidence that the default path issues what it issued before).
(b) the two merge kernels alone at that step's operands (rows = 32768, W = 512, bf16), every call between two device events, next to
    the repository's own dropout kernel (mts_dropout_fwd without a mask: read n, write n) at the SAME byte volume -- 4 rows W 2 bytes
    for the forward, 7 rows W 2 for the backward -- and next to a device copy of that volume.  Rate = compulsory bytes / time.

  python tools/gated_fusion_bench.py [--out profiles/gated_fusion_bench.json] [--steps 150] [--warmup 15] [--reps 3] [--iters 200]

--kernels-only runs (b) alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/gated_fusion_bench.py --kernels-only).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import ops  # noqa: E402
from multimodaltopicsegmentation_amd.rnn_taggers import BiLSTMLateFusion  # noqa: E402
from multimodaltopicsegmentation_amd.trainer import NativeTrainer  # noqa: E402

B, L, D1, D2, H, NL = 64, 512, 1024, 768, 256, 2
DEV = 'cuda'
HBM_PEAK_TBPS = 8.0          # spec; a float4 copy measures 6.29 TB/s on this part


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _batch():
    g = torch.Generator().manual_seed(4321)
    x1, x2 = torch.randn(B, L, D1, generator=g), torch.randn(B, L, D2, generator=g)
    y = (torch.rand(B, L, generator=g) < 0.05).float()
    return {'src_tokens': x1.to(DEV), 'src_tokens2': x2.to(DEV), 'src_lengths': torch.full((B,), L, dtype=torch.int64), 'tgt_tokens': y.to(DEV)}


def _labels(trainer, batch):
    """the kernel labels of one step, in issue order (ops.KernelTimer brackets every labelled launch)"""
    seq = []

    class Recorder(ops.KernelTimer):
        def begin(self, tag):
            seq.append('/'.join(str(t) for t in tag))
            return None
    ops.TIMER = Recorder()
    try:
        trainer.step(batch)
    finally:
        ops.TIMER = None
    torch.cuda.synchronize()
    return seq


def step_legs(steps, warmup, reps, say):
    batch = _batch()
    trainers = {m: NativeTrainer(BiLSTMLateFusion(2, [D1, D2], H, num_layers=NL, loss_fn='FocalLoss', compute_dtype='bf16', seed=1234, merge=m).to(DEV),
                                 lr=1e-3, optimizer='Adam') for m in ('concat', 'gate')}
    ms = {m: [] for m in trainers}
    for _ in range(reps):
        for m, tr in trainers.items():
            for _ in range(warmup):
                tr.step(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(batch)
            torch.cuda.synchronize()
            ms[m].append(1e3 * (time.perf_counter() - t0) / steps)
    say(f'(a) NativeTrainer.step, late fusion {D1}+{D2} H={H} layers={NL} bf16 at {B} x {L}: ms per step over windows of {steps} steps '
        f'({warmup} warm-up steps each), the legs in turn, {reps} repetitions')
    for m in trainers:
        say(f'  merge={m:7s} ' + '  '.join(f'{t:.4f}' for t in ms[m]) + f'   median {median(ms[m]):.4f}  spread {max(ms[m]) - min(ms[m]):.4f}')
    diff = [a - b for a, b in zip(ms['gate'], ms['concat'])]
    say('  gate - concat per repetition: ' + '  '.join(f'{1e3 * d:+.1f} us' for d in diff) + f'   median {1e3 * median(diff):+.1f} us')
    labels = {m: _labels(tr, batch) for m, tr in trainers.items()}
    for m, seq in labels.items():
        say(f'  kernel labels of one step, merge={m} ({len(seq)}): ' + ' '.join(seq))
    return {'step_ms': {m: [round(t, 4) for t in v] for m, v in ms.items()}, 'median_ms': {m: round(median(v), 4) for m, v in ms.items()},
            'gate_minus_concat_us': [round(1e3 * d, 1) for d in diff], 'labels': labels}


def kernel_legs(iters, reps, say):
    rows, W = B * L, 2 * H
    g = torch.Generator().manual_seed(1)
    a, h1, h2, dm = ((torch.randn(rows, W, generator=g) * s).to(torch.bfloat16).to(DEV) for s in (2.0, 0.5, 0.5, 1.0))
    m, da, dh1, dh2 = (torch.empty(rows, W, dtype=torch.bfloat16, device=DEV) for _ in range(4))
    nb = {'fwd': 4 * rows * W * 2, 'bwd': 7 * rows * W * 2}
    # the yardsticks at the same byte volume: n elements read + n written = 4 n bytes in bf16
    n_f, n_b = nb['fwd'] // 4, nb['bwd'] // 4 // 4 * 4
    xf, yf = torch.randn(n_f, device=DEV).to(torch.bfloat16), torch.empty(n_f, dtype=torch.bfloat16, device=DEV)
    xb, yb = torch.randn(n_b, device=DEV).to(torch.bfloat16), torch.empty(n_b, dtype=torch.bfloat16, device=DEV)
    legs = {'mts_gate_merge_fwd': (lambda: ops.gate_merge_fwd(a, h1, h2, m), nb['fwd']),
            'mts_dropout_fwd, fwd volume': (lambda: ops.dropout_fwd(xf, yf, 0.1, 7), 4 * n_f),
            'device copy, fwd volume': (lambda: yf.copy_(xf), 4 * n_f),
            'mts_gate_merge_bwd': (lambda: ops.gate_merge_bwd(a, h1, h2, dm, da, dh1, dh2), nb['bwd']),
            'mts_dropout_fwd, bwd volume': (lambda: ops.dropout_fwd(xb, yb, 0.1, 7), 4 * n_b),
            'device copy, bwd volume': (lambda: yb.copy_(xb), 4 * n_b)}
    for _ in range(8):
        for f, _ in legs.values():
            f()
    torch.cuda.synchronize()
    out = {name: [] for name in legs}
    for _ in range(reps):
        ev = {name: [] for name in legs}
        for _ in range(iters):
            for name, (f, _) in legs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f()
                e.record()
                ev[name].append((s, e))
        torch.cuda.synchronize()
        for name in legs:
            out[name].append(median([s.elapsed_time(e) * 1e3 for s, e in ev[name]]))
    say(f'(b) one call between two device events, median of {iters} per repetition, the legs in turn; rows {rows}, W {W}, bf16')
    res = {}
    for name, us in out.items():
        nbytes = legs[name][1]
        rates = [nbytes / (t * 1e-6) / 1e12 for t in us]
        say(f'  {name:30s} {nbytes / 1e6:7.1f} MB   ' + '  '.join(f'{t:7.1f} us' for t in us) + '   ' + '  '.join(f'{r:5.2f}' for r in rates)
            + f' TB/s   ({100 * median(rates) / HBM_PEAK_TBPS:.0f} % of the {HBM_PEAK_TBPS:.0f} TB/s HBM peak)')
        res[name] = {'MB': round(nbytes / 1e6, 1), 'us': [round(t, 1) for t in us], 'TBps': [round(r, 3) for r in rates]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernels-only', action='store_true', help='leg (b) alone, e.g. under a kernel trace')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--steps', type=int, default=150)
    ap.add_argument('--warmup', type=int, default=15)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'gated_fusion_bench.json')
    if not torch.cuda.is_available():
        sys.exit('gated_fusion_bench: no GPU visible; nothing is measured without one')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f'tools/gated_fusion_bench.py {"--kernels-only " if a.kernels_only else ""}--iters {a.iters} --steps {a.steps} --warmup {a.warmup} '
        f'--reps {a.reps}   ({torch.cuda.get_device_name(0)})')
    res = {'device': torch.cuda.get_device_name(0), 'args': vars(a).copy()}
    if not a.kernels_only:
        res.update(step_legs(a.steps, a.warmup, a.reps, say))
    res['kernels'] = kernel_legs(a.iters, a.reps, say)
    res['report'] = lines
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
