#!/usr/bin/env python3
"""Time the domain-switched head kernels (csrc/switch_head.hip) against the unswitched head kernels, and the SwitchBiLSTM training step
against BiLSTM.

  * mts_switch_head_fwd / _bwd_params / _bwd_data against mts_head_fwd / _bwd_params / _bwd_data at 64 x 256, D = 512, n_out = 1, bf16
    and fp32, identity maps (a single-domain batch: every document reads its own rows through head 0), the two alternating in one
    process; a mixed batch (alternating domains) is timed next to them.  Algorithmic bytes (N = B L rows, element size e):
    forward N D e + 4 N, params N D e + 4 N, data N D e + 4 N;
  * one fwd + bwd + Adam step (NativeTrainer) of SwitchBiLSTM(1792, 256, 2, dense) at 64 x 256, bf16 and fp32, against
    BiLSTM(1792, 256, 2, FocalLoss) in the same process, the two alternating; single-domain and mixed batches.
Prints one line per measurement (median of 5 repetitions of back-to-back calls)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import ops  # noqa: E402
from multimodaltopicsegmentation_amd.rnn_taggers import BiLSTM, SwitchBiLSTM  # noqa: E402
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


def kernels(B=64, Lq=256, D=512, n_out=1, dtype=torch.bfloat16):
    N = B * Lq
    es = 2 if dtype == torch.bfloat16 else 4
    g = torch.Generator(device=DEV).manual_seed(1)
    x = (torch.randn(N, D, device=DEV, generator=g) * 0.5).to(dtype)
    w = torch.randn(2, n_out, D, device=DEV, generator=g) * 0.1
    b = torch.randn(2, n_out, device=DEV, generator=g)
    ds = torch.randn(B, Lq, n_out, device=DEV, generator=g)
    scores = torch.empty(N, n_out, device=DEV)
    dw, db = torch.empty(2, n_out, D, device=DEV), torch.empty(2, n_out, device=DEV)
    dx = torch.empty(N, D, dtype=dtype, device=DEV)
    same, mixed = [1] * B, [i & 1 for i in range(B)]
    nbytes = N * D * es + 4 * N
    label = f'{B} x {Lq}, D {D}, n_out {n_out}, {"bf16" if es == 2 else "fp32"}'
    trio = {
        'fwd': (lambda: ops.head_fwd(x, w[0], b[0], scores),
                lambda: ops.switch_head_fwd(x, w, b, same, B, Lq, scores), lambda: ops.switch_head_fwd(x, w, b, mixed, B, Lq, scores)),
        'bwd_params': (lambda: ops.head_bwd_params(x, ds.view(N, n_out), dw[0], db[0]),
                       lambda: ops.switch_head_bwd_params(x, ds, same, B, Lq, dw, db), lambda: ops.switch_head_bwd_params(x, ds, mixed, B, Lq, dw, db)),
        'bwd_data': (lambda: ops.head_bwd_data(ds.view(N, n_out), w[0], dx),
                     lambda: ops.switch_head_bwd_data(ds, w, same, B, Lq, dx), lambda: ops.switch_head_bwd_data(ds, w, mixed, B, Lq, dx)),
    }
    for name, fns in trio.items():
        rounds = [[timed(fn, inner=50) for fn in fns] for _ in range(3)]  # the three alternate: a drift of the box hits all of them
        plain, ident, mix = (sorted(r[i] for r in rounds)[1] for i in range(3))
        print(f'{name} {label}: mts_head_{name} {plain:7.1f} us ({nbytes / (plain * 1e-6) / HBM * 100:4.1f} % of 6.3 TB/s)   '
              f'mts_switch_head_{name} identity {ident:7.1f} us ({ident / plain:.3f}x, {nbytes / (ident * 1e-6) / HBM * 100:4.1f} %)   '
              f'mixed {mix:7.1f} us ({mix / plain:.3f}x)')


def steps(B=64, Lq=256, D=1792, H=256, NL=2):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, Lq, D, generator=g).to(DEV)
    y = (torch.rand(B, Lq, generator=g) < 0.05).float().to(DEV)
    y[:, -1] = 0
    lengths = torch.full((B,), Lq, dtype=torch.int64)
    for dt in ('bf16', 'fp32'):
        for what, doms in (('single-domain', [1] * B), ('mixed', [i & 1 for i in range(B)])):
            batch = {'src_tokens': x, 'src_lengths': lengths, 'tgt_tokens': y, 'domain': doms}
            models = (('BiLSTM', BiLSTM(2, D, H, num_layers=NL, loss_fn='FocalLoss', compute_dtype=dt, seed=3)),
                      ('SwitchBiLSTM', SwitchBiLSTM(2, D, H, num_layers=NL, loss_fn='FocalLoss', switch_dense_adapt=True, compute_dtype=dt, seed=3)))
            trainers = {name: NativeTrainer(m.to(DEV), lr=1e-4, optimizer='Adam') for name, m in models}
            out = {name: [] for name in trainers}
            for _ in range(3):                                           # the two alternate: a drift of the box hits both
                for name, tr in trainers.items():
                    out[name].append(timed(lambda: tr.step(batch), reps=3, inner=10))
            med = {name: sorted(v)[1] for name, v in out.items()}
            for name in trainers:
                print(f'training step {dt} {what} {B} x {Lq} x {D}, H {H}, NL {NL}, {name}: {med[name] / 1e3:7.3f} ms   '
                      f'(rounds: {", ".join(f"{v / 1e3:.3f}" for v in out[name])})')
            print(f'SwitchBiLSTM(dense) - BiLSTM step, {dt} {what}: {(med["SwitchBiLSTM"] - med["BiLSTM"]):+.1f} us '
                  f'({med["SwitchBiLSTM"] / med["BiLSTM"]:.3f}x)')


if __name__ == '__main__':
    if '--step-only' not in sys.argv:
        kernels(dtype=torch.bfloat16)
        kernels(dtype=torch.float32)
    steps()
