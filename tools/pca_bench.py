#!/usr/bin/env python3
"""What the on-device PCA projection costs (pca.py, csrc/pca.hip; DESIGN.md "PCA projection of the resident corpus") next to the host
route a user had before it.  One process, every leg warmed, the legs taken in turn, REPS repetitions, each repetition reported.

(a) the device route at RadioNews' size, 33 179 rows x 1792 -> 167, on a ResidentCorpus in fp32 and in bf16: ``fit_pca`` (column sums,
    the Gram matrix, the read-back and the host eigenproblem) and ``projected``, a host clock round work that ends in a device
    synchronise; the three kernels alone between device events, with the rate of the Gram kernel computed from the flops the algorithm
    needs (the triangle on and above the diagonal: rows * D * (D + 64) flops in 64-wide tiles);
(b) the host route: sklearn's ``PCA(167, svd_solver='full').fit_transform`` on the fp32 matrix where sklearn is importable, else NumPy
    fp64 (covariance, eigh, projection), with the threads the environment allows, plus the upload of the projected matrix;
(c) one training step of a one-layer BiLSTM (hidden 256, bf16, 8 documents per batch) fed from the corpus at width 1792 and at width 167.

  python tools/pca_bench.py [--out profiles/pca_bench.json] [--reps 3] [--rows 33179] [--width 1792] [--components 167]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodaltopicsegmentation_amd import AudioPortionDataset, BiLSTM, ResidentCorpus, ops  # noqa: E402
from multimodaltopicsegmentation_amd.trainer import NativeTrainer  # noqa: E402

DEV = 'cuda'
N_DOCS = 55


def dataset(rows, D, seed=0):
    """N_DOCS ragged documents, ``rows`` sentences in all; columns with means several times their spread, as text encoders give"""
    g = torch.Generator().manual_seed(seed)
    cut = torch.linspace(0, rows, N_DOCS + 1).round().long()
    cut[1:-1] += torch.randint(-100, 101, (N_DOCS - 1,), generator=g).clamp(min=-(rows // (4 * N_DOCS)), max=rows // (4 * N_DOCS))
    mean = 3.0 * torch.randn(D, generator=g)
    mix = torch.randn(64, D, generator=g) / 8.0
    lines = []
    for k in range(N_DOCS):
        n = int(cut[k + 1] - cut[k])
        x = torch.randn(n, 64, generator=g) @ mix + 0.2 * torch.randn(n, D, generator=g) + mean
        y = (torch.rand(n, generator=g) < 0.05).float()
        y[-1] = 0.0
        lines.append((x, y.tolist(), f'doc{k}.wav'))
    return AudioPortionDataset(lines, {'O': 0, 'B': 1}, CRF=False, truncate=False)


def host_clock(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def device_clock(fn, reps, inner=5):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def device_route(ds, k, reps):
    report = {}
    for wire in ('fp32', 'bf16'):
        corpus = ResidentCorpus(ds, DEV, wire_dtype=wire)
        x = corpus.corpus
        rows, D = int(x.shape[0]), int(x.shape[1])
        reducer = corpus.fit_pca(k)                                                # warm: code objects, LAPACK's workspace
        corpus.projected(reducer)
        center, w = reducer._on_device(x.device)
        leg = {'fit_pca ms': host_clock(lambda: corpus.fit_pca(k), reps),
               'projected ms': host_clock(lambda: corpus.projected(reducer), reps),
               'colsum kernel ms': device_clock(lambda: ops.pca_colsum(x), reps),
               'gram kernel ms': device_clock(lambda: ops.pca_gram(x, center), reps, inner=2),
               'project kernel ms': device_clock(lambda: ops.pca_project(x, center, w), reps)}
        gram_flop = float(rows) * D * (D + 64)
        leg['gram kernel TFLOP/s (triangle flops over kernel time)'] = [gram_flop / (t * 1e-3) / 1e12 for t in leg['gram kernel ms']]
        leg['project kernel TFLOP/s'] = [2.0 * rows * D * k / (t * 1e-3) / 1e12 for t in leg['project kernel ms']]
        report[wire] = leg
        del corpus
    return report


def host_route(ds, k, reps):
    x = torch.cat([torch.as_tensor(e, dtype=torch.float32) for e in ds.embeddings]).numpy()
    try:
        from sklearn.decomposition import PCA

        def project():
            return PCA(n_components=k, svd_solver='full').fit_transform(x)
        how = 'sklearn PCA(svd_solver=full).fit_transform, fp32'
    except ImportError:
        def project():
            x64 = x.astype(np.float64)
            z = x64 - x64.mean(axis=0)
            lam, vec = np.linalg.eigh(z.T @ z / (x.shape[0] - 1))
            return z @ vec[:, ::-1][:, :k]
        how = 'NumPy fp64: covariance, eigh, projection'
    project()
    fit, upload = [], []
    for _ in range(reps):
        t = time.perf_counter()
        y = project()
        fit.append((time.perf_counter() - t) * 1e3)
        yt = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
        upload += host_clock(lambda: yt.to(DEV), 1)
    return {'how': how, 'threads': os.environ.get('OMP_NUM_THREADS', 'unset'), 'fit_transform ms': fit, 'upload ms': upload}


def step_legs(ds, k, reps, steps=20):
    corpus = ResidentCorpus(ds, DEV, wire_dtype='bf16')
    small = corpus.projected(corpus.fit_pca(k))
    out = {}
    for name, c in (('width %d' % corpus.corpus.shape[1], corpus), ('width %d' % k, small)):
        model = BiLSTM(2, int(c.corpus.shape[1]), 256, num_layers=1, loss_fn='FocalLoss', compute_dtype='bf16', seed=1).to(DEV)
        trainer = NativeTrainer(model, lr=1e-3)
        batches = [c.batch(list(range(s, s + 8))) for s in range(0, 48, 8)]

        def run():
            for i in range(steps):
                trainer.step(batches[i % len(batches)])
        run()
        out[name + ': BiLSTM step ms'] = [t / steps for t in host_clock(run, reps)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rows', type=int, default=33179)
    ap.add_argument('--width', type=int, default=1792)
    ap.add_argument('--components', type=int, default=167)
    ap.add_argument('--skip-host', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pca_bench: no GPU visible; nothing is measured on the CPU')
    ds = dataset(a.rows, a.width)
    report = {'device': torch.cuda.get_device_name(0), 'rows': a.rows, 'width': a.width, 'components': a.components,
              'device route': device_route(ds, a.components, a.reps)}
    if not a.skip_host:
        report['host route'] = host_route(ds, a.components, a.reps)
    report['training step'] = step_legs(ds, a.components, a.reps)
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
