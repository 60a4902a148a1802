#!/usr/bin/env python3
"""Generate g19_sheikh_bilstm.npz by running the REFERENCE's SheikhBiLSTM (models/CRF.py:980-1041) on CPU.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_golden_sheikh.py

Imports the reference through make_golden.py (same three stub modules).  Weights follow make_golden.seeded_param; case c multiplies both
`*_dense.weight` by 6 so that |s| reaches ~4 and the decode lists are mixed.  Stores data only: inputs, lengths, tags, the recipe's seed
and dense-weight scale, and the reference's eval-mode scores (every row, the appended 1.0 included), loss, input gradient, the gradient
of every live parameter, the decode lists at th 0.5 / 0.4 / 0.3, the live and state_dict key lists (also under TextSegmenter), the two
upstream errors (type and message) and the all-length-1 result (NaN loss, zero gradients).

The model is built with dropout_in = 0: RNN.forward applies F.dropout without training=, so the class default 0.5 would drop
half the input in eval mode too.

Conditions asserted here, never relaxed: max |s| <= 8 over every row (beyond it the reference's 1 - sigmoid(s) loses the loss to
rounding), and every valid position has |1 - sigmoid(s) - th| >= 1e-4 for each stored threshold -- a threshold that fails is dropped.

Cases (key prefix):
  a_  D 64, H 32, 2 layers, lengths [23, 17, 1, 9, 23, 2] (69 loss elements; a length-1 document contributes nothing)
  b_  D 24, H 12, 1 layer, lengths [19, 7, 1] (H not a multiple of 8: stored padded by the product)
  c_  D 64, H 32, 1 layer, lengths [40, 29, 3], dense weights x 6
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (stubs + the reference's modules, seeded_param, make_targets, save)

CASES = {
    'a': dict(D=64, H=32, NL=2, lengths=[23, 17, 1, 9, 23, 2], seed=1901, wscale=1.0),
    'b': dict(D=24, H=12, NL=1, lengths=[19, 7, 1], seed=1902, wscale=1.0),
    'c': dict(D=64, H=32, NL=1, lengths=[40, 29, 3], seed=1903, wscale=6.0),
}
THRESHOLDS = (0.5, 0.4, 0.3)
MARGIN = 1e-4


def live(name):
    return not name.startswith('classification.')


def ref_class():
    return sys.modules['models.CRF'].SheikhBiLSTM


def build(c, **kw):
    m = ref_class()(2, c['D'], c['H'], c['NL'], dropout_in=0.0, **kw)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if live(n):
                w = G.seeded_param(n, tuple(p.shape), c['seed'])
                if n.endswith('_dense.weight'):
                    w = w * np.float32(c['wscale'])
                p.copy_(torch.from_numpy(w))
    return m.eval()


def run_case(c):
    D, H, NL, lengths, seed = (c[k] for k in ('D', 'H', 'NL', 'lengths', 'seed'))
    B, L = len(lengths), max(lengths)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, L, D)).astype(np.float32)
    y = G.make_targets(rng, lengths, L, -1)
    torch.manual_seed(seed)
    m = build(c)
    xt = torch.from_numpy(x).requires_grad_(True)
    lt, yt = torch.tensor(lengths), torch.from_numpy(y)
    loss = m.loss(xt, lt, yt)
    loss.backward()
    out = {'x': x, 'lengths': np.array(lengths, dtype=np.int64), 'tags': y, 'cfg': np.array([D, H, NL], dtype=np.int64),
           'seed': np.array(seed), 'wscale': np.array(c['wscale'], dtype=np.float64), 'loss': np.array(loss.item(), dtype=np.float64),
           'gx': xt.grad.numpy().copy()}
    kept = []
    for th in THRESHOLDS:
        m.th = th
        with torch.no_grad():
            scores, tags = m(torch.from_numpy(x), lt)
        s = scores.numpy().astype(np.float64)
        assert np.abs(s).max() <= 8.0, np.abs(s).max()
        q = 1.0 - 1.0 / (1.0 + np.exp(-s[:, :, 0]))
        margin = min(np.abs(q[b, :n] - th).min() for b, n in enumerate(lengths))
        print(f'case seed {seed} th {th}: min margin {margin:.2e}, max |s| {np.abs(s).max():.3f}')
        if margin < MARGIN:
            continue                              # dropped, never a wider tolerance
        kept.append(th)
        out[f'tags{th}'] = np.concatenate([np.array(t, dtype=np.int64) for t in tags])
    out['scores'] = scores.numpy().copy()
    out['ths'] = np.array(kept, dtype=np.float64)
    out['live_keys'] = np.array(sorted(n for n, _ in m.named_parameters() if live(n)))
    out['ref_keys'] = np.array(sorted(m.state_dict().keys()))
    for n, p in m.named_parameters():
        if not live(n):
            assert p.grad is None, n              # classification.*: read by no method
            continue
        out['g.' + n] = p.grad.detach().numpy().copy()
    return out


def upstream_errors():
    out = {}
    c = CASES['b']
    try:
        ref_class()(2, c['D'], c['H'], c['NL'], loss_fn='CrossEntropy')
    except Exception as e:  # noqa: BLE001
        out['err_loss_type'], out['err_loss_msg'] = np.array(type(e).__name__), np.array(str(e))
    m = build(c, loss_fn='FocalLoss')             # accepted; the loss is nn.BCELoss all the same (:1002)
    assert type(m.loss_fn).__name__ == 'BCELoss'
    try:
        m(torch.zeros(2, 5, c['D']), torch.tensor([5, 3]))
    except Exception as e:  # noqa: BLE001
        out['err_th_type'], out['err_th_msg'] = np.array(type(e).__name__), np.array(str(e))
    return out


def all_length_one():
    c = CASES['b']
    m = build(c)
    rng = np.random.default_rng(1904)
    x = rng.standard_normal((3, 1, c['D'])).astype(np.float32)
    lt = torch.tensor([1, 1, 1])
    loss = m.loss(torch.from_numpy(x), lt, torch.zeros(3, 1))
    loss.backward()
    gmax = max(0.0 if p.grad is None else float(p.grad.abs().max()) for n, p in m.named_parameters() if live(n))
    m.th = 0.4
    with torch.no_grad():
        scores, tags = m(torch.from_numpy(x), lt)
    return {'len1_x': x, 'len1_loss': np.array(loss.item(), dtype=np.float64), 'len1_gmax': np.array(gmax), 'len1_scores': scores.numpy().copy(),
            'len1_tags0.4': np.concatenate([np.array(t, dtype=np.int64) for t in tags])}


def text_segmenter_keys():
    ts = G.TextSegmenter(2, 24, 12, architecture='SheikhBiLSTM')
    return {'ts_keys': np.array(sorted(ts.state_dict().keys())),
            'ts_dropout': np.array([ts.model.lstm.dropout_in, ts.model.lstm.dropout_out], dtype=np.float64)}


def main():
    arrays = {}
    for k, c in CASES.items():
        arrays.update({f'{k}_{n}': v for n, v in run_case(c).items()})
    arrays.update(upstream_errors())
    arrays.update(all_length_one())
    arrays.update(text_segmenter_keys())
    G.save('g19_sheikh_bilstm', **arrays)


if __name__ == '__main__':
    main()
