#!/usr/bin/env python3
"""Generate g18_recurrent_longt5.npz by running the REFERENCE's RecurrentLongT5 on CPU.

Run in the build container only (needs the reference checkout and transformers, which never travel to the GPU box):

    python tests/golden/make_golden_recurrent_longt5.py

Imports the reference through make_golden.py (same three stub modules).  Weights follow make_golden.seeded_param with two changes
(mirrored by tests/longt5_oracle.py::seeded_longt5_param): RMSNorm weights (`*layer_norm.weight`) get 1 + 0.1 u, and the dead
`shared.weight` [32128, d] keeps its own init (it never reaches the output).  Stores data only: inputs, lengths, tags, the recipe's
seed, and the reference's eval-mode scores (padded rows included), loss, tags at threshold 0.5, the input gradient and the gradients
of every live parameter, the live and state_dict keys; the two upstream errors (type and message); and the reference's offset ->
bucket tables (_relative_position_bucket on offsets -r..r with this wrapper's bucket count max(4, r) and max distance r + 1), so
that no test has to import transformers.

Cases (key prefix):
  a_  D 64, H 32, 4 heads, r 8, 2 blocks, FocalLoss, ragged lengths with a length-1 document, max length 23 (not a multiple of
      r + 1); every gradient stored whole
  b_  D 128, H 64, 2 heads, r 3 (buckets = max(4, r) = 4), 1 block, BinaryCrossEntropy; parameter gradients as checksum
      [sum, sum |.|, sum of squares] + first 32 values
  c_  D 64, H 32, 2 heads, r 15 (an odd bucket count), 1 block, FocalLoss; gradients as in b_
"""
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (stubs + the reference's modules, make_targets, checksum, save)

CASES = {
    'a': dict(D=64, H=32, heads=4, r=8, NL=2, loss_fn='FocalLoss', B=3, L=23, lengths=[23, 1, 17], seed=1801, full=True),
    'b': dict(D=128, H=64, heads=2, r=3, NL=1, loss_fn='BinaryCrossEntropy', B=2, L=19, lengths=[19, 7], seed=1802, full=False),
    'c': dict(D=64, H=32, heads=2, r=15, NL=1, loss_fn='FocalLoss', B=3, L=40, lengths=[40, 29, 3], seed=1803, full=False),
}
TABLE_RADII = list(range(1, 17)) + [30, 60, 120, 127, 200, 300]


def live(name):
    return not name.endswith('shared.weight') and 'embed_tokens' not in name


def seeded_longt5_param(name, shape, seed):
    rng = np.random.default_rng((zlib.crc32(name.encode()) + seed) & 0xFFFFFFFF)
    u = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    if name.endswith('layer_norm.weight'):
        return 1.0 + 0.1 * u
    return G.seeded_param(name, shape, seed)


def build(c, loss_fn=None, D=None, NL=None):
    return sys.modules['models.CRF'].RecurrentLongT5(2, D or c['D'], c['H'], num_layers=NL or c['NL'], nheads=c['heads'],
                                                       loss_fn=loss_fn or c['loss_fn'], window_size=c['r'])


def run_case(c):
    D, H, heads, r, NL, B, L, lengths, seed = (c[k] for k in ('D', 'H', 'heads', 'r', 'NL', 'B', 'L', 'lengths', 'seed'))
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, L, D)).astype(np.float32)
    y = G.make_targets(rng, lengths, L, -1)
    torch.manual_seed(seed)
    m = build(c)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if live(n):
                p.copy_(torch.from_numpy(seeded_longt5_param(n, tuple(p.shape), seed)))
    m.eval()
    xt = torch.from_numpy(x).requires_grad_(True)
    lt, yt = torch.tensor(lengths), torch.from_numpy(y)
    loss = m.loss(xt, lt, yt)
    loss.backward()
    out = {'x': x, 'lengths': np.array(lengths, dtype=np.int64), 'tags': y, 'cfg': np.array([D, H, heads, r, NL], dtype=np.int64),
           'seed': np.array(seed), 'loss': np.array(loss.item(), dtype=np.float64), 'gx': xt.grad.numpy().copy()}
    with torch.no_grad():
        m.th = 0.5
        scores, tags = m(torch.from_numpy(x), lt)
    out['scores'] = scores.numpy().copy()
    out['tags0.5'] = np.concatenate([np.array(t, dtype=np.int64) for t in tags])
    out['live_keys'] = np.array(sorted(n for n, _ in m.named_parameters() if live(n)))
    out['ref_keys'] = np.array(sorted(m.state_dict().keys()))
    for n, p in m.named_parameters():
        if not live(n):
            assert p.grad is None or not p.grad.any(), n
            continue
        gv = p.grad.detach().numpy().copy()
        if c['full']:
            out['g.' + n] = gv
        else:
            out['gsum.' + n] = G.checksum(gv)
            out['ghead.' + n] = gv.ravel()[:32].copy()
    return out


def upstream_errors():
    out = {}
    c = CASES['a']
    try:
        build(c, loss_fn='CrossEntropy')
    except Exception as e:  # noqa: BLE001
        out['err_ce_type'], out['err_ce_msg'] = np.array(type(e).__name__), np.array(str(e))
    x = torch.randn(2, 5, 48)
    for NL in (1, 2):
        torch.manual_seed(0)
        m = build(c, D=48, NL=NL)               # embedding_dim 48 != 2 * hidden 64: constructs, fails on the first call
        m.eval()
        try:
            m.loss(x, torch.tensor([5, 3]), torch.zeros(2, 5))
        except Exception as e:  # noqa: BLE001
            out[f'err_d_nl{NL}_type'], out[f'err_d_nl{NL}_msg'] = np.array(type(e).__name__), np.array(str(e))
    return out


def bucket_tables():
    from transformers.models.longt5.modeling_longt5 import LongT5LocalAttention
    out = {}
    for r in TABLE_RADII:
        t = LongT5LocalAttention._relative_position_bucket(torch.arange(-r, r + 1), bidirectional=True, num_buckets=max(4, r + 1 // 4),
                                                           max_distance=r + 1)
        out[f'bucket_r{r}'] = t.numpy().astype(np.int64)
    return out


def main():
    arrays = {}
    for k, c in CASES.items():
        arrays.update({f'{k}_{n}': v for n, v in run_case(c).items()})
    arrays.update(upstream_errors())
    arrays.update(bucket_tables())
    G.save('g18_recurrent_longt5', **arrays)


if __name__ == '__main__':
    main()
