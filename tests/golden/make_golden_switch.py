#!/usr/bin/env python3
"""Generate g20_switch_bilstm.npz by running the REFERENCE's SwitchBiLSTM (models/CRF.py:1046-1270) on CPU.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_golden_switch.py

Imports the reference through make_golden.py (same three stub modules).  Weights follow make_golden.seeded_param; every head weight
(`classification*.weight`) is multiplied by 16 so that the scores spread and the decode lists are mixed.  Stores data only: inputs, lengths,
tags, domains, the recipe's seed and head scale, and the reference's eval-mode scores (every row), loss, input gradient, the gradient of
every parameter that has one, the names of those whose grad is None, the decode lists at th 0.5 / 0.4 / 0.3, the state_dict key lists per
mode (also under TextSegmenter), the exception of a mixed batch in lstm mode and the exception types of predict_step and switch='bias'.

What the reference does with a mixed batch in dense mode (the generator re-asserts it): with idx1 = the truthy documents and idx2 = the
rest, regroup assigns out[idx1[k]] = head_1(h)[k] and out[idx2[k]] = head_2(h)[k] -- document i gets the scores computed from the encoder
rows of document rank(i), its position inside its own group.

Conditions asserted here, never relaxed: every valid position has |prob - th| >= 1e-4 for each stored threshold -- a threshold that fails
is dropped -- and at least one kept threshold per case has a decode list with both values.

Cases (key prefix), all dense unless said:
  a_   D 64, H 32, 2 layers, lengths [23, 17, 1, 9, 23, 2], domains [1, 0, 1, 1, 0, 0], FocalLoss
  b_   D 24, H 12, 1 layer, lengths [19, 7, 1], domains [0, 1, 0], BinaryCrossEntropy (H not a multiple of 8: stored padded by the product)
  c_   D 64, H 32, 1 layer, lengths [40, 29, 3, 12], domains [0, 0, 1, 0], CrossEntropy
  d1_ / d0_   case a with domains all 1 / all 0
  e1_ / e0_   D 24, H 12, 1 layer, lengths [19, 7, 1], domains all 1 / all 0, FocalLoss, lstm mode
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (stubs + the reference's modules, seeded_param, make_targets, save)

A = dict(D=64, H=32, NL=2, lengths=[23, 17, 1, 9, 23, 2], loss_fn='FocalLoss', mode='dense', seed=2001)
E = dict(D=24, H=12, NL=1, lengths=[19, 7, 1], loss_fn='FocalLoss', mode='lstm', seed=2004)
CASES = {
    'a': dict(A, domains=[1, 0, 1, 1, 0, 0]),
    'b': dict(D=24, H=12, NL=1, lengths=[19, 7, 1], domains=[0, 1, 0], loss_fn='BinaryCrossEntropy', mode='dense', seed=2002),
    'c': dict(D=64, H=32, NL=1, lengths=[40, 29, 3, 12], domains=[0, 0, 1, 0], loss_fn='CrossEntropy', mode='dense', seed=2003),
    'd1': dict(A, domains=[1] * 6),
    'd0': dict(A, domains=[0] * 6),
    'e1': dict(E, domains=[1] * 3),
    'e0': dict(E, domains=[0] * 3),
}
THRESHOLDS = (0.5, 0.4, 0.3)
MARGIN = 1e-4
HEAD_SCALE = 16.0


def ref_class():
    return sys.modules['models.CRF'].SwitchBiLSTM


def build(c):
    m = ref_class()(2, c['D'], c['H'], c['NL'], loss_fn=c['loss_fn'], switch_lstm_adapt=c['mode'] == 'lstm',
                    switch_dense_adapt=c['mode'] == 'dense')
    assert m.switch == (c['mode'] if c['mode'] != 'plain' else 0)
    with torch.no_grad():
        for n, p in m.named_parameters():
            w = G.seeded_param(n, tuple(p.shape), c['seed'])
            if n.startswith('classification') and n.endswith('.weight'):
                w = w * np.float32(HEAD_SCALE)
            p.copy_(torch.from_numpy(w))
    return m.eval()


def rank_map(domains):
    """document i -> (the document whose encoder rows it is scored from, its head)"""
    idx1 = [i for i, d in enumerate(domains) if d]
    idx2 = [i for i, d in enumerate(domains) if not d]
    src = {i: k for k, i in enumerate(idx1)}
    src.update({i: k for k, i in enumerate(idx2)})
    return [src[i] for i in range(len(domains))], [0 if d else 1 for d in domains]


def run_case(c):
    D, H, NL, lengths, seed, domains = (c[k] for k in ('D', 'H', 'NL', 'lengths', 'seed', 'domains'))
    B, L = len(lengths), max(lengths)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, L, D)).astype(np.float32)
    y = G.make_targets(rng, lengths, L, -1)
    torch.manual_seed(seed)
    m = build(c)
    xt = torch.from_numpy(x).requires_grad_(True)
    lt, yt = torch.tensor(lengths), torch.from_numpy(y)
    loss = m.loss(xt, lt, yt, domains)
    loss.backward()
    out = {'x': x, 'lengths': np.array(lengths, dtype=np.int64), 'tags': y, 'domains': np.array(domains, dtype=np.int64),
           'cfg': np.array([D, H, NL], dtype=np.int64), 'seed': np.array(seed), 'wscale': np.array(HEAD_SCALE, dtype=np.float64),
           'loss_fn': np.array(c['loss_fn']), 'mode': np.array(c['mode']), 'loss': np.array(loss.item(), dtype=np.float64),
           'gx': xt.grad.numpy().copy()}
    kept, mixed = [], False
    for th in THRESHOLDS:
        m.th = th
        with torch.no_grad():
            scores, tags = m(torch.from_numpy(x), lt, domains)
        s = scores.numpy().astype(np.float64)
        if m.bce:
            prob = 1.0 / (1.0 + np.exp(-s[:, :, 0]))
        else:
            e = np.exp(s - s.max(axis=2, keepdims=True))
            prob = (e / e.sum(axis=2, keepdims=True))[:, :, 1]
        margin = min(np.abs(prob[b, :n] - th).min() for b, n in enumerate(lengths))
        flat = np.concatenate([np.array(t, dtype=np.int64) for t in tags])
        print(f'case seed {seed} domains {domains} th {th}: min margin {margin:.2e}, max |s| {np.abs(s).max():.3f}, ones {int(flat.sum())}/{flat.size}')
        if margin < MARGIN:
            continue                              # dropped, never a wider tolerance
        kept.append(th)
        mixed = mixed or (0 < flat.sum() < flat.size)
        out[f'tags{th}'] = flat
    assert kept and mixed, (seed, kept, mixed)
    out['scores'] = scores.numpy().copy()
    out['ths'] = np.array(kept, dtype=np.float64)
    out['ref_keys'] = np.array(sorted(m.state_dict().keys()))
    none = []
    for n, p in m.named_parameters():
        if p.grad is None:
            none.append(n)
        else:
            out['g.' + n] = p.grad.detach().numpy().copy()
    out['none_keys'] = np.array(sorted(none), dtype=str)
    if c['mode'] == 'dense':
        # the rank map, re-asserted on the reference's own tensors: "quirk" reproduces the scores bit for bit, "fixed" does not (mixed batch)
        with torch.no_grad():
            h = m.model(torch.from_numpy(x), lt)
            heads = (m.classification_1(h), m.classification_2(h))
        src, head = rank_map(domains)
        quirk = torch.stack([heads[head[i]][src[i]] for i in range(B)])
        fixed = torch.stack([heads[head[i]][i] for i in range(B)])
        assert torch.equal(quirk, scores), seed
        if any(domains) and not all(domains):
            assert not torch.equal(fixed, scores), seed
        else:
            assert src == list(range(B))
    return out


def upstream_errors():
    out = {}
    m = build(dict(E, domains=None))
    x, lt, y = torch.zeros(3, 19, E['D']), torch.tensor(E['lengths']), torch.zeros(3, 19)
    for what, call in (('loss', lambda: m.loss(x, lt, y, [0, 1, 0])), ('fwd', lambda: m(x, lt, [0, 1, 0]))):
        try:
            call()
            raise SystemExit(f'lstm mixed {what} did not raise')
        except Exception as e:  # noqa: BLE001
            out[f'lstm_mixed_{what}_type'], out[f'lstm_mixed_{what}_msg'] = np.array(type(e).__name__), np.array(str(e))
    try:
        m.loss(x, lt, y, None)
    except Exception as e:  # noqa: BLE001
        out['none_domains_type'] = np.array(type(e).__name__)
    ts = G.TextSegmenter(2, 24, 12, architecture='SwitchBiLSTM', switch='dense', loss_fn='FocalLoss')
    batch = {'src_tokens': x, 'src_lengths': lt, 'tgt_tokens': y, 'domain': [0, 1, 0], 'src_tokens2': None}
    try:
        ts.predict_step(batch, 0)
        raise SystemExit('predict_step did not raise')
    except Exception as e:  # noqa: BLE001
        out['predict_type'] = np.array(type(e).__name__)
    try:
        G.TextSegmenter(2, 24, 12, architecture='SwitchBiLSTM', switch='bias')
        raise SystemExit("switch='bias' did not raise")
    except Exception as e:  # noqa: BLE001
        out['bias_type'] = np.array(type(e).__name__)
    return out


def key_lists():
    out = {}
    for mode, switch in (('dense', 'dense'), ('lstm', 'lstm'), ('plain', 'anything-else')):
        ts = G.TextSegmenter(2, 24, 12, architecture='SwitchBiLSTM', switch=switch, loss_fn='FocalLoss')
        assert ts.domain is True
        out[f'ts_keys_{mode}'] = np.array(sorted(ts.state_dict().keys()))
        out[f'keys_{mode}'] = np.array(sorted(ts.model.state_dict().keys()))
        out[f'shapes_{mode}'] = np.array([','.join(str(v) for v in ts.model.state_dict()[k].shape) for k in sorted(ts.model.state_dict().keys())])
    return out


def main():
    arrays = {}
    for k, c in CASES.items():
        r = run_case(c)
        if k in ('d1', 'd0'):
            assert (r['x'] == arrays['a_x']).all() and (r['tags'] == arrays['a_tags']).all()
            del r['x'], r['tags']                 # case a's
        if k == 'e0':
            assert (r['x'] == arrays['e1_x']).all() and (r['tags'] == arrays['e1_tags']).all()
            del r['x'], r['tags']                 # case e1's
        arrays.update({f'{k}_{n}': v for n, v in r.items()})
    arrays.update(upstream_errors())
    arrays.update(key_lists())
    G.save('g20_switch_bilstm', **arrays)


if __name__ == '__main__':
    main()
