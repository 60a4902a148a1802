#!/usr/bin/env python3
"""Generate g21_cosine_loss.npz by running the `segments=` branch of the REFERENCE's BiLSTM.loss and BiLSTMLateFusion.loss
(models/CRF.py:23-92, :319-337, :420-442) on CPU.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_golden_cosine.py

Imports the reference through make_golden.py (same three stub modules).  Weights follow make_golden.seeded_param and are not stored.
Stores data only: inputs, lengths, collater-style tags (pad -1; pad 0, the CRF collater's value, for BinaryCrossEntropy -- see below), the segment lists (flattened, with offsets), the recipe's seed, and the
reference's eval-mode loss, input gradient, every parameter gradient and the cosine of every pair (torch.cosine_similarity of the
reference's own aggregate_embeddings samples, positives then negatives as cosine_loss concatenates them); the result without any pair
(segments = [[]] * B: the cosine term is the int 0 and the main loss stays unmasked); the IndexError of a `segments` shorter than the
batch; the ValueError of each loss function when the targets do not cover exactly max(lengths) positions; and the RuntimeError of
BinaryCrossEntropy on pad -1: the branch does not un-pad, and nn.BCELoss refuses targets outside [0, 1] (FocalLoss evaluates its
formula at y = -1, CrossEntropy ignores -1).

Conditions asserted here, never relaxed: every negative pair with a non-empty partner has |cos| >= 0.05 (the clamp side of max(cos, 0)
cannot flip under bf16), at least one such pair over the fixture has cos < 0, every stored value is finite.  The seeds were picked by
scanning 2101..2130 for these conditions with the widest margin.

Cases (key prefix; between them: a singleton segment, odd-length segments, a last end equal to and below the length, a length-1 document
with and without a listed end, documents with [], and H = 12, which the product stores padded to 16):
  fo_  BiLSTM, FocalLoss,          D 64, H 32, 2 layers, lengths [23, 17, 1, 9, 23, 2]
  bc_  BiLSTM, BinaryCrossEntropy, D 24, H 12, 1 layer,  lengths [19, 7, 1], pad 0
  ce_  BiLSTM, CrossEntropy,       D 64, H 32, 1 layer,  lengths [40, 29, 3]
  lf_  BiLSTMLateFusion, FocalLoss, D (64, 24), H 12, 1 layer, lengths [23, 17, 1, 9, 23, 2]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402  (stubs + the reference's modules, seeded_param, make_targets, save)

SEG_A = [[1, 4, 9, 16, 23], [5, 6, 12], [1], [], [2, 3, 10, 20], [2]]
CASES = {
    'fo': dict(cls='BiLSTM', loss_fn='FocalLoss', D=64, H=32, NL=2, lengths=[23, 17, 1, 9, 23, 2], segments=SEG_A, seed=2101),
    'bc': dict(cls='BiLSTM', loss_fn='BinaryCrossEntropy', D=24, H=12, NL=1, lengths=[19, 7, 1], segments=[[3, 4, 11, 19], [2, 5], []], seed=2105, pad=0),
    'ce': dict(cls='BiLSTM', loss_fn='CrossEntropy', D=64, H=32, NL=1, lengths=[40, 29, 3], segments=[[7, 8, 21, 33], [], [1, 3]], seed=2103),
    'lf': dict(cls='BiLSTMLateFusion', loss_fn='FocalLoss', D=(64, 24), H=12, NL=1, lengths=[23, 17, 1, 9, 23, 2], segments=SEG_A, seed=2112),
}
MIN_COS = 0.05


def build(c):
    m = getattr(sys.modules['models.CRF'], c['cls'])(2, list(c['D']) if isinstance(c['D'], tuple) else c['D'], c['H'], num_layers=c['NL'],
                                                     loss_fn=c['loss_fn'], device='cpu')
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.from_numpy(G.seeded_param(n, tuple(p.shape), c['seed'])))
    return m.eval()


def inputs(c):
    lengths = c['lengths']
    B, L = len(lengths), max(lengths)
    rng = np.random.default_rng(c['seed'])
    Ds = c['D'] if isinstance(c['D'], tuple) else (c['D'],)
    xs = [rng.standard_normal((B, L, D)).astype(np.float32) for D in Ds]
    return xs, G.make_targets(rng, lengths, L, c.get('pad', -1))


def call_loss(m, xs, lengths, y, segments):
    xt = [torch.from_numpy(x).requires_grad_(True) for x in xs]
    loss = m.loss(*xt, torch.tensor(lengths), torch.from_numpy(y), segments=segments)
    return loss, xt


def pair_cosines(m, xs, lengths, segments):
    """cos of every pair from the reference's own encoder and aggregate_embeddings; also which negative pairs have a non-empty partner"""
    C = sys.modules['models.CRF']
    lt = torch.tensor(lengths)
    with torch.no_grad():
        if len(xs) == 1:
            e = m.model(torch.from_numpy(xs[0]), lt)
        else:
            e = torch.cat((m.model1(torch.from_numpy(xs[0]), lt), m.model2(torch.from_numpy(xs[1]), lt)), axis=2)
        p1, p2 = C.aggregate_embeddings(e, lt, segments, 'cpu')
        n1, n2 = C.aggregate_embeddings(e, lt, segments, 'cpu', positive=False)
    a, b = torch.cat((p1, n1)), torch.cat((p2, n2))
    cos = torch.cosine_similarity(a.double(), b.double(), dim=1).numpy()
    nonempty = np.concatenate([np.zeros(len(p1), dtype=bool), (n2.abs().sum(1) > 0).numpy()])
    return cos, nonempty, len(p1)


def run_case(c):
    xs, y = inputs(c)
    lengths, segments = c['lengths'], c['segments']
    torch.manual_seed(c['seed'])
    m = build(c)
    loss, xt = call_loss(m, xs, lengths, y, segments)
    loss.backward()
    cos, nonempty, npos = pair_cosines(m, xs, lengths, segments)
    neg = cos[nonempty]
    print(f"{c['cls']} {c['loss_fn']} seed {c['seed']}: loss {loss.item():.6f}, {npos} positive + {len(cos) - npos} negative pairs, "
          f"min |cos| over negatives with a partner {np.abs(neg).min():.3f}, {int((neg < 0).sum())} of them < 0")
    assert np.abs(neg).min() >= MIN_COS, np.abs(neg).min()
    D = c['D'] if isinstance(c['D'], tuple) else (c['D'], 0)
    out = {'lengths': np.array(lengths, dtype=np.int64), 'tags': y, 'cfg': np.array([D[0], D[1], c['H'], c['NL']], dtype=np.int64),
           'seed': np.array(c['seed']), 'loss_fn': np.array(c['loss_fn']), 'cls': np.array(c['cls']),
           'seg_flat': np.array([s for d in segments for s in d], dtype=np.int64),
           'seg_off': np.cumsum([0] + [len(d) for d in segments]).astype(np.int64),
           'loss': np.array(loss.item(), dtype=np.float64), 'cos': cos.astype(np.float64), 'npos': np.array(npos),
           'cos_nonempty': nonempty}
    for i, (x, t) in enumerate(zip(xs, xt)):
        out[f'x{i + 1}'], out[f'gx{i + 1}'] = x, t.grad.numpy().copy()
    for n, p in m.named_parameters():
        out['g.' + n] = p.grad.detach().numpy().copy()
    # no pair at all: the cosine term is the int 0, the main loss stays unmasked
    m.zero_grad()
    loss0, xt0 = call_loss(m, xs, lengths, y, [[] for _ in lengths])
    loss0.backward()
    out['p0_loss'] = np.array(loss0.item(), dtype=np.float64)
    out['p0_gx1'] = xt0[0].grad.numpy().copy()
    out['p0_g.classification.bias'] = m.classification.bias.grad.detach().numpy().copy()
    assert all(np.isfinite(v).all() for v in out.values() if v.dtype.kind == 'f')
    return out, bool((neg < 0).any())


def upstream_errors():
    out = {}
    c = CASES['bc']
    xs, y = inputs(c)
    m = build(c)
    try:
        call_loss(m, xs, c['lengths'], y, c['segments'][:-1])
    except Exception as e:  # noqa: BLE001
        out['err_short_type'], out['err_short_msg'] = np.array(type(e).__name__), np.array(str(e))
    ypad = y.copy()
    for b, n in enumerate(c['lengths']):
        ypad[b, n:] = -1                          # the non-CRF collater's pad
    try:
        call_loss(m, xs, c['lengths'], ypad, c['segments'])
    except Exception as e:  # noqa: BLE001
        out['err_bce_pad_type'], out['err_bce_pad_msg'] = np.array(type(e).__name__), np.array(str(e))
    ylong = np.concatenate([y, np.full((y.shape[0], 1), -1, dtype=np.float32)], axis=1)
    for loss_fn in ('FocalLoss', 'BinaryCrossEntropy', 'CrossEntropy'):
        m = build(dict(c, loss_fn=loss_fn))
        try:
            call_loss(m, xs, c['lengths'], ylong, c['segments'])
        except Exception as e:  # noqa: BLE001
            out[f'err_tags_{loss_fn}_type'], out[f'err_tags_{loss_fn}_msg'] = np.array(type(e).__name__), np.array(str(e))
    assert len(out) == 10, sorted(out)
    return out


def main():
    arrays, any_negative = {}, False
    for k, c in CASES.items():
        out, negative = run_case(c)
        any_negative |= negative
        arrays.update({f'{k}_{n}': v for n, v in out.items()})
    assert any_negative
    arrays.update(upstream_errors())
    G.save('g21_cosine_loss', **arrays)


if __name__ == '__main__':
    main()
