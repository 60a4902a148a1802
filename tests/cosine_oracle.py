"""fp64 restatement of the `segments=` branch of BiLSTM.loss / BiLSTMLateFusion.loss (models/CRF.py:23-92, :322-337, :427-442) on top of
oracle.restatement's LSTM and loss elements.

    e = encoder output [B, Lm, W] (Lm = max(lengths); rows at or past a document's length are 0), dropout 0
    per document b, e_b = e[b, :len_b], prev = 0; for every listed end s_j, in order, seg_j = e_b[prev:s_j]:
        positive pair (target +1), only if len(seg_j) > 1:  (seg_j[::2].sum(0), seg_j[1::2].sum(0))
        negative pair (target -1), always:                  (seg_j.sum(0), nxt.sum(0)),  nxt = e_b[s_j:s_{j+1}], e_b[s_j:] after the last end
        prev = s_j
    pairs are concatenated as upstream does: every positive pair (document order), then every negative pair
    cos = a.b / sqrt((|a|^2 + 1e-12)(|b|^2 + 1e-12));  term = 1 - cos (+1) | max(cos, 0) (-1);  cos_loss = mean over all pairs, or the int 0
    main loss: NOT un-padded -- loss_fn over all B * Lm positions with whatever target sits there (CE keeps ignore_index = -1)
    total = 0.1 * cos_loss + main
"""
from typing import Dict, List, Sequence, Tuple

import torch
from torch import Tensor

from oracle.restatement import bce_on_probs, cross_entropy_ignore, rnn_forward, sigmoid_focal_loss
from tests.helpers import bilstm_param_shapes

EPS = 1e-12
WEIGHT = 0.1


def param_shapes(D, H, NL, n_out, late_fusion=False):
    if not late_fusion:
        s = bilstm_param_shapes(D, H, NL, n_out, prefix='model.')
        s['classification.weight'], s['classification.bias'] = (n_out, 2 * H), (n_out,)
        return s
    s = bilstm_param_shapes(D[0], H, NL, n_out, prefix='model1.')
    s.update(bilstm_param_shapes(D[1], H, NL, n_out, prefix='model2.'))
    s['classification.weight'], s['classification.bias'] = (n_out, 4 * H), (n_out,)
    return s


def pair_samples(e: Tensor, lengths: Sequence[int], segments: Sequence[Sequence[int]]) -> Tuple[List[Tensor], List[Tensor], List[int]]:
    """aggregate_embeddings twice (positive, then negative), with Python slicing as upstream: IndexError when segments is short."""
    a, b, t = [], [], []
    for positive in (True, False):
        for bi in range(e.shape[0]):
            eb = e[bi, :int(lengths[bi])]
            ends = segments[bi]
            prev = 0
            for j, s in enumerate(ends):
                seg = eb[prev:s]
                if positive:
                    if len(seg) > 1:
                        a.append(seg[::2].sum(0))
                        b.append(seg[1::2].sum(0))
                        t.append(1)
                else:
                    nxt = eb[s:ends[j + 1]] if j + 1 < len(ends) else eb[s:]
                    a.append(seg.sum(0))
                    b.append(nxt.sum(0))
                    t.append(-1)
                prev = s
    return a, b, t


def cosine_loss(e: Tensor, lengths, segments):
    """-> (mean cosine-embedding loss or the int 0, cos of every pair [P], targets [P])"""
    a, b, t = pair_samples(e, lengths, segments)
    if not t:
        return 0, torch.zeros(0, dtype=e.dtype), torch.zeros(0, dtype=torch.long)
    A, Bm, T = torch.stack(a), torch.stack(b), torch.tensor(t)
    cos = (A * Bm).sum(1) / torch.sqrt(((A * A).sum(1) + EPS) * ((Bm * Bm).sum(1) + EPS))
    term = torch.where(T > 0, 1 - cos, cos.clamp(min=0))
    return term.mean(), cos, T


def main_loss(scores: Tensor, tags: Tensor, loss_fn: str, alpha: float = 0.9, gamma: float = 2.0) -> Tensor:
    """The unmasked main loss of the segments branch over all B * Lm positions (models/CRF.py:328-333)."""
    if loss_fn == 'CrossEntropy':
        return cross_entropy_ignore(scores, tags)
    x, y = scores.reshape(-1), tags.reshape(-1).to(scores.dtype)
    if x.shape != y.shape:
        raise ValueError(f'target size {tuple(y.shape)} differs from input size {tuple(x.shape)}')
    return sigmoid_focal_loss(x, y, alpha, gamma) if loss_fn == 'FocalLoss' else bce_on_probs(x, y)


def encoder(x, lengths: Tensor, p: Dict[str, Tensor], batched: bool = True) -> Tensor:
    """x: a tensor (BiLSTM) or a pair (BiLSTMLateFusion: the concatenation of the two encoders' outputs)."""
    NL = sum(1 for k in p if '.rnn.weight_hh_l' in k and not k.endswith('_reverse') and not k.startswith('model2.'))
    if isinstance(x, (tuple, list)):
        return torch.cat((rnn_forward(x[0], lengths, p, 'model1.', NL, True, batched), rnn_forward(x[1], lengths, p, 'model2.', NL, True, batched)), dim=2)
    return rnn_forward(x, lengths, p, 'model.', NL, True, batched)


def loss(x, lengths: Tensor, tags: Tensor, segments, p: Dict[str, Tensor], loss_fn: str, batched: bool = True):
    """-> (total, cos of every pair, scores [B, Lm, n_out])"""
    e = encoder(x, lengths, p, batched)
    cl, cos, _ = cosine_loss(e, lengths.tolist(), segments)
    scores = e @ p['classification.weight'].t() + p['classification.bias']
    return WEIGHT * cl + main_loss(scores, tags, loss_fn), cos, scores
