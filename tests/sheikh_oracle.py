"""fp64 restatement of SheikhBiLSTM (models/CRF.py:980-1041) on top of oracle.restatement's LSTM.

    h = RNN(x, lengths)                                  [B, Lm, 2H], Lm = max(lengths); rows at or past a document's length are 0
    F = forward_dense(h[:, :-1, :H]),  G = backward_dense(h[:, 1:, H:])
    s[b, t] = sum_h F[b, t, h] G[b, t, h]                t < Lm - 1: the forward state at t with the backward state at t + 1
    forward appends one step of ones -> [B, Lm, 1]; padded positions hold real values (bias . bias, F(h_t) . b_b at t = len - 1)
    loss  = BCELoss(1 - sigmoid(s), 1 - y) over the concatenation of s[b, :len_b - 1]  =  BCE-with-logits(s, y), stated here in its
            stable form (the reference's fp32 value is within 2e-7 of it for |s| <= 8; beyond |s| ~ 17 the reference saturates)
    decode = (1 - sigmoid(s))[:, :, 0] < th, strict, trimmed to each length
"""
from typing import Dict, List

import torch
from torch import Tensor

from oracle.restatement import rnn_forward
from tests.helpers import bilstm_param_shapes


def param_shapes(D, H, NL):
    """Live state_dict keys of the reference's SheikhBiLSTM and their shapes (classification.* is read by no method)."""
    s = bilstm_param_shapes(D, H, NL, 1, prefix='lstm.')
    for n in ('forward_dense', 'backward_dense'):
        s[n + '.weight'] = (H, H)
        s[n + '.bias'] = (H,)
    return s


def scores(x: Tensor, lengths: Tensor, p: Dict[str, Tensor], batched: bool = True) -> Tensor:
    """Every row [B, max(len), 1], the appended 1.0 included (dropout 0)."""
    NL = sum(1 for k in p if k.startswith('lstm.rnn.weight_hh_l') and not k.endswith('_reverse'))
    h = rnn_forward(x, lengths, p, 'lstm.', NL, True, batched)
    H = h.shape[2] // 2
    F = h[:, :-1, :H] @ p['forward_dense.weight'].t() + p['forward_dense.bias']
    G = h[:, 1:, H:] @ p['backward_dense.weight'].t() + p['backward_dense.bias']
    s = (F * G).sum(dim=2, keepdim=True)
    return torch.cat((s, torch.ones(h.shape[0], 1, 1, dtype=s.dtype)), dim=1)


def loss(s: Tensor, lengths: Tensor, tags: Tensor) -> Tensor:
    """Mean over sum_b max(len_b - 1, 0) elements (NaN when there is none, as the mean of an empty tensor upstream)."""
    xs, ys = [], []
    for b in range(s.shape[0]):
        n = max(int(lengths[b]) - 1, 0)
        xs.append(s[b, :n, 0])
        ys.append(tags[b, :n])
    x = torch.cat(xs)
    y = torch.cat(ys).to(x.dtype)
    return ((1 - y) * x - torch.nn.functional.logsigmoid(x)).mean()


def decode(s: Tensor, lengths: Tensor, th: float) -> List[List[bool]]:
    tag = (1 - torch.sigmoid(s))[:, :, 0] < th
    return [tag[i].tolist()[:int(n)] for i, n in enumerate(lengths)]
