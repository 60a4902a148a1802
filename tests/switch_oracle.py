"""fp64 restatement of SwitchBiLSTM (models/CRF.py:1046-1270) on top of oracle.restatement's LSTM, with the rank map written out.

    idx1 = the documents whose domain is truthy, idx2 = the rest, both in batch order

    dense   h = RNN('model.')(x, lengths)                          [B, Lm, 2H], Lm = max(lengths); rows at or past a length are 0
            mixed batch: both heads run over the whole batch and ``regroup`` assigns out[idx1[k]] = head_1(h)[k], out[idx2[k]] =
            head_2(h)[k], i.e. with rank(i) = the position of document i inside its own group
                s[i] = h[rank(i)] @ W_{head(i)}^T + b_{head(i)}          head(i) = 1 for a truthy domain, 2 otherwise
            document i is scored from the rows of document rank(i), not its own.  Single-domain batch: rank(i) = i.
    lstm    a single-domain batch runs RNN('model_1.') (all truthy) or RNN('model_2.'), then the one head; a mixed batch raises upstream
    plain   BiLSTM: RNN('model.') and the one head; domains are ignored

    loss / decode: oracle.restatement.tagger_loss / greedy_decode (row i un-padded by lengths[i] against tags[i], as BiLSTM)
"""
from typing import Dict, List, Sequence, Tuple

import torch
from torch import Tensor

from oracle.restatement import rnn_forward
from tests.helpers import bilstm_param_shapes


def param_shapes(D, H, NL, n_out, mode):
    if mode == 'lstm':
        s = bilstm_param_shapes(D, H, NL, n_out, prefix='model_1.')
        s.update(bilstm_param_shapes(D, H, NL, n_out, prefix='model_2.'))
        heads = ('classification',)
    else:
        s = bilstm_param_shapes(D, H, NL, n_out, prefix='model.')
        heads = ('classification_1', 'classification_2') if mode == 'dense' else ('classification',)
    for h in heads:
        s[h + '.weight'] = (n_out, 2 * H)
        s[h + '.bias'] = (n_out,)
    return s


def rank_map(domains: Sequence) -> Tuple[List[int], List[int]]:
    """document i -> (rank(i) = the document whose encoder rows it is scored from, head(i) - 1)"""
    idx1 = [i for i, d in enumerate(domains) if d]
    idx2 = [i for i, d in enumerate(domains) if not d]
    src = [0] * len(domains)
    for k, i in enumerate(idx1):
        src[i] = k
    for k, i in enumerate(idx2):
        src[i] = k
    return src, [0 if d else 1 for d in domains]


def unread_params(p: Dict[str, Tensor], domains: Sequence, mode: str) -> List[str]:
    """The parameters a batch does not read (their grad stays None upstream)."""
    truthy = [bool(d) for d in domains]
    if all(truthy) or not any(truthy):
        if mode == 'dense':
            other = 'classification_2.' if truthy[0] else 'classification_1.'
            return sorted(n for n in p if n.startswith(other))
        if mode == 'lstm':
            other = 'model_2.' if truthy[0] else 'model_1.'
            return sorted(n for n in p if n.startswith(other))
    return []


def scores(x: Tensor, lengths: Tensor, domains: Sequence, p: Dict[str, Tensor], mode: str, batched: bool = True) -> Tensor:
    """Every row [B, max(len), n_out] (dropout 0)."""
    truthy = [bool(d) for d in domains]
    if mode == 'lstm':
        if any(truthy) and not all(truthy):
            raise AttributeError("'list' object has no attribute 'data'")
        pre = 'model_1.' if truthy[0] else 'model_2.'
    else:
        pre = 'model.'
    NL = sum(1 for k in p if k.startswith(pre + 'rnn.weight_hh_l') and not k.endswith('_reverse'))
    h = rnn_forward(x, lengths, p, pre, NL, True, batched)
    if mode != 'dense':
        return h @ p['classification.weight'].t() + p['classification.bias']
    src, head = rank_map(domains)
    rows = []
    for i in range(h.shape[0]):
        name = 'classification_1' if head[i] == 0 else 'classification_2'
        rows.append(h[src[i]] @ p[name + '.weight'].t() + p[name + '.bias'])
    return torch.stack(rows)
