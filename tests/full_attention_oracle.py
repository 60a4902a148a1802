"""fp64 restatement of Transformer_segmenter(restricted=False): the BertModel of Classic_Transformer
(models/RestrictedTransformerLayer.py:16-63, models/CRF.py:543-549) and its full self-attention.

Differences from oracle.restatement.band_encoder: positions 0..L-1 (no Longformer padding offset), every valid key of the
document (j < len_b) in each softmax, padded keys probability exactly 0 (BERT adds finfo.min to their scores), padded query rows
NOT zeroed.  The LayerNorm, GELU and loss tail are oracle.restatement's.
"""
import math
from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor

from oracle.restatement import gelu_erf, layer_norm, tagger_loss  # noqa: F401  (tagger_loss re-exported for the tests)


def full_attention(q: Tensor, k: Tensor, v: Tensor, lengths: Tensor, keep: Optional[Tensor] = None, return_lse: bool = False):
    """q, k, v: [B, L, heads, hd], q already scaled by 1/sqrt(hd).  Softmax over keys j < len_b for every query row (padded rows
    included).  keep (optional, [B, L(query), heads, L(key)]): attention dropout -- multiplies the probabilities before they weight V
    (pass the keep mask times 1/(1-p)).  return_lse: also return log sum_j exp(s_ij) as [B, L, heads]."""
    B, L, H, hd = q.shape
    s = torch.einsum('bihd,bjhd->bihj', q, k)                                   # [B, Lq, H, Lk]
    key_ok = torch.arange(L).view(1, L) < lengths.view(B, 1).clamp(max=L)
    s = s.masked_fill(~key_ok.view(B, 1, 1, L), float('-inf'))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    if keep is not None:
        p = p * keep
    ctx = torch.einsum('bihj,bjhd->bihd', p, v)
    return (ctx, lse) if return_lse else ctx


def full_encoder(x: Tensor, lengths: Tensor, p: Dict[str, Tensor], heads: int, num_layers: int, prefix: str = 'model.model.',
                 ln_eps: float = 1e-12, keeps=None) -> Tensor:
    """BertModel(inputs_embeds=x, attention_mask=valid) in eval mode: x + pos_emb[i] + type_emb[0] -> LayerNorm; per layer
    q = (Wq h + b) / sqrt(hd), k, v, full attention, a = LN(Wo ctx + b + h), h' = LN(W2 gelu(W1 a + b) + b + a).
    keeps (optional): per layer, the attention-dropout factor of full_attention (training mode)."""
    B, L, D = x.shape
    hd = D // heads
    e = prefix + 'embeddings.'
    h = x + p[e + 'position_embeddings.weight'][:L].unsqueeze(0) + p[e + 'token_type_embeddings.weight'][0]
    h = layer_norm(h, p[e + 'LayerNorm.weight'], p[e + 'LayerNorm.bias'], ln_eps)
    for li in range(num_layers):
        lp = f'{prefix}encoder.layer.{li}.'
        a = lp + 'attention.self.'
        q = (h @ p[a + 'query.weight'].t() + p[a + 'query.bias']) / math.sqrt(hd)
        k = h @ p[a + 'key.weight'].t() + p[a + 'key.bias']
        v = h @ p[a + 'value.weight'].t() + p[a + 'value.bias']
        ctx = full_attention(q.view(B, L, heads, hd), k.view(B, L, heads, hd), v.view(B, L, heads, hd), lengths,
                             keep=keeps[li] if keeps else None).reshape(B, L, D)
        o = lp + 'attention.output.'
        a1 = layer_norm(ctx @ p[o + 'dense.weight'].t() + p[o + 'dense.bias'] + h, p[o + 'LayerNorm.weight'], p[o + 'LayerNorm.bias'], ln_eps)
        f = gelu_erf(a1 @ p[lp + 'intermediate.dense.weight'].t() + p[lp + 'intermediate.dense.bias'])
        h = layer_norm(f @ p[lp + 'output.dense.weight'].t() + p[lp + 'output.dense.bias'] + a1,
                       p[lp + 'output.LayerNorm.weight'], p[lp + 'output.LayerNorm.bias'], ln_eps)
    return h


def full_scores(x: Tensor, lengths: Tensor, p: Dict[str, Tensor], heads: int, num_layers: int, keeps=None) -> Tensor:
    """Transformer_segmenter(restricted=False): encoder -> Linear(D -> 1|2), on every row (padded rows included)."""
    return full_encoder(x, lengths, p, heads, num_layers, keeps=keeps) @ p['classification.weight'].t() + p['classification.bias']


def keep_mask(n: int, p: float, seed: int) -> np.ndarray:
    """Host replica of the kernels' keep decision: mts_hash32(seed, idx) >= threshold for idx = 0..n-1 (include/mts.h, full attention)."""
    idx = np.arange(1, n + 1, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * idx
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    thr = int(max(1.0, min(4294967295.0, float(np.float32(p)) * 4294967296.0)))
    return (z >> np.uint64(32)) >= np.uint64(thr)
