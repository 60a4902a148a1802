"""fp64 restatement of RecurrentLongT5 (models/CRF.py:613-762; the LongT5EncoderModel of models/RestrictedTransformerLayer.py:135-187).

Per block: RNN (oracle.restatement.rnn_forward, one bidirectional layer) -> one LongT5 encoder block on width d = 2H, eval mode:
    h = x;  h = h + o(attn(rms(h, w_ln0)));  h = h + wo(relu(wi(rms(h, w_ln1))));  out = rms(h, w_final)
with rms(x, w) = w * x / sqrt(mean(x^2) + 1e-6), and per head s_ij = q_i . k_j + T[bucket(j - i), h] (no 1/sqrt(d)):
valid query rows i < len_b softmax over j in [i - r, i + r], j < len_b; padded rows the uniform mean of v over their three blocks of
r + 1 rows divided by 3 (r + 1).  Then Linear(D -> 1) and the loss tail of oracle.restatement.
"""
import math
import zlib
from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor

from oracle.restatement import rnn_forward, tagger_loss  # noqa: F401  (tagger_loss re-exported for the tests)


def seeded_longt5_param(name, shape, seed):
    """tests/golden/make_golden_recurrent_longt5.py's recipe: helpers.seeded_param, except RMSNorm weights get 1 + 0.1 u."""
    from tests.helpers import seeded_param
    if name.endswith('layer_norm.weight'):
        rng = np.random.default_rng((zlib.crc32(name.encode()) + seed) & 0xFFFFFFFF)
        return 1.0 + 0.1 * rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    return seeded_param(name, shape, seed)


def param_shapes(D, H, heads, radius, NL):
    """Live state_dict keys of the reference's RecurrentLongT5 (BCE / focal head) and their shapes."""
    s, d, inner = {}, 2 * H, heads * 64
    for k in range(NL):
        for sfx in ('', '_reverse'):
            s[f'model.{k}.lstm.rnn.weight_ih_l0{sfx}'] = (4 * H, D)
            s[f'model.{k}.lstm.rnn.weight_hh_l0{sfx}'] = (4 * H, H)
            s[f'model.{k}.lstm.rnn.bias_ih_l0{sfx}'] = (4 * H,)
            s[f'model.{k}.lstm.rnn.bias_hh_l0{sfx}'] = (4 * H,)
        tp = f'model.{k}.transformer.model.encoder.'
        a = tp + 'block.0.layer.0.LocalSelfAttention.'
        for n in 'qkv':
            s[a + n + '.weight'] = (inner, d)
        s[a + 'o.weight'] = (d, inner)
        s[a + 'relative_attention_bias.weight'] = (max(4, radius), heads)
        s[tp + 'block.0.layer.0.layer_norm.weight'] = (d,)
        s[tp + 'block.0.layer.1.DenseReluDense.wi.weight'] = (d, d)
        s[tp + 'block.0.layer.1.DenseReluDense.wo.weight'] = (d, d)
        s[tp + 'block.0.layer.1.layer_norm.weight'] = (d,)
        s[tp + 'final_layer_norm.weight'] = (d,)
    s['classification.weight'] = (1, D)
    s['classification.bias'] = (1,)
    return s


def bucket_table(radius: int) -> Tensor:
    """Offsets -r..r -> bucket: HF's bidirectional _relative_position_bucket (fp32 log) with max(4, r) buckets, max distance r + 1."""
    nb = max(4, radius) // 2
    rp = torch.arange(-radius, radius + 1)
    ret = (rp > 0).to(torch.long) * nb
    rp = rp.abs()
    me = nb // 2
    large = me + (torch.log(rp.float() / me) / math.log((radius + 1) / me) * (nb - me)).to(torch.long)
    return ret + torch.where(rp < me, rp, torch.clamp(large, max=nb - 1))


def rms(x: Tensor, w: Tensor, eps: float = 1e-6) -> Tensor:
    return w * (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps))


def local_attention(q: Tensor, k: Tensor, v: Tensor, lengths: Tensor, radius: int, table: Tensor, bucket: Tensor,
                    keep: Optional[Tensor] = None, return_lse: bool = False):
    """q, k, v [B, L, heads, hd]; table [buckets, heads]; bucket [2r + 1] (offset -r..r).  keep (optional, [B, L, heads, 2r + 1],
    indexed by offset): the attention-dropout factor on valid rows.  -> ctx [B, L, heads, hd] (and lse [B, L, heads], 0 on padded rows)."""
    B, L, H, hd = q.shape
    r, blk = radius, radius + 1
    s = torch.einsum('bihd,bjhd->bhij', q, k)
    i = torch.arange(L).view(L, 1)
    j = torch.arange(L).view(1, L)
    off = j - i
    band = off.abs() <= r
    bias = table[bucket[(off.clamp(-r, r) + r)]]                              # [L, L, heads]
    s = s + bias.permute(2, 0, 1).unsqueeze(0).to(s.dtype)
    key_ok = (j.view(1, L) < lengths.view(B, 1)).view(B, 1, 1, L) & band.view(1, 1, L, L)
    s = s.masked_fill(~key_ok, float('-inf'))
    valid = (torch.arange(L).view(1, L) < lengths.view(B, 1))                  # [B, L] query rows
    s = s.masked_fill(~valid.view(B, 1, L, 1), 0.0)                            # padded rows: any finite value, replaced below
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    if keep is not None:
        kf = torch.zeros(B, H, L, L, dtype=p.dtype)
        for o in range(-r, r + 1):
            ii = torch.arange(max(0, -o), min(L, L - o))
            kf[:, :, ii, ii + o] = keep[:, ii, :, o + r].permute(0, 2, 1).to(p.dtype)
        p = p * kf
    ctx = torch.einsum('bhij,bjhd->bihd', p, v)
    # padded rows: uniform mean over [(i // blk - 1) blk, (i // blk + 2) blk) clipped to [0, L), divided by 3 blk
    lo = (torch.arange(L) // blk - 1) * blk
    win = ((j >= lo.view(L, 1)) & (j < lo.view(L, 1) + 3 * blk)).to(v.dtype) / (3 * blk)    # [L(query), L(key)]
    mean = torch.einsum('ij,bjhd->bihd', win, v)
    ctx = torch.where(valid.view(B, L, 1, 1), ctx, mean)
    lse = torch.where(valid.view(B, 1, L), lse, torch.zeros_like(lse)).permute(0, 2, 1)
    return (ctx, lse) if return_lse else ctx


def longt5_block(x: Tensor, lengths: Tensor, p: Dict[str, Tensor], prefix: str, heads: int, radius: int, keep=None) -> Tensor:
    """One LongT5 encoder block + final RMSNorm (eval mode, or training with attention dropout `keep` only)."""
    B, L, d = x.shape
    a = prefix + 'block.0.layer.0.LocalSelfAttention.'
    f = prefix + 'block.0.layer.1.'
    h = x
    n = rms(h, p[prefix + 'block.0.layer.0.layer_norm.weight'])
    q, k, v = (n @ p[a + s + '.weight'].t() for s in 'qkv')
    sh = (B, L, heads, 64)
    table = p[a + 'relative_attention_bias.weight']
    ctx = local_attention(q.view(sh), k.view(sh), v.view(sh), lengths, radius, table, bucket_table(radius), keep=keep)
    h = h + ctx.reshape(B, L, heads * 64) @ p[a + 'o.weight'].t()
    n = rms(h, p[f + 'layer_norm.weight'])
    h = h + torch.relu(n @ p[f + 'DenseReluDense.wi.weight'].t()) @ p[f + 'DenseReluDense.wo.weight'].t()
    return rms(h, p[prefix + 'final_layer_norm.weight'])


def recurrent_longt5_scores(x: Tensor, lengths: Tensor, p: Dict[str, Tensor], heads: int, radius: int, num_layers: int,
                            batched: bool = True) -> Tensor:
    """RecurrentLongT5 scores [B, max(len), 1] (padded rows included; dropout 0, eval mode)."""
    h = x
    for k in range(num_layers):
        h = rnn_forward(h, lengths, p, f'model.{k}.lstm.', 1, True, batched)
        h = longt5_block(h, lengths, p, f'model.{k}.transformer.model.encoder.', heads, radius)
    return h @ p['classification.weight'].t() + p['classification.bias']
