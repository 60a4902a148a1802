"""fp64 restatement of the tagger tail as the C ABI describes it (include/mts.h: mts_tagger_loss, mts_greedy_decode, mts_layernorm_loss_tail), written
from the header and oracle.restatement (layer_norm, tagger_loss, sigmoid_focal_loss, bce_on_probs, cross_entropy_ignore, greedy_decode).  Plain torch on
the CPU; it never calls the library.

    batch:   B documents of at most L sentences; targets [B, Lt], Lt >= L (columns at or past L are never read); lengths [B] or None (= L each)
    rows:    padded layout: row r is sentence (b, i) = (r // L, r % L), N = B * L rows
             packed layout: row r is sentence row_src[r] = b * L + i, N = len(row_src) rows (document after document, every row inside its document)
    BCE / focal (n_out = 1): the rows with i < len_b are averaged (the un-pad loop of models/CRF.py:348-350); count = sum of min(max(len_b, 0), L)
    CrossEntropy (n_out = 2..4): the rows whose target is not -1 are averaged (ignore_index = -1, models/CRF.py:298); count = their number
    loss = sum of the row terms / count, or 0 when count == 0; every other row has gradient exactly 0
    tail:    scores = LN(x; gamma, beta, eps) @ head_w^T + head_b, the loss over those scores, gradients of grad_scale * loss by autograd
    decode:  p = sigmoid(score) (n_out = 1) or softmax(scores)[1] (n_out = 2..4); tag = p > threshold (strict) inside the document, 0 past its length
"""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

CE, BCE, FOCAL = 0, 1, 2                     # MTS_LOSS_* of include/mts.h
KIND_NAMES = {CE: 'CrossEntropy', BCE: 'BinaryCrossEntropy', FOCAL: 'FocalLoss'}


def row_sentences(B: int, L: int, row_src: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """-> (document b, position i) of every row"""
    src = torch.arange(B * L) if row_src is None else row_src.long()
    return src // L, src % L


def pack_rows(lengths: Sequence[int], L: int) -> Tensor:
    """row_src of the packed form of a batch: the valid sentences, document after document"""
    return torch.cat([b * L + torch.arange(int(n)) for b, n in enumerate(lengths)]).to(torch.int32)


def layer_norm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float) -> Tensor:
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma + beta


def focal_terms(x: Tensor, y: Tensor, alpha: float, gamma_f: float) -> Tensor:
    """models/focal_loss.py:38-57 per element"""
    p = torch.sigmoid(x)
    ce = (1 - y) * x - torch.nn.functional.logsigmoid(x)
    p_t = p * y + (1 - p) * (1 - y)
    t = ce * (1 - p_t) ** gamma_f
    if alpha >= 0:
        t = (alpha * y + (1 - alpha) * (1 - y)) * t
    return t


def bce_terms(x: Tensor, y: Tensor) -> Tensor:
    """nn.BCELoss(sigmoid(x), y) per element, both logs clamped at -100 (models/CRF.py:303; oracle.restatement.bce_on_probs).  A clamped log passes
    no gradient, as the header's kernels state it; written with torch.where so that a probability that is exactly 1 in the number format (x = 40)
    gives that 0 instead of the 0 / 0 that log(1 - p).clamp(min=-100) hands autograd."""
    p = torch.sigmoid(x)

    def clamped_log(q):
        ok = q > math.exp(-100.0)
        return torch.where(ok, torch.log(torch.where(ok, q, torch.ones_like(q))), torch.full_like(q, -100.0))
    return -(y * clamped_log(p) + (1 - y) * clamped_log(1 - p))


def ce_terms(x: Tensor, t: Tensor) -> Tensor:
    """-log softmax(x)[t] per row; x [n, n_out], t long [n]"""
    return torch.logsumexp(x, dim=-1) - x.gather(1, t.unsqueeze(1)).squeeze(1)


def averaged_rows(targets: Tensor, lengths: Optional[Tensor], kind: int, batch_shape, row_src: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, int]:
    """-> (bool [N]: the row is averaged, the target of every row [N], count).  count follows the header: from the lengths alone for BCE / focal (a
    packed batch that leaves valid sentences out would still be divided by all of them), from the targets of the rows for CrossEntropy."""
    B, L = batch_shape
    b, i = row_sentences(B, L, row_src)
    y = targets[b, i]
    if kind == CE:
        use = y != -1
        return use, y, int(use.sum())
    ln = torch.full((B,), L, dtype=torch.long) if lengths is None else lengths.long()
    return i < ln[b], y, int(ln.clamp(0, L).sum())


def masked_loss(scores: Tensor, targets: Tensor, lengths: Optional[Tensor], kind: int, alpha: float, gamma_f: float, batch_shape,
                row_src: Optional[Tensor] = None) -> Tuple[Tensor, int]:
    """scores [N, n_out] -> (loss 0-d, count); differentiable in scores"""
    use, y, count = averaged_rows(targets, lengths, kind, batch_shape, row_src)
    x = scores.reshape(-1, scores.shape[-1])[use]
    y = y[use]
    if kind == CE:
        terms = ce_terms(x, y.long())
    elif kind == FOCAL:
        terms = focal_terms(x[:, 0], y.to(x.dtype), alpha, gamma_f)
    elif kind == BCE:
        terms = bce_terms(x[:, 0], y.to(x.dtype))
    else:
        raise ValueError('Choose one of CrossEntropy or BinaryCrossEntropy as loss function')      # models/CRF.py:312
    total = terms.sum()
    return (total / count if count > 0 else total * 0.0), count


def loss_reference(scores: Tensor, targets: Tensor, lengths: Optional[Tensor], kind: int, alpha: float = 0.9, gamma_f: float = 2.0, batch_shape=None,
                   row_src: Optional[Tensor] = None) -> Dict[str, object]:
    """mts_tagger_loss.  scores [B, L, n_out] (batch_shape may be None) or, packed, [n_rows, n_out] with row_src and batch_shape = (B, L).
    -> {'loss': float, 'count': int, 'dscores': fp64, shaped as scores}"""
    if batch_shape is None:
        batch_shape = tuple(scores.shape[:2])
    s = scores.detach().double().requires_grad_(True)
    loss, count = masked_loss(s, targets.double(), lengths, kind, alpha, gamma_f, batch_shape, row_src)
    (ds,) = torch.autograd.grad(loss, s, allow_unused=True)
    return dict(loss=loss.item(), count=count, dscores=torch.zeros_like(s) if ds is None else ds)


def tail_reference(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, head_w: Tensor, head_b: Tensor, targets: Tensor, lengths: Optional[Tensor],
                   kind: int, alpha: float, gamma_f: float, grad_scale: float, batch_shape, row_src: Optional[Tensor] = None,
                   dtype=torch.float64) -> Dict[str, object]:
    """mts_layernorm_loss_tail.  x [rows, D] -> scores [rows, n_out], loss, count and the gradients of grad_scale * loss wrt x, gamma, beta, head_w,
    head_b.  dtype = torch.float32 evaluates the same formula in fp32 (to measure what the number format alone costs)."""
    leaf = lambda t: t.detach().to(dtype).requires_grad_(True)
    xv, gv, bv, wv, hbv = leaf(x), leaf(gamma), leaf(beta), leaf(head_w), leaf(head_b)
    scores = layer_norm(xv, gv, bv, eps) @ wv.t() + hbv
    loss, count = masked_loss(scores, targets.to(dtype), lengths, kind, alpha, gamma_f, batch_shape, row_src)
    grads = torch.autograd.grad(grad_scale * loss, [xv, gv, bv, wv, hbv], allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, (xv, gv, bv, wv, hbv))]
    return dict(scores=scores.detach(), loss=loss.item(), count=count, dx=grads[0], dgamma=grads[1], dbeta=grads[2], dhead_w=grads[3], dhead_b=grads[4])


def tail_backward_reference(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, head_w: Tensor, head_b: Tensor, dscores: Tensor) -> Dict[str, Tensor]:
    """The backward half alone, for a given d loss / d scores [rows, n_out]: gradients of sum(scores * dscores) in fp64."""
    leaf = lambda t: t.detach().double().requires_grad_(True)
    xv, gv, bv, wv, hbv = leaf(x), leaf(gamma), leaf(beta), leaf(head_w), leaf(head_b)
    scores = layer_norm(xv, gv, bv, eps) @ wv.t() + hbv
    grads = torch.autograd.grad((scores * dscores.double()).sum(), [xv, gv, bv, wv, hbv])
    return dict(scores=scores.detach(), dx=grads[0], dgamma=grads[1], dbeta=grads[2], dhead_w=grads[3], dhead_b=grads[4])


def decode_reference(scores: Tensor, lengths: Optional[Tensor], threshold: float) -> Tuple[Tensor, Tensor]:
    """mts_greedy_decode (models/CRF.py:362-369; softmax class 1 for n_out 3 and 4 as for 2).  scores [B, L, n_out] -> (tags uint8 [B, L], zero past
    the length; probability fp64 [B, L])"""
    B, L, n_out = scores.shape
    s = scores.double()
    prob = torch.sigmoid(s[..., 0]) if n_out == 1 else torch.softmax(s, dim=-1)[..., 1]
    ln = torch.full((B,), L, dtype=torch.long) if lengths is None else lengths.long()
    valid = torch.arange(L).unsqueeze(0) < ln.unsqueeze(1)
    return ((prob > threshold) & valid).to(torch.uint8), prob


def decode_lists(tags: Tensor, lengths: Tensor) -> List[List[bool]]:
    """the list-of-lists form of oracle.restatement.greedy_decode"""
    return [tags[b, :int(n)].bool().tolist() for b, n in enumerate(lengths)]
