"""Oracle of the CRF posterior-marginal decode (mts_crf_marginals): a log-domain forward-backward on the CPU, fp64 unless asked otherwise.

The recursion is the reference's forward algorithm (models/CRF.py:218-240, restated in oracle.restatement.crf_forward_score) and its mirror
image: with alpha_0 the START one-hot in the -1e4 convention,

    alpha_{t+1}(i) = lse_j(alpha_t(j) + T[i][j]) + f_t(i)          beta_n(i) = T[stop][i]
    beta_t(j)      = lse_i(T[i][j] + f_t(i) + beta_{t+1}(i))       lm_t(i)   = alpha_{t+1}(i) + beta_{t+1}(i) - log Z

Only steps t < n_b move a document's recursion.  ``marginals`` returns the UNCLAMPED logit lm_t(cls) - lse_{i != cls} lm_t(i) (0 past a
document's length), log Z and the log-marginals themselves; ``brute_force`` enumerates every path of one document.
"""
import itertools

import torch

from oracle import restatement as R

CLAMP = 80.0


def marginals(feats, lengths, trans, cls, dtype=torch.float64):
    """feats [B, L, C], lengths (list, or None = all L), trans [C, C], cls in 0..C-1
    -> (logit [B, L] unclamped and 0 past each length, logz [B], lm [B, L, C] log-marginals, 0 past each length), all in ``dtype``."""
    B, L, C = feats.shape
    start, stop = C - 2, C - 1
    f, T = feats.to(dtype), trans.to(dtype)
    n = torch.full((B,), L, dtype=torch.long) if lengths is None else torch.as_tensor(lengths, dtype=torch.long).clamp(0, L)
    a = f.new_full((B, C), R.IMPOSSIBLE)
    a[:, start] = 0.0
    alphas = [a]
    for t in range(L):
        nxt = torch.logsumexp(a.unsqueeze(1) + T.unsqueeze(0), dim=-1) + f[:, t]          # [B, C(to)] over C(from)
        a = torch.where((t < n).unsqueeze(1), nxt, a)
        alphas.append(a)
    logz = torch.logsumexp(a + T[stop], dim=-1)
    beta = T[stop].unsqueeze(0).expand(B, C).clone()
    lm = f.new_zeros(B, L, C)
    for t in range(L - 1, -1, -1):
        live = (t < n).unsqueeze(1)
        lm[:, t] = torch.where(live, alphas[t + 1] + beta - logz.unsqueeze(1), lm[:, t])
        prev = torch.logsumexp(T.unsqueeze(0) + (f[:, t] + beta).unsqueeze(2), dim=1)      # over i (to), for every j (from)
        beta = torch.where(live, prev, beta)
    others = [i for i in range(C) if i != cls]
    logit = lm[:, :, cls] - torch.logsumexp(lm[:, :, others], dim=-1)
    valid = torch.arange(L).unsqueeze(0) < n.unsqueeze(1)
    return torch.where(valid, logit, torch.zeros_like(logit)), logz, lm


def clamped(logit):
    return logit.clamp(-CLAMP, CLAMP)


def brute_force(feats, trans, cls):
    """One document feats [n, C] in fp64, every one of the C^n paths (START / STOP tags included, at their -1e4 transitions)
    -> (logit [n] of tag ``cls``, log Z)."""
    n, C = feats.shape
    start, stop = C - 2, C - 1
    f, T = feats.double(), trans.double()
    paths = list(itertools.product(range(C), repeat=n))
    scores = torch.empty(len(paths), dtype=torch.float64)
    for k, path in enumerate(paths):
        s, prev = 0.0, start
        for t, y in enumerate(path):
            s = s + float(T[y, prev]) + float(f[t, y])
            prev = y
        scores[k] = s + float(T[stop, prev])
    logz = torch.logsumexp(scores, dim=0)
    tags = torch.tensor(paths, dtype=torch.long).view(len(paths), n)
    logit = torch.empty(n, dtype=torch.float64)
    for t in range(n):
        on = tags[:, t] == cls
        logit[t] = torch.logsumexp(scores[on], dim=0) - torch.logsumexp(scores[~on], dim=0)
    return logit, logz
