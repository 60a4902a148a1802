"""Host oracle of negative-sentence masking (include/mts.h mts_mask_plan, mts_gather_rows; resident.MaskedCorpus), written from the rule,
in plain Python and NumPy: the counter hash is tests/bootstrap_oracle.hash32 (the replica of common.h's mts_hash32), the keep decision is
taken row by row and the compaction is an explicit loop -- nothing of the product's vectorised plan is used.  It is the project's own
rule; upstream's draw (NumPy reseeded with 1 for every document) is not reproduced."""
import torch

from tests.bootstrap_oracle import hash32

M64 = (1 << 64) - 1


def threshold(p):
    """T = clamp((uint64)(p * 2^32), 0, 2^32), in double"""
    return max(0, min(int(float(p) * 4294967296.0), 1 << 32))


def doc_seed(seed, epoch, n_docs, d):
    """(hash32(seed, 2c) << 32) | hash32(seed, 2c + 1), c = epoch * n_docs + d"""
    c = (int(epoch) * int(n_docs) + int(d)) & M64
    s = int(seed) & M64
    hi, lo = (int(v) for v in hash32(s, [(2 * c) & M64, (2 * c + 1) & M64]))
    return (hi << 32) | lo


def kept_rows(labels, dseed, p):
    """-> the indices of the rows of a document that masking keeps, ascending: a row stays when its label is not 0 or when its hash falls
    below the threshold; row 0 when none does"""
    T = threshold(p)
    n = len(labels)
    h = [int(v) for v in hash32(int(dseed), list(range(n)))] if n else []
    kept = []
    for r in range(n):
        if float(labels[r]) != 0.0 or h[r] < T:
            kept.append(r)
    if n and not kept:
        kept = [0]
    return kept


def plan(labels, dseed, p, Lmax):
    """-> (src_row of one batch row [Lmax], kept): the first Lmax kept rows, -1 behind them; the count is not clipped"""
    rows = kept_rows(labels, dseed, p)
    out = [-1] * Lmax
    for t, r in enumerate(rows):
        if t < Lmax:
            out[t] = r
    return out, len(rows)


def mask_document(emb, labels, dseed, p):
    """-> (kept rows of emb, their labels as an fp32 tensor): what upstream pops together stays together"""
    rows = kept_rows(labels, dseed, p)
    emb = torch.as_tensor(emb)
    lab = torch.tensor([float(labels[r]) for r in rows], dtype=torch.float32)
    if not rows:
        return emb[:0], lab
    return torch.stack([emb[r] for r in rows]), lab


def segments(labels, length):
    """src_segments of a document with these (masked) labels: the positions just behind the ones inside the reported length"""
    return [t + 1 for t in range(int(length)) if float(labels[t]) == 1.0]


def gather_rows(corpus, row_start, doc_index, src_row, pad, dtype=None):
    """mts_gather_rows on the host: corpus [total_rows(, D)], src_row a list of B lists of Lmax entries -> [B, Lmax(, D)]; an entry that
    is negative or outside its document, and every row of an index outside the corpus, is pad"""
    B, Lmax = len(src_row), len(src_row[0])
    n_docs = len(row_start) - 1
    out = torch.full((B, Lmax) + tuple(corpus.shape[1:]), pad, dtype=corpus.dtype)
    for b in range(B):
        d = int(doc_index[b])
        if not 0 <= d < n_docs:
            continue
        s, n = int(row_start[d]), int(row_start[d + 1]) - int(row_start[d])
        for t in range(Lmax):
            e = int(src_row[b][t])
            if 0 <= e < n:
                out[b, t] = corpus[s + e]
    return out if dtype is None else out.to(dtype)
