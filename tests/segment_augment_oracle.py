"""Host statement of segment-order augmentation in plain numpy / torch, independent of the package: what
``ResidentCorpus.batch_segments`` and ``AugmentedCorpus`` must produce.  No GPU, no import of the product.

A document of n rows with labels y in {0, 1}: segment ends are [t + 1 for t < n if y[t] == 1], plus n if it is not the last entry; segment j
is the rows between consecutive ends, *closed* if it ends in a label 1 and otherwise the *tail* (only the last segment can be one)."""
import numpy as np
import torch


def segment_ends(labels):
    labels = [int(v) for v in labels]
    n = len(labels)
    ends = [t + 1 for t in range(n) if labels[t] == 1]
    if n and (not ends or ends[-1] != n):
        ends.append(n)
    return ends


def segment_ranges(labels):
    """-> [(first row, end row, closed)] per segment"""
    ends = segment_ends(labels)
    return [(a, b, int(labels[b - 1]) == 1) for a, b in zip([0] + ends[:-1], ends)]


def augment_document(emb, labels, order, close_last):
    """-> (rows of the listed segments in that order, labels: 0 but for a 1 on the last row of every listed segment, and ``close_last`` on
    the very last row)"""
    seg = segment_ranges(labels)
    order = [int(j) for j in order]
    assert order and len(set(order)) == len(order) and all(0 <= j < len(seg) for j in order)
    emb = torch.as_tensor(emb)
    rows, lab = [], []
    for j in order:
        a, b, _ = seg[j]
        rows.append(emb[a:b])
        lab += [0.0] * (b - a - 1) + [1.0]
    lab[-1] = 1.0 if close_last else 0.0
    return torch.cat(rows), torch.tensor(lab, dtype=torch.float32)


def reverse_rule(labels):
    """-> (order, close_last) of mode 'reverse': the closed segments in descending order, the tail left out, the last label 1 (the
    reference, utils/load_datasets_precomputed.py:71-96).  A document without a closed segment keeps itself: ([0], False)."""
    closed = [j for j, (_, _, c) in enumerate(segment_ranges(labels)) if c]
    if not closed:
        return [0], False
    return closed[::-1], True


def shuffle_rule(labels, seed, epoch, d):
    """-> (order, close_last) of mode 'shuffle' for stored document d"""
    return np.random.default_rng([seed, epoch, d]).permutation(len(segment_ends(labels))).tolist(), False


def identity_rule(labels):
    """the stored document itself: every segment in place and its own last label"""
    seg = segment_ranges(labels)
    return list(range(len(seg))), seg[-1][2]


def augmented_segments(aug_labels, length):
    return [t + 1 for t in range(int(length)) if float(aug_labels[t]) == 1.0]


def padded_batch(docs, Lmax, pad, dtype=None):
    """list of [n, D] (or [n]) host tensors -> [B, Lmax(, D)] cut / padded to Lmax"""
    out = torch.full((len(docs), Lmax) + tuple(docs[0].shape[1:]), pad, dtype=docs[0].dtype)
    for b, t in enumerate(docs):
        n = min(int(t.shape[0]), Lmax)
        out[b, :n] = t[:n]
    return out if dtype is None else out.to(dtype)
