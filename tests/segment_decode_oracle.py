"""Host restatement of mts_segment_decode (include/mts.h), written from the header: python integers and numpy, no GPU, no package code.

    fixed_point(prob, threshold)      -> q [n] int64:  rint(prob * 2^32) - rint(threshold * 2^32), half to even, in float64 (exact)
    constrained_tags(q, m, last_tag)  -> tags uint8 [n]: the recurrence and the walk back of the header
    brute_force(q, m)                 -> (the optimum of sum_{t in S} q_t over ALL admissible sets S, the number of sets tried)
    admissible(tags, m)               -> every segment but possibly none holds at least m sentences (the interior tags' constraint)
    segment_table(tags, n, close_last, Smax) -> (seg_end int32 [Smax], n_seg)
    decode(prob, lengths, threshold, m, close_last, Smax) -> (tags [B, L], seg_end [B, Smax], n_seg [B]) for a padded batch
"""
import itertools

import numpy as np

TWO32 = 4294967296.0


def fixed_point(prob, threshold):
    """prob: float32 [n]; threshold: a python float holding a float32 value.  np.rint rounds half to even; float32 * 2^32 is exact in
    float64 and below 2^53."""
    p = np.rint(np.asarray(prob, dtype=np.float32).astype(np.float64) * TWO32).astype(np.int64)
    return p - np.int64(np.rint(float(np.float32(threshold)) * TWO32))


def constrained_tags(q, m, last_tag):
    """the header's rule for min_segment = m >= 1 over the weights q (integers): interior boundaries at t in [m-1, n-1-m], the last
    sentence's tag given.  m == 1 is not special here: the recurrence then takes exactly the positive weights (tests hold it to q > 0)."""
    q = [int(v) for v in q]
    n = len(q)
    tags = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return tags
    lo, hi = m - 1, n - 1 - m
    best, take = {}, {}

    def B(u):
        return best[u] if u >= lo else 0
    for t in range(lo, hi + 1):
        cand = q[t] + B(t - m)
        take[t] = cand > B(t - 1)
        best[t] = max(B(t - 1), cand)
    t = hi
    while t >= lo:
        while t >= lo and not take[t]:
            t -= 1
        if t < lo:
            break
        tags[t] = 1
        t -= m
    tags[n - 1] = 1 if last_tag else 0
    return tags


def dp_value(q, m):
    """sum of q over the interior boundaries constrained_tags picks"""
    tags = constrained_tags(q, m, False)
    return int(sum(int(v) for v, t in zip(q, tags) if t))


def admissible_sets(n, m):
    """every subset of [m-1, n-1-m] whose members are at least m apart"""
    span = list(range(m - 1, n - m))
    for k in range(len(span) + 1):
        for s in itertools.combinations(span, k):
            if all(b - a >= m for a, b in zip(s, s[1:])):
                yield s


def brute_force(q, m):
    best, tried = None, 0
    for s in admissible_sets(len(q), m):
        v = sum(int(q[t]) for t in s)
        best = v if best is None or v > best else best
        tried += 1
    return best, tried


def admissible(tags, m):
    """the interior boundaries of ``tags`` (all but the last sentence's) lie in [m-1, n-1-m] and at least m apart"""
    n = len(tags)
    inner = [int(i) for i in np.flatnonzero(np.asarray(tags)[:max(n - 1, 0)])]
    return all(m - 1 <= t <= n - 1 - m for t in inner) and all(b - a >= m for a, b in zip(inner, inner[1:]))


def segment_table(tags, n, close_last, Smax):
    ends = [int(i) + 1 for i in np.flatnonzero(np.asarray(tags)[:n])]
    if close_last and n > 0 and not tags[n - 1]:
        ends.append(n)
    out = np.full(Smax, -1, dtype=np.int32)
    k = min(len(ends), Smax)
    out[:k] = ends[:k]
    return out, len(ends)


def decode(prob, lengths, threshold, m, close_last, Smax):
    """prob float32 [B, L] as the device wrote it; lengths: ints (clamped to 0..L) or None"""
    prob = np.asarray(prob, dtype=np.float32)
    B, L = prob.shape
    th = np.float32(threshold)
    tags = np.zeros((B, L), dtype=np.uint8)
    seg_end = np.empty((B, Smax), dtype=np.int32)
    n_seg = np.empty(B, dtype=np.int32)
    for b in range(B):
        n = L if lengths is None else min(max(int(lengths[b]), 0), L)
        p = prob[b, :n]
        if m == 1:
            tags[b, :n] = p > th
        elif n:
            tags[b, :n] = constrained_tags(fixed_point(p, th), m, bool(p[n - 1] > th))
        seg_end[b], n_seg[b] = segment_table(tags[b], n, close_last, Smax)
    return tags, seg_end, n_seg
