"""Plain python / numpy statements of the WinPR sweep (include/mts.h, mts_winpr_sweep), in three forms that must agree exactly:

    via_metrics(h, t, k)      (precision, recall, f1) by metrics.WinPR(reference=h, hypothesis=t, k) on integer lists, with the sweep's
                              convention (0, 0, 0) where metrics.WinPR raises ZeroDivisionError (threshold_search.py)
    counts_literal(h, t, k)   {TP, FP, FN} by WinPR's own loop over python slices (wrap-around for a negative start included)
    counts_closed(h, t, k)    {TP, FP, FN} by the closed form of include/mts.h: two prefix-count differences per window and one bit

`h`: the hypothesis AFTER the threshold (0 / 1 per sentence of one document), `t`: the target, 0 / 1 per sentence -- both as `operands`
leaves them (under end_boundary the last sentence of both is 0; nothing else is cleared).
"""
import numpy as np

from multimodaltopicsegmentation_amd import metrics


def operands(tags, target, end_boundary=False):
    """integer lists as the scaiano branch of TextSegmenter.test_step hands them to WinPR"""
    h = [int(bool(v)) for v in tags]
    t = [int(v == 1) for v in np.asarray(target).tolist()]
    assert len(h) == len(t)
    if end_boundary and h:
        h[-1] = 0
        t[-1] = 0
    return h, t


def counts_literal(h, t, k=10):
    n = len(h)
    if n == 0:
        return (0, 0, 0)
    tp = fp = fn = 0
    last_r = last_c = None
    for i in range(1 - k, n + 1):
        pr = 1 if (last_r is not None and len(last_r) > 0 and last_r[0] == 1) else 0
        pc = 1 if (last_c is not None and len(last_c) > 0 and last_c[0] == 1) else 0
        last_r, last_c = h[i:i + k], t[i:i + k]
        R, C = sum(h[max(i, 0):i + k]) + pr, sum(t[max(i, 0):i + k]) + pc
        tp, fp, fn = tp + min(R, C), fp + max(0, C - R), fn + max(0, R - C)
    return (tp, fp, fn)


def _prev(a, n, k, i):
    if i == 1 - k:
        return 0
    if i >= 1:
        return a[i - 1]
    lo, hi = max(n + i - 1, 0), min(i - 1 + k, n)
    return a[lo] if lo < hi else 0


def counts_closed(h, t, k=10):
    n = len(h)
    if n == 0:
        return (0, 0, 0)
    ph, pt = np.concatenate([[0], np.cumsum(h)]), np.concatenate([[0], np.cumsum(t)])     # pos(x) = boundaries strictly before x, x = 0 .. n
    tp = fp = fn = 0
    for i in range(1 - k, n + 1):
        lo, hi = max(i, 0), min(i + k, n)
        R = int(ph[hi] - ph[lo]) + _prev(h, n, k, i)
        C = int(pt[hi] - pt[lo]) + _prev(t, n, k, i)
        tp, fp, fn = tp + min(R, C), fp + max(0, C - R), fn + max(0, R - C)
    return (tp, fp, fn)


def wrap_prevs(a, k=10):
    """how many of the windows 2-k <= i <= 0 take a non-zero `prev` through python's wrap-around (possible only for len(a) < k)"""
    n = len(a)
    return sum(1 for i in range(2 - k, 1) if _prev(a, n, k, i) != 0) if n else 0


def floats(c):
    """(precision, recall, f1) from {TP, FP, FN} by metrics.WinPR's expressions; (0, 0, 0) in the three degenerate classes"""
    tp, fp, fn = (int(v) for v in c)
    if tp + fp == 0 or tp + fn == 0 or tp == 0:
        return (0.0, 0.0, 0.0)
    p, r = tp / (tp + fp), tp / (tp + fn)
    return (p, r, 2 * (p * r / (p + r)))


def degenerate(c):
    tp, fp, fn = (int(v) for v in c)
    return tp + fp == 0 or tp + fn == 0 or tp == 0


def via_metrics(h, t, k=10):
    if len(h) == 0:
        return (0.0, 0.0, 0.0)
    try:
        p, r, f = metrics.WinPR(list(h), list(t), k=k)
    except ZeroDivisionError:
        return (0.0, 0.0, 0.0)
    return (float(p), float(r), float(f))


def mean_table(per_doc, thresholds):
    """per_doc: list over documents of [T][3] (P, R, F) -> the table, summed document after document as test_step's `+=`"""
    out = {'thresholds': list(thresholds), 'b_precision': [], 'b_recall': [], 'b_f1': []}
    for j in range(len(thresholds)):
        s = [0.0, 0.0, 0.0]
        for doc in per_doc:
            for c in range(3):
                s[c] += doc[j][c]
        for c, key in enumerate(('b_precision', 'b_recall', 'b_f1')):
            out[key].append(s[c] / len(per_doc))
    return out


def select(table):
    """lightning_model.py:493-508 with the fallback of :546-551"""
    best, best_idx, best_th = -1, 0, None
    for idx, th in enumerate(table['thresholds']):
        if table['b_f1'][idx] > best:
            best, best_idx, best_th = table['b_f1'][idx], idx, th
    return {'b_precision': float(table['b_precision'][best_idx]), 'b_recall': float(table['b_recall'][best_idx]),
            'valid_loss': float(table['b_f1'][best_idx]), 'threshold': 0.4 if best_th is None else float(best_th)}
