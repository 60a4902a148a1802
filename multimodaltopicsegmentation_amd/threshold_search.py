"""Decision-threshold search on the device (reference: models/lightning_model.py:435-553, the validation-epoch sweep that upstream
disabled by renaming the hook).

Every tagger that decodes by a threshold uses ``prob > th`` (SheikhBiLSTM: ``1 - prob < th``).  ``ThresholdSweep`` takes the device
scores, targets and lengths of validation batches, launches ``mts_threshold_sweep`` once per batch -- the six integers
``{pk_err, wd_err, windows, tp, fp, fn}`` of every document x threshold, no copy and no synchronise -- and finishes on the host in
float64 with the expressions and the summation order of ``metrics.py`` and ``TextSegmenter.test_step``: the table row of a threshold
EQUALS what ``test_step`` reports at that threshold over the same documents.

Deviations from upstream's dead code, all on purpose: the probability is the decode rule's (upstream compares the raw ``tag[:, 1]``
with the threshold, which is wrong for 1-wide heads); F1 sees the operands as ``test_step`` leaves them (target's last sentence 0).
Not covered: metrics 'b' / 'scaiano' (B-measure, WinPR), the CRF tagger (Viterbi decode has no threshold), and merging the sweeps of
several ranks.

segeval: ``metrics.py`` hands Pk / WindowDiff to the third-party package segeval when it is importable.  Its conventions are not
pinned here, so in that case ``add`` does not use the count kernel: it decodes the tags on the device per threshold
(``ops.greedy_decode``) and runs the host metrics over them, so that sweep and ``test_step`` keep ONE convention.  That path costs
T copies per batch and could not be exercised where this was written (segeval is not installed there).
"""
import numpy as np
import torch

from . import metrics, ops

DEFAULT_THRESHOLDS = np.arange(0.05, 1, 0.05)           # lightning_model.py:440 -- 19 float64 values

PK_ERR, WD_ERR, WINDOWS, TP, FP, FN = range(6)
FALLBACK_THRESHOLD = 0.4                                 # lightning_model.py:547-551


class ThresholdSweep:
    """Accumulates the sweep of a validation epoch.

    thresholds: the grid (float64 as given; the device compares with their fp32 casts, the cast ``greedy_decode``'s
    ``float(threshold)`` -> ``c_float`` makes).  end_boundary: ``TextSegmenter(end_boundary=...)``, the hypothesis' last sentence is 0
    for F1.  invert: SheikhBiLSTM's rule ``1 - prob < th``, i.e. the device thresholds are ``float32(1.0 - th)`` as that tagger's
    forward passes ``1.0 - threshold`` to the decode kernel.
    """

    def __init__(self, thresholds=None, end_boundary=False, invert=False):
        self.thresholds = np.array(DEFAULT_THRESHOLDS if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
        if not 1 <= len(self.thresholds) <= 64:
            raise ValueError(f'ThresholdSweep: {len(self.thresholds)} thresholds, 1..64 are covered')
        self.end_boundary, self.invert = bool(end_boundary), bool(invert)
        dev = [1.0 - float(t) for t in self.thresholds] if self.invert else [float(t) for t in self.thresholds]
        self._device_values = np.array(dev, dtype=np.float32)
        self._th_cache = {}
        self.reset()

    def reset(self):
        self._chunks, self._host_rows = [], []

    def _device_thresholds(self, device):
        key = str(device)
        if key not in self._th_cache:
            self._th_cache[key] = torch.from_numpy(self._device_values).to(device)
        return self._th_cache[key]

    def add(self, scores, targets, lengths):
        """scores [B, L, n_out], targets [B, Lt >= L] on the device; lengths [B] (any device) or None.  One launch; the counts stay on the device."""
        dev = scores.device
        scores = scores.detach().to(torch.float32).contiguous()
        targets = targets.detach().to(device=dev, dtype=torch.float32).contiguous()
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
        if metrics._segeval is not None:  # pragma: no cover - segeval is not installed where this was written
            return self._add_on_host(scores, targets, lengths)
        counts = torch.empty(scores.shape[0], len(self.thresholds), 6, dtype=torch.int32, device=dev)
        ops.threshold_sweep(scores, targets, lengths, self._device_thresholds(dev), counts, self.end_boundary)
        self._chunks.append(counts)

    def add_counts(self, counts):
        """Counts computed elsewhere ([docs, T, 6] integers, numpy or tensor): the seam the selection rules are tested through."""
        if not isinstance(counts, torch.Tensor):
            counts = np.asarray(counts)
        assert tuple(counts.shape[1:]) == (len(self.thresholds), 6), tuple(counts.shape)
        self._chunks.append(counts)

    def _add_on_host(self, scores, targets, lengths):  # pragma: no cover
        B, Lq, _ = scores.shape
        lens = [Lq] * B if lengths is None else [min(max(int(v), 0), Lq) for v in lengths.tolist()]
        tgt = targets.cpu().numpy()
        tags = torch.empty(B, Lq, dtype=torch.uint8, device=scores.device)
        rows = np.zeros((B, len(self.thresholds), 3))
        for j, th in enumerate(self._device_values):
            ops.greedy_decode(scores, lengths, float(th), tags)
            tags_h = tags.cpu().numpy()
            for b, n in enumerate(lens):
                if n:
                    rows[b, j] = host_metrics(tags_h[b, :n], tgt[b, :n], self.end_boundary)
        self._host_rows.append(rows)

    def counts(self):
        """int64 numpy [docs, T, 6] in the order added: one concatenation, one copy."""
        if self._host_rows:  # pragma: no cover
            raise NotImplementedError('ThresholdSweep.counts: with segeval importable the sweep keeps host metrics, not counts')
        if not self._chunks:
            return np.zeros((0, len(self.thresholds), 6), dtype=np.int64)
        if all(isinstance(c, torch.Tensor) for c in self._chunks):
            return torch.cat(self._chunks, dim=0).cpu().numpy().astype(np.int64)
        return np.concatenate([(c.cpu().numpy() if isinstance(c, torch.Tensor) else c).astype(np.int64) for c in self._chunks], axis=0)

    def _per_document(self):
        """float64 [docs, T, 3] = Pk, WD, F1 of every document x threshold, by the expressions of metrics.pk / window_diff / f1_boundary."""
        if self._host_rows:  # pragma: no cover
            return np.concatenate(self._host_rows, axis=0)
        c = self.counts()
        w = c[..., WINDOWS]
        has = w > 0
        safe = np.where(has, w, 1)
        pk = np.where(has, c[..., PK_ERR] / safe.astype(np.float64), 0.0)
        wd = np.where(has, c[..., WD_ERR] / safe.astype(np.float64), 0.0)
        tp, fp, fn = (c[..., i].astype(np.float64) for i in (TP, FP, FN))
        den = 2 * tp + fp + fn
        f1 = np.where(tp == 0, 0.0, 2 * tp / np.where(den == 0, 1.0, den))
        return np.stack([pk, wd, f1], axis=-1)

    def table(self):
        """{'thresholds', 'Pk_loss', 'WD_loss', 'F1_loss'}: arrays of length T, the mean over the documents added, summed in that order."""
        per = self._per_document()
        docs = per.shape[0]
        if docs == 0:
            raise ValueError('ThresholdSweep.table: no documents were added')
        acc = np.zeros(per.shape[1:])
        for d in range(docs):                            # one document after the other, as test_step's `+=` (np.sum adds pairwise)
            acc = acc + per[d]
        acc = acc / docs
        return {'thresholds': self.thresholds.copy(), 'Pk_loss': acc[:, 0], 'WD_loss': acc[:, 1], 'F1_loss': acc[:, 2]}

    def best(self, metric='Pk'):
        """The reference's result dict (lightning_model.py:510-553): 'F1' maximises from -1 with >, 'WD' minimises from 1 with <, anything else
        is Pk and minimises from 1; the first best threshold wins; no threshold beating the start value gives the first row with threshold 0.4."""
        tab = self.table()
        key = {'F1': 'F1_loss', 'WD': 'WD_loss'}.get(metric, 'Pk_loss')
        maximise = key == 'F1_loss'
        best, best_idx, best_th = (-1, 0, None) if maximise else (1, 0, None)
        for idx, th in enumerate(self.thresholds):
            v = tab[key][idx]
            if (v > best) if maximise else (v < best):
                best, best_idx, best_th = v, idx, th
        out = {k: float(tab[k][best_idx]) for k in ('Pk_loss', 'F1_loss', 'WD_loss')}
        out['valid_loss'] = out.pop(key)
        out['threshold'] = float(best_th) if best_th is not None else FALLBACK_THRESHOLD
        return out


def host_metrics(tags, target, end_boundary=False):
    """(Pk, WD, F1) of one document by metrics.py in test_step's order (lightning_model.py:558-676), on copies."""
    tag = np.array(tags).astype(int)
    tgt = np.array(target).astype(np.float32)
    if end_boundary:
        tag[-1] = 0
        tgt[-1] = 0
    pk = float(metrics.compute_Pk(np.array(tag), tgt))
    f1 = metrics.f1_boundary(tgt.astype(int), np.array(tag).astype(int))
    try:
        wd = float(metrics.compute_window_diff(np.array(tag), tgt))
    except AssertionError:
        wd = float(metrics.compute_Pk(np.array(tag), tgt))
    return pk, wd, f1
