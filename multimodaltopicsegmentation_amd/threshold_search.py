"""Decision-threshold search on the device (reference: models/lightning_model.py:435-553, the validation-epoch sweep that upstream
disabled by renaming the hook).

Every tagger that decodes by a threshold uses ``prob > th`` (SheikhBiLSTM: ``1 - prob < th``).  ``ThresholdSweep`` takes the device
scores, targets and lengths of validation batches, launches ``mts_threshold_sweep`` once per batch -- the six integers
``{pk_err, wd_err, windows, tp, fp, fn}`` of every document x threshold, no copy and no synchronise -- and finishes on the host in
float64 with the expressions and the summation order of ``metrics.py`` and ``TextSegmenter.test_step``: the table row of a threshold
EQUALS what ``test_step`` reports at that threshold over the same documents.

Deviations from upstream's dead code, all on purpose: the probability is the decode rule's (upstream compares the raw ``tag[:, 1]``
with the threshold, which is wrong for 1-wide heads); F1 sees the operands as ``test_step`` leaves them (target's last sentence 0).
Not covered: metric 'b' (B-measure: boundary edit distance lives in segeval), the CRF tagger in its default Viterbi decode (a best path
has no threshold).  Covered since the posterior-marginal decode: ``BiRnnCrf(decode='marginal')`` / ``TextSegmenter(crf_decode='marginal')``
scores every sentence with the logit of P(y_t = 1 | x) (mts_crf_marginals), a 1-wide head like any other to this sweep.

WinPR (``metric='scaiano'``): ``add`` launches ``mts_winpr_sweep`` instead, three integers ``{TP, FP, FN}`` per document x threshold of
upstream's call ``WinPR(reference=tags, hypothesis=target)`` (lightning_model.py:622) on the operands the scaiano branch of ``test_step``
leaves (nothing cleared but, under ``end_boundary``, both last sentences), and the floats follow on the host from the integers with
``metrics.WinPR``'s expressions.  One more deviation, on purpose: ``TP + FN == 0`` or ``TP == 0`` gives (0, 0, 0) here, where upstream and
``metrics.WinPR`` raise ZeroDivisionError (``TP + FP == 0`` is (0, 0, 0) upstream too) -- a sweep reaches an empty hypothesis at its
high thresholds by design.  WinPR needs no segeval, so this sweep always takes the count kernel.

Several ranks: validation under data parallelism shards the documents, so ``gather()`` merges the ranks' integer counts before any rank
chooses a threshold.  With a key per document (``add(..., keys=)``, e.g. the corpus index) the merged sweep is in ascending key order and
its ``table()`` has the bytes of a single-process sweep fed the same documents in that order: the integers are exact and the float64 sum
runs over the same documents in the same order.

segeval: ``metrics.py`` hands Pk / WindowDiff to the third-party package segeval when it is importable.  Its conventions are not
pinned here, so in that case ``add`` does not use the count kernel: it decodes the tags on the device per threshold
(``ops.greedy_decode``) and runs the host metrics over them, so that sweep and ``test_step`` keep ONE convention.  That path costs
T copies per batch and could not be exercised where this was written (segeval is not installed there).
"""
import numpy as np
import torch
import torch.distributed as dist

from . import metrics, ops

DEFAULT_THRESHOLDS = np.arange(0.05, 1, 0.05)           # lightning_model.py:440 -- 19 float64 values

PK_ERR, WD_ERR, WINDOWS, TP, FP, FN = range(6)
W_TP, W_FP, W_FN = range(3)                              # the WinPR sweep's integers
FALLBACK_THRESHOLD = 0.4                                 # lightning_model.py:547-551


class ThresholdSweep:
    """Accumulates the sweep of a validation epoch.

    thresholds: the grid (float64 as given; the device compares with their fp32 casts, the cast ``greedy_decode``'s
    ``float(threshold)`` -> ``c_float`` makes).  end_boundary: ``TextSegmenter(end_boundary=...)``, the hypothesis' last sentence is 0
    for F1.  invert: SheikhBiLSTM's rule ``1 - prob < th``, i.e. the device thresholds are ``float32(1.0 - th)`` as that tagger's
    forward passes ``1.0 - threshold`` to the decode kernel.  metric: None / 'Pk' / 'WD' / 'F1' -> the six-integer sweep; 'scaiano' (any
    case) -> the WinPR sweep with window ``winpr_k`` (1..64; upstream's default 10): ``counts()`` is [docs, T, 3], ``table()`` has
    'b_precision' / 'b_recall' / 'b_f1', ``best()`` maximises b_f1; 'b' raises NotImplementedError.
    """

    def __init__(self, thresholds=None, end_boundary=False, invert=False, metric=None, winpr_k=10):
        name = None if metric is None else str(metric).lower()
        if name == 'b':
            raise NotImplementedError("ThresholdSweep: metric 'b' (B-measure) needs the third-party package segeval (boundary edit "
                                      'distance); there is no kernel for it')
        self.metric = metric
        self.winpr = name == 'scaiano'
        self.winpr_k = int(winpr_k)
        if self.winpr and not 1 <= self.winpr_k <= 64:
            raise ValueError(f'ThresholdSweep: winpr_k={self.winpr_k}, windows of 1..64 sentences are covered')
        self.width = 3 if self.winpr else 6
        self.thresholds = np.array(DEFAULT_THRESHOLDS if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
        if not 1 <= len(self.thresholds) <= 64:
            raise ValueError(f'ThresholdSweep: {len(self.thresholds)} thresholds, 1..64 are covered')
        self.end_boundary, self.invert = bool(end_boundary), bool(invert)
        dev = [1.0 - float(t) for t in self.thresholds] if self.invert else [float(t) for t in self.thresholds]
        self._device_values = np.array(dev, dtype=np.float32)
        self._th_cache = {}
        self.reset()

    def reset(self):
        self._chunks, self._keys, self._host_rows = [], [], []

    def _device_thresholds(self, device):
        key = str(device)
        if key not in self._th_cache:
            self._th_cache[key] = torch.from_numpy(self._device_values).to(device)
        return self._th_cache[key]

    @staticmethod
    def _as_keys(keys, docs):
        if keys is None:
            return None
        k = (keys.detach().cpu().numpy() if isinstance(keys, torch.Tensor) else np.asarray(keys)).astype(np.int64).reshape(-1)
        if k.size != docs:
            raise ValueError(f'ThresholdSweep: {k.size} keys for {docs} documents')
        return k

    def add(self, scores, targets, lengths, keys=None):
        """scores [B, L, n_out], targets [B, Lt >= L] on the device; lengths [B] (any device) or None; keys: one int64 per document (host
        data, e.g. the corpus indices) or None.  One launch; the counts stay on the device."""
        dev = scores.device
        keys = self._as_keys(keys, scores.shape[0])
        scores = scores.detach().to(torch.float32).contiguous()
        targets = targets.detach().to(device=dev, dtype=torch.float32).contiguous()
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
        if self.winpr:
            counts = torch.empty(scores.shape[0], len(self.thresholds), 3, dtype=torch.int32, device=dev)
            ops.winpr_sweep(scores, targets, lengths, self._device_thresholds(dev), counts, self.end_boundary, self.winpr_k)
            self._chunks.append(counts)
            self._keys.append(keys)
            return None
        if metrics._segeval is not None:  # pragma: no cover - segeval is not installed where this was written
            return self._add_on_host(scores, targets, lengths)
        counts = torch.empty(scores.shape[0], len(self.thresholds), 6, dtype=torch.int32, device=dev)
        ops.threshold_sweep(scores, targets, lengths, self._device_thresholds(dev), counts, self.end_boundary)
        self._chunks.append(counts)
        self._keys.append(keys)

    def add_counts(self, counts, keys=None):
        """Counts computed elsewhere ([docs, T, 6] integers, [docs, T, 3] for the WinPR sweep; numpy or tensor): the seam the selection
        rules and the rank merge are tested through."""
        if not isinstance(counts, torch.Tensor):
            counts = np.asarray(counts)
        assert tuple(counts.shape[1:]) == (len(self.thresholds), self.width), tuple(counts.shape)
        self._chunks.append(counts)
        self._keys.append(self._as_keys(keys, counts.shape[0]))

    def gather(self, group=None):
        """Merge the sweeps of every rank of ``group``: afterwards each rank's sweep holds all ranks' documents.  EVERY rank calls it, a rank
        without documents too.  Order: ascending key when every chunk of every rank carried keys (a key held twice raises ValueError, on
        every rank, after the collectives), rank-major otherwise.  No initialised process group, or a group of one: nothing happens.
        The ranks' document counts are all-gathered, then the int32 counts (and the int64 keys) padded to the largest rank: over RCCL on
        the device (a rank whose counts are on the host, or that has none, uses the current device), over any other backend on the host."""
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        if self._host_rows:  # pragma: no cover
            raise NotImplementedError('ThresholdSweep.gather: with segeval importable the sweep keeps host metrics, not counts')
        world, T = dist.get_world_size(group), len(self.thresholds)
        if dist.get_backend(group) == 'nccl':
            on = [c.device for c in self._chunks if isinstance(c, torch.Tensor) and c.device.type == 'cuda']
            dev = on[0] if on else torch.device('cuda', torch.cuda.current_device())
        else:
            dev = torch.device('cpu')
        parts = [(c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c))).to(device=dev, dtype=torch.int32) for c in self._chunks]
        mine = torch.cat(parts, dim=0) if parts else torch.zeros(0, T, self.width, dtype=torch.int32, device=dev)
        keyed = all(k is not None for k in self._keys)
        head = torch.tensor([mine.shape[0], int(keyed)], dtype=torch.int64, device=dev)
        heads = [torch.empty_like(head) for _ in range(world)]
        dist.all_gather(heads, head, group=group)
        heads = torch.stack(heads).cpu().numpy()
        docs, keyed = heads[:, 0].tolist(), bool(heads[:, 1].min())
        most = max(docs)
        if most == 0:
            return self
        padded = torch.zeros(most, T, self.width, dtype=torch.int32, device=dev)
        padded[:mine.shape[0]] = mine
        every = [torch.empty_like(padded) for _ in range(world)]
        dist.all_gather(every, padded, group=group)
        counts = torch.cat([c[:n] for c, n in zip(every, docs)], dim=0).cpu().numpy()              # rank-major
        keys = None
        if keyed:
            kp = torch.zeros(most, dtype=torch.int64, device=dev)
            if mine.shape[0]:
                kp[:mine.shape[0]] = torch.from_numpy(np.concatenate(self._keys)).to(dev)
            kevery = [torch.empty_like(kp) for _ in range(world)]
            dist.all_gather(kevery, kp, group=group)
            keys = torch.cat([k[:n] for k, n in zip(kevery, docs)]).cpu().numpy()
            order = np.argsort(keys, kind='stable')
            keys, counts = keys[order], counts[order]
            if (np.diff(keys) == 0).any():
                raise ValueError(f'ThresholdSweep.gather: document key {int(keys[1:][np.diff(keys) == 0][0])} is held more than once')
        self._chunks, self._keys = [counts], [keys]
        return self

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
        """int64 numpy [docs, T, 6] ([docs, T, 3] for the WinPR sweep) in the order added: one concatenation, one copy."""
        if self._host_rows:  # pragma: no cover
            raise NotImplementedError('ThresholdSweep.counts: with segeval importable the sweep keeps host metrics, not counts')
        if not self._chunks:
            return np.zeros((0, len(self.thresholds), self.width), dtype=np.int64)
        if all(isinstance(c, torch.Tensor) for c in self._chunks):
            return torch.cat(self._chunks, dim=0).cpu().numpy().astype(np.int64)
        return np.concatenate([(c.cpu().numpy() if isinstance(c, torch.Tensor) else c).astype(np.int64) for c in self._chunks], axis=0)

    def _per_document(self):
        """float64 [docs, T, 3] = Pk, WD, F1 of every document x threshold, by the expressions of metrics.pk / window_diff / f1_boundary."""
        if self._host_rows:  # pragma: no cover
            return np.concatenate(self._host_rows, axis=0)
        c = self.counts()
        if self.winpr:
            return winpr_floats(c)
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
        """{'thresholds', 'Pk_loss', 'WD_loss', 'F1_loss'} ({'thresholds', 'b_precision', 'b_recall', 'b_f1'} for the WinPR sweep): arrays of
        length T, the mean over the documents added, summed in that order."""
        per = self._per_document()
        docs = per.shape[0]
        if docs == 0:
            raise ValueError('ThresholdSweep.table: no documents were added')
        acc = np.zeros(per.shape[1:])
        for d in range(docs):                            # one document after the other, as test_step's `+=` (np.sum adds pairwise)
            acc = acc + per[d]
        acc = acc / docs
        if self.winpr:
            return {'thresholds': self.thresholds.copy(), 'b_precision': acc[:, 0], 'b_recall': acc[:, 1], 'b_f1': acc[:, 2]}
        return {'thresholds': self.thresholds.copy(), 'Pk_loss': acc[:, 0], 'WD_loss': acc[:, 1], 'F1_loss': acc[:, 2]}

    def best(self, metric='Pk'):
        """The reference's result dict (lightning_model.py:510-553): 'F1' maximises from -1 with >, 'WD' minimises from 1 with <, anything else
        is Pk and minimises from 1; the first best threshold wins; no threshold beating the start value gives the first row with threshold 0.4.
        The WinPR sweep has one rule whatever ``metric`` says (lightning_model.py:493-508): b_f1 maximised from -1 with >, returned as
        'valid_loss' next to 'b_precision', 'b_recall' and 'threshold'."""
        tab = self.table()
        if self.winpr:
            best, best_idx, best_th = -1, 0, None
            for idx, th in enumerate(self.thresholds):
                if tab['b_f1'][idx] > best:
                    best, best_idx, best_th = tab['b_f1'][idx], idx, th
            return {'b_precision': float(tab['b_precision'][best_idx]), 'b_recall': float(tab['b_recall'][best_idx]),
                    'valid_loss': float(tab['b_f1'][best_idx]), 'threshold': float(best_th) if best_th is not None else FALLBACK_THRESHOLD}
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


def winpr_floats(counts):
    """float64 [..., 3] = (precision, recall, f1) from the integers [..., 3] = {TP, FP, FN} by the expressions of metrics.WinPR, in its
    order; (0, 0, 0) where TP + FP == 0 (upstream) and where TP + FN == 0 or TP == 0 (the module docstring's deviation)."""
    c = np.asarray(counts).astype(np.int64)
    tp, fp, fn = c[..., W_TP], c[..., W_FP], c[..., W_FN]
    ok = (tp + fp != 0) & (tp + fn != 0) & (tp != 0)
    p = tp / np.where(ok, tp + fp, 1)                    # int64 / int64 -> float64, correctly rounded as python's int / int
    r = tp / np.where(ok, tp + fn, 1)
    f = 2 * (p * r / np.where(ok, p + r, 1.0))
    return np.stack([np.where(ok, p, 0.0), np.where(ok, r, 0.0), np.where(ok, f, 0.0)], axis=-1)


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
