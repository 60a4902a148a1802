"""The test pass on the device and the reporting behind it (reference: what follows ``trainer.fit`` in train_fit.py -- ``trainer.test``
over the test split with per-document results, :414-427, the fold means, :497-520, and the 10 000-sample bootstrap that turns them into
"mean +- 95 % half-width", :540-562 and compute_accuracy_metrics_sentence.py:63-260).

    evaluate(trainer_or_model, corpus, batch_size=8, threshold=None, min_segment=None) -> per-document Pk / WD / F1 / WinPR, their means, the integers
    bootstrap_ci(values, samples=10000, seed=0)                           -> mean, 2.5 / 97.5 percentiles of the resample means, half width
    paired_bootstrap(a, b, samples=10000, seed=0)                         -> the same for a - b, and the share of resamples on either side of 0
    cross_validate(make_trainer, folds, **fit_keywords)                   -> fit + evaluate per fold, fold means, report, pooled report

``evaluate`` is ``fit``'s validation pass turned into a test pass: eval mode, documents ``rank::world`` of the corpus in index order in
batches of ``batch_size``, no document dropped, a rank without documents skips the forward and still joins the collectives.  The scores of
every batch go to TWO ``ThresholdSweep`` objects with the one-value grid ``[threshold]``, keyed by corpus index: the six-integer sweep
(Pk, WindowDiff, F1) and the WinPR sweep; ``gather()`` merges the ranks, the floats follow from the integers by the sweeps' own
expressions and the means by ``table()``'s sequential float64 sum -- so ``mean`` EQUALS what ``TextSegmenter.test_step`` reports for the
same model over a batch of all the documents, for metric 'Pk' / 'WD' / 'F1' and for metric 'scaiano' (up to the WinPR sweep's stated
zero convention where ``metrics.WinPR`` divides by zero).  Nothing is decoded to python lists for the metrics and no host loop runs per
document.  Metric 'b' is not offered: it needs segeval, as everywhere else in this package.

The threshold is the argument, else ``model.th`` when that is set, else 0.4; a falsy one becomes 0.5 (test_step's rule,
lightning_model.py:583-587).  Two hypotheses have no threshold: the Viterbi path of ``BiRnnCrf(decode='viterbi')`` and the all-zero
baseline (``zero_baseline=True``, lightning_model.py:572-581).  Either reaches the same two kernels as saturated logits, +30 where the tag
is 1 and -30 elsewhere, swept at 0.5; the reported ``threshold`` is 0.5 for the Viterbi path and 0.4 for the baseline.

The bootstrap is one launch of ``mts_bootstrap_sums`` (csrc/bootstrap.hip): resample s draws its n documents by a counter hash of
(seed, s * n + j) and sums every metric row over them sequentially in float64, so the resample means are the same bits on every rank and
machine, and a host loop with the same hash reproduces them (the tests hold such a loop against the kernel).  The division by n and the percentiles are
numpy's, on the host.  ``paired_bootstrap`` stands where the reference's post-hoc script runs t-tests between two systems
(compute_accuracy_metrics_sentence.py:280-321); it is an extension, not a port of them.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .fit import _forward, fit
from .rnn_taggers import SheikhBiLSTM
from .taggers import decodes_by_viterbi
from .threshold_search import FALLBACK_THRESHOLD, ThresholdSweep

SIX_KEYS = ('Pk', 'WD', 'F1')
WINPR_KEYS = ('b_precision', 'b_recall', 'b_f1')
METRIC_KEYS = SIX_KEYS + WINPR_KEYS
SATURATED = 30.0                                         # sigmoid(+-30) is 1 - 9e-14 / 9e-14: on either side of 0.5 whatever the format


def _unwrap(trainer_or_model):
    """-> (tagger, rank, world, process group, merge the ranks?)"""
    from .trainer import NativeTrainer
    if isinstance(trainer_or_model, NativeTrainer):
        t = trainer_or_model
        return t.model, (dist.get_rank(t.pg) if t.world > 1 else 0), t.world, t.pg, True
    model = trainer_or_model.model if hasattr(trainer_or_model, 'training_step') else trainer_or_model
    return model, 0, 1, None, False


def _saturated(tags, L, device):
    """tag lists (one per document) -> fp32 [B, L, 1] logits: +30 where the tag is 1, -30 elsewhere"""
    h = np.full((len(tags), L, 1), -SATURATED, dtype=np.float32)
    for b, t in enumerate(tags):
        t = np.asarray(t).reshape(-1)[:L]
        h[b, :t.size, 0] = np.where(t == 1, SATURATED, -SATURATED)
    return torch.from_numpy(h).to(device)


def _constrained_logits(scores, lengths, threshold, min_segment):
    """scores [B, L, n_out] -> the saturated fp32 [B, L, 1] logits of the constrained decode's tags, built on the device"""
    scores = scores.detach().to(torch.float32).contiguous()
    B, Lq = int(scores.shape[0]), int(scores.shape[1])
    dev = scores.device
    li = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
    tags = torch.empty((B, Lq), dtype=torch.uint8, device=dev)
    ops.segment_decode(scores, li, threshold, torch.empty((B, 1), dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                       min_segment=min_segment, close_last=False, tags=tags)
    return (tags.to(torch.float32) * (2 * SATURATED) - SATURATED).unsqueeze(-1)


def evaluate(trainer_or_model, corpus, *, batch_size=8, threshold=None, end_boundary=False, winpr_k=10, zero_baseline=False,
             return_scores=False, min_segment=None):
    """-> {'threshold', 'documents': int64 corpus indices ascending, 'per_document': {'Pk', 'WD', 'F1', 'b_precision', 'b_recall', 'b_f1'}
    float64 [n] each, 'mean': the same six keys -> float, 'counts': {'sweep': int64 [n, 6] = {pk_err, wd_err, windows, tp, fp, fn}, 'winpr':
    int64 [n, 3] = {TP, FP, FN}}}; the same values on every rank.  ``trainer_or_model``: a ``NativeTrainer`` (rank, world and process group
    are its) or a bare tagger / ``TextSegmenter`` (a single process).  ``return_scores=True`` adds 'scores': one fp32 array [length, n_out]
    per document THIS rank scored (``documents[rank::world]``), trimmed to the document's length -- the saturated logits for the Viterbi
    path and the baseline.  With segeval importable the six-integer sweep keeps host metrics (ThresholdSweep's rule): 'counts'['sweep'] is
    None then.  ``min_segment=m >= 2``: the hypothesis is the constrained decode of ``predict`` (``ops.segment_decode`` at the threshold,
    segments of at least m sentences; an extension without an upstream counterpart): its tags become saturated logits on the device and
    both sweeps run at 0.5; 'threshold' is the one the decode used, 'scores' the saturated logits.  None or 1 leaves the pass as it is."""
    model, rank, world, pg, merge = _unwrap(trainer_or_model)
    n_docs = len(corpus)
    if n_docs == 0:
        raise ValueError('evaluate: the corpus has no documents')
    if not getattr(corpus, 'labelled', True):
        raise ValueError('evaluate: the corpus is unlabelled (ResidentCorpus.from_documents); predict is the pass that needs no labels')
    viterbi = decodes_by_viterbi(model)                # BiRnnCrf / TransformerCRF in their default decode
    m = 1 if min_segment is None else int(min_segment)
    if m < 1:
        raise ValueError(f'evaluate: min_segment={min_segment}; a segment holds at least one sentence')
    if m > 1 and viterbi:
        raise ValueError("evaluate: min_segment > 1 needs probabilities; BiRnnCrf(decode='viterbi') has a path, not scores "
                         "(decode='marginal' gives them)")
    constrained = m > 1 and not zero_baseline
    if zero_baseline:
        reported, at = FALLBACK_THRESHOLD, 0.5
    elif viterbi:
        reported, at = 0.5, 0.5
    else:
        th = threshold if threshold is not None else getattr(model, 'th', None)
        if th is None:
            th = FALLBACK_THRESHOLD
        if not th:
            th = 0.5
        reported = at = float(th)
    invert = isinstance(model, SheikhBiLSTM) and not zero_baseline
    if constrained:                                    # the decode takes the threshold (and SheikhBiLSTM's inversion); the sweeps see decisions
        decode_at, at, invert = (1.0 - at if invert else at), 0.5, False
    six = ThresholdSweep(thresholds=[at], end_boundary=end_boundary, invert=invert, metric=None)
    win = ThresholdSweep(thresholds=[at], end_boundary=end_boundary, invert=invert, metric='scaiano', winpr_k=winpr_k)
    docs = list(range(rank, n_docs, world))
    dev = model.flat.device
    kept = []
    was_training = model.training
    model.eval()
    try:
        if not hasattr(model, 'th'):
            model.th = None                            # SheikhBiLSTM's forward reads it (upstream never sets it before test_step does)
        with torch.cuda.device(dev):
            for s in range(0, len(docs), batch_size):
                idx = docs[s:s + batch_size]
                batch = corpus.batch(idx)
                if zero_baseline:
                    scores = torch.full((len(idx), batch['tgt_tokens'].shape[1], 1), -SATURATED, dtype=torch.float32, device=dev)
                elif viterbi:
                    scores = _saturated(model(batch['src_tokens'], batch['src_lengths'])[1], batch['tgt_tokens'].shape[1], dev)
                else:
                    scores = _forward(model, batch)
                if constrained:
                    scores = _constrained_logits(scores, batch['src_lengths'], decode_at, m)
                six.add(scores, batch['tgt_tokens'], batch['src_lengths'], keys=idx)
                win.add(scores, batch['tgt_tokens'], batch['src_lengths'], keys=idx)
                if return_scores:
                    host = scores.detach().to(torch.float32).cpu().numpy()
                    kept += [host[b, :min(int(n), host.shape[1])].copy() for b, n in enumerate(batch['src_lengths'].tolist())]
    finally:
        model.train(was_training)
    if merge:
        six.gather(pg)
        win.gather(pg)
    documents = np.concatenate([np.asarray(k, dtype=np.int64) for k in win._keys])
    if documents.size != n_docs or (np.diff(documents) <= 0).any():
        raise RuntimeError(f'evaluate: the merged sweep holds {documents.size} documents out of order or incomplete ({n_docs} expected)')
    per6, perw = six._per_document()[:, 0, :], win._per_document()[:, 0, :]
    tab6, tabw = six.table(), win.table()
    out = {'threshold': reported, 'documents': documents,
           'per_document': {**{k: per6[:, i].copy() for i, k in enumerate(SIX_KEYS)}, **{k: perw[:, i].copy() for i, k in enumerate(WINPR_KEYS)}},
           'mean': {**{k: float(tab6[k + '_loss'][0]) for k in SIX_KEYS}, **{k: float(tabw[k][0]) for k in WINPR_KEYS}},
           'counts': {'sweep': None if six._host_rows else six.counts()[:, 0, :], 'winpr': win.counts()[:, 0, :]}}
    if return_scores:
        out['scores'] = kept
    return out


# ---- the statistics -----------------------------------------------------------------------------------------------------------
def _as_rows(values):
    """-> (float64 [M, n] on the host, the dict's keys or None)"""
    keys = None
    if isinstance(values, dict):
        keys = list(values)
        rows = [_host(values[k]).reshape(-1) for k in keys]
        if len({r.size for r in rows}) > 1:
            raise ValueError(f'bootstrap: the arrays of the dict differ in length ({[r.size for r in rows]})')
        v = np.stack(rows) if rows else np.zeros((0, 0))
    else:
        v = _host(values)
        v = v.reshape(1, -1) if v.ndim <= 1 else v
    if v.ndim != 2 or v.shape[0] == 0 or v.shape[1] == 0:
        raise ValueError(f'bootstrap: values of shape {tuple(v.shape)}; [n] or [M, n] with M, n >= 1 are covered')
    return np.ascontiguousarray(v, dtype=np.float64), keys


def _host(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


def resample_means(values, samples=10000, seed=0, device=None, *, sums=None):
    """float64 [M, samples]: the mean of every row of ``values`` ([M, n] on the host) over each resample.  One launch of
    ``ops.bootstrap_sums`` on ``device`` (default: the current GPU), then ``sums / n`` in float64.  ``sums``: resample sums computed
    elsewhere ([M, samples]) in place of the launch -- the seam the statistics are tested through without a GPU."""
    M, n = values.shape
    if sums is None:
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        with torch.cuda.device(dev):
            sums = ops.bootstrap_sums(torch.from_numpy(values).to(dev), samples, seed).cpu().numpy()
    sums = np.asarray(sums, dtype=np.float64).reshape(M, -1)
    if sums.shape[1] != int(samples):
        raise ValueError(f'bootstrap: sums of {sums.shape[1]} resamples for samples={int(samples)}')
    return sums / n


def _keyed(arr, keys):
    return arr if keys is None else {k: float(arr[i]) for i, k in enumerate(keys)}


def bootstrap_ci(values, samples=10000, seed=0, device=None, *, sums=None):
    """Percentile bootstrap of the mean (train_fit.py:540-562): -> {'mean': the plain mean of ``values``, 'lo' / 'hi': the 2.5 / 97.5
    percentiles (np.percentile) of the ``samples`` resample means, 'half_width': (hi - lo) / 2, the reference's expression :550}.
    ``values``: float64 [n] or [M, n] (M <= 16 rows resampled TOGETHER: row m of every resample covers the same documents) -> arrays of
    length M; or a dict of equal-length arrays -> dicts of floats under the same keys.  ``sums``: see ``resample_means``."""
    v, keys = _as_rows(values)
    means = resample_means(v, samples, seed, device, sums=sums)
    lo, hi = np.percentile(means, 2.5, axis=1), np.percentile(means, 97.5, axis=1)
    return {'mean': _keyed(v.mean(axis=1), keys), 'lo': _keyed(lo, keys), 'hi': _keyed(hi, keys), 'half_width': _keyed((hi - lo) / 2, keys)}


def paired_bootstrap(a, b, samples=10000, seed=0, device=None, *, sums=None):
    """Two systems' per-document values over the SAME documents (e.g. text-only against text + audio): bootstraps d = a - b with the same
    kernel -> {'mean_diff', 'lo', 'hi' (2.5 / 97.5 percentiles of the resample means of d), 'p_le_0': the share of resample means <= 0,
    'p_ge_0': the share >= 0}, arrays of length M (1 for [n] inputs) or dicts for dict inputs.  ValueError when the lengths differ.

    An extension: the reference's post-hoc script compares two systems with t-tests (compute_accuracy_metrics_sentence.py:280-321); this
    takes their role with the resampling the intervals already use, and is not a port of them."""
    va, ka = _as_rows(a)
    vb, kb = _as_rows(b)
    if va.shape != vb.shape or ka != kb:
        raise ValueError(f'paired_bootstrap: the two systems differ in shape or keys ({tuple(va.shape)} against {tuple(vb.shape)})')
    d = np.ascontiguousarray(va - vb)
    means = resample_means(d, samples, seed, device, sums=sums)
    return {'mean_diff': _keyed(d.mean(axis=1), ka), 'lo': _keyed(np.percentile(means, 2.5, axis=1), ka),
            'hi': _keyed(np.percentile(means, 97.5, axis=1), ka), 'p_le_0': _keyed((means <= 0).mean(axis=1), ka),
            'p_ge_0': _keyed((means >= 0).mean(axis=1), ka)}


def _by_metric(ci):
    """bootstrap_ci's dict of dicts, turned round: {metric: {'mean', 'lo', 'hi', 'half_width'}}"""
    return {k: {stat: ci[stat][k] for stat in ('mean', 'lo', 'hi', 'half_width')} for k in ci['mean']}


def cross_validate(make_trainer, folds, *, samples=10000, bootstrap_seed=0, winpr_k=10, **fit_kw):
    """The driver over folds (train_fit.py:497-562).  ``folds``: a list of (train, val, test) ``ResidentCorpus`` triples, ``val`` may be
    None; ``make_trainer()`` gives a fresh ``NativeTrainer`` per fold; ``fit_kw`` goes to ``fit`` (``batch_size`` and ``end_boundary`` to
    the test pass too).  Per fold: ``fit``, then ``evaluate(trainer, test, threshold=None)`` -- the fit's threshold is on ``model.th``.
    -> {'folds': [{'fit', 'test'}], 'fold_means': {metric: float64 [k]}, 'report': {metric: bootstrap_ci over the k fold means}, the
    reference's rule, 'pooled': {metric: bootstrap_ci over all folds' per-document values}, the post-hoc script's rule}, each
    {'mean', 'lo', 'hi', 'half_width'} of floats; the six metrics share a resample.  The same on every rank; nothing is written to disk."""
    if not folds:
        raise ValueError('cross_validate: no folds')
    runs = []
    for train, val, test in folds:
        trainer = make_trainer()
        record = fit(trainer, train, val, **fit_kw)
        runs.append({'fit': record, 'test': evaluate(trainer, test, batch_size=fit_kw.get('batch_size', 8), threshold=None,
                                                     end_boundary=fit_kw.get('end_boundary', False), winpr_k=winpr_k)})
        device = trainer.model.flat.device
    fold_means = {k: np.array([r['test']['mean'][k] for r in runs], dtype=np.float64) for k in METRIC_KEYS}
    pooled = {k: np.concatenate([r['test']['per_document'][k] for r in runs]) for k in METRIC_KEYS}
    return {'folds': runs, 'fold_means': fold_means,
            'report': _by_metric(bootstrap_ci(fold_means, samples, bootstrap_seed, device)),
            'pooled': _by_metric(bootstrap_ci(pooled, samples, bootstrap_seed, device))}
