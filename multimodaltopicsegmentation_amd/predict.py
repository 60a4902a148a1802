"""The prediction pass on the device: a folder of unlabelled documents -> segments (reference: predict.py -- ``Predictor.predict`` loads
``load_dataset_for_inference(dir)``, wraps it in ``AudioPortionDatasetInference``, runs ``trainer.predict`` and turns every tag list into
spans with ``segment_audio``, :268-349 and :92-129).

    corpus = ResidentCorpus.from_documents(*load_dataset_for_inference(folder)[:1], device, names=files)
    predict(trainer_or_model, corpus, batch_size=8, threshold=None, min_segment=1, close_last=True)   -> Prediction
    Prediction.spans(times) / .pool(corpus, mode) / .as_saturated(device) / Prediction.merge(parts)
    segment_audio(n_samples, segmentation, sr, interval, adaptive)                                   -> sample spans, upstream's rule

``predict`` is ``evaluate`` without targets: eval mode (restored afterwards), documents ``rank::world`` of the corpus in index order in
batches of ``batch_size``, the same threshold rule (the argument, else ``model.th``, else 0.4; a falsy one becomes 0.5), ``SheikhBiLSTM``
handing ``1 - th`` to the kernel as ``ThresholdSweep(invert=True)`` does.  Per batch there is ONE forward and ONE ``ops.segment_decode``
launch (csrc/segment_decode.hip): tags, probabilities and every document's segment table -- the exclusive ends of its segments -- are made
on the device, and only the table and the counts come back, in one copy per batch with ``Smax`` = the batch's padded length; tags and
probabilities are read back when asked for.  Nothing is decoded to python lists per sentence and no host loop runs over sentences.  The
Viterbi path of ``BiRnnCrf(decode='viterbi')`` reaches the same kernel as saturated logits, as in ``evaluate``; ``decode='marginal'`` is an
ordinary 1-wide head.  The ranks' parts are merged (``Prediction.merge``, keyed by corpus index) so that every rank returns the same object.

``min_segment = m >= 2`` is a decode the per-sentence threshold cannot express: the best boundary set all of whose segments hold at least m
sentences, exact in integers (include/mts.h).  The reference's basic unit for audio is a 1-second chunk, where ``prob > th`` gives one-unit
segments wherever the score flickers, and its only answer is ``add_overlap``.  It is an EXTENSION: upstream has no counterpart to hold it
against, and no claim about Pk is made for it.  It needs probabilities, so it refuses the Viterbi path.

Not here: audio I/O, resampling, writing segment files and the ``Predictor`` class's hyper-parameter-file parsing.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .evaluate import _saturated, _unwrap
from .fit import _forward
from .rnn_taggers import SheikhBiLSTM
from .taggers import decodes_by_viterbi
from .threshold_search import FALLBACK_THRESHOLD

POOL_MODES = ('mean', 'max', 'mean_std', 'max_std')


class Prediction:
    """The segments of a set of documents, on the host.

    ``threshold`` (the one the decode used), ``min_segment``, ``close_last``; ``documents``: int64 corpus indices, ascending; ``names``: the
    file names in that order, or None; ``lengths`` / ``n_segments``: int64 per document; ``segment_ends``: one int64 array per document, the
    exclusive ends of its segments in order (under ``close_last`` the last one is the document's length); ``tags`` (uint8) and
    ``probabilities`` (float32): one array per document trimmed to its length, or None when they were not asked for."""

    def __init__(self, threshold, min_segment, close_last, documents, names, lengths, segment_ends, tags=None, probabilities=None):
        self.threshold, self.min_segment, self.close_last = float(threshold), int(min_segment), bool(close_last)
        self.documents = np.asarray(documents, dtype=np.int64).reshape(-1)
        n = self.documents.size
        self.names = None if names is None else list(names)
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        self.segment_ends = [np.asarray(e, dtype=np.int64).reshape(-1) for e in segment_ends]
        self.n_segments = np.array([e.size for e in self.segment_ends], dtype=np.int64)
        self.tags = None if tags is None else [np.asarray(t, dtype=np.uint8).reshape(-1) for t in tags]
        self.probabilities = None if probabilities is None else [np.asarray(p, dtype=np.float32).reshape(-1) for p in probabilities]
        for what, v in (('names', self.names), ('lengths', self.lengths), ('segment_ends', self.segment_ends), ('tags', self.tags),
                        ('probabilities', self.probabilities)):
            if v is not None and len(v) != n:
                raise ValueError(f'Prediction: {n} documents but {len(v)} {what}')

    def __len__(self):
        return int(self.documents.size)

    @classmethod
    def merge(cls, parts):
        """the parts of several ranks (or batches) -> one Prediction over their documents in ascending corpus index.  ValueError: no
        parts, parts decoded differently (threshold, min_segment, close_last, or only some with names / tags / probabilities), a document
        held twice, or a gap -- the merged documents must be exactly 0 .. n-1."""
        parts = list(parts)
        if not parts:
            raise ValueError('Prediction.merge: no parts')
        first = parts[0]
        full = [p for p in parts if len(p)] or [first]
        for p in parts:
            if (p.threshold, p.min_segment, p.close_last) != (first.threshold, first.min_segment, first.close_last):
                raise ValueError('Prediction.merge: the parts were decoded with different settings')
        for what in ('names', 'tags', 'probabilities'):
            if len({getattr(p, what) is None for p in full}) > 1:
                raise ValueError(f'Prediction.merge: only some parts carry {what}')
        documents = np.concatenate([p.documents for p in parts])
        order = np.argsort(documents, kind='stable')
        documents = documents[order]
        if documents.size and (np.diff(documents) == 0).any():
            raise ValueError(f'Prediction.merge: document {int(documents[1:][np.diff(documents) == 0][0])} is held more than once')
        if not np.array_equal(documents, np.arange(documents.size)):
            missing = sorted(set(range(int(documents.max()) + 1)) - set(documents.tolist()))
            raise ValueError(f'Prediction.merge: document {missing[0]} is missing')

        def gathered(what):
            if getattr(full[0], what) is None:
                return None
            flat = [v for p in parts if len(p) for v in getattr(p, what)]
            return [flat[i] for i in order.tolist()]
        return cls(first.threshold, first.min_segment, first.close_last, documents, gathered('names'),
                   np.concatenate([p.lengths for p in parts])[order], gathered('segment_ends'), gathered('tags'), gathered('probabilities'))

    def spans(self, times=None):
        """-> per document a list of (start, end): segment j covers sentences start .. end - 1 (sentence indices, end exclusive).  With
        ``times`` -- per document one [n, 2] array of every sentence's start and end in seconds -- each span is (the start of its first
        sentence, the end of its last).  Without ``close_last`` the sentences behind the last boundary belong to no span."""
        out = []
        for k, ends in enumerate(self.segment_ends):
            e = ends.tolist()
            pairs = list(zip([0] + e[:-1], e))
            if times is not None:
                t = np.asarray(times[k])
                if t.shape != (int(self.lengths[k]), 2):
                    raise ValueError(f'spans: times of document {int(self.documents[k])} are {t.shape}, not ({int(self.lengths[k])}, 2)')
                pairs = [(t[a, 0].item(), t[b - 1, 1].item()) for a, b in pairs]
            out.append(pairs)
        return out

    def pool(self, corpus, mode='mean', field='embeddings'):
        """-> (segment embeddings [total_segments, D or 2 D] on the device in the corpus' wire dtype, segment_doc int64 [total_segments] on
        the host): every predicted segment's sentences pooled in ``mode`` ('mean' | 'max' | 'mean_std' | 'max_std').  A predicted segment
        is a run of stored rows, so this is ``ops.frame_pool`` (csrc/frame_pool.hip) over the offsets row_start[d] + [0, ends ...]: no
        new kernel.  ValueError: a prediction without ``close_last`` (rows would belong to no segment), a truncated corpus, a corpus
        with other documents or lengths, an unknown mode or field."""
        if mode not in POOL_MODES:
            raise ValueError(f'pool: mode is one of {POOL_MODES}, not {mode!r}')
        if field not in ('embeddings', 'embeddings2'):
            raise ValueError(f"pool: field is 'embeddings' or 'embeddings2', not {field!r}")
        if not self.close_last:
            raise ValueError('pool: the prediction was made with close_last=False: the rows behind the last boundary belong to no segment')
        if corpus.truncate:
            raise ValueError('pool: the corpus truncates its documents: a predicted segment is not a run of stored rows')
        if len(self) != corpus.n_docs or not np.array_equal(self.lengths, corpus.rows):
            raise ValueError('pool: the prediction does not cover this corpus (documents or sentences per document differ)')
        x = corpus.corpus if field == 'embeddings' else corpus.corpus2
        if x is None:
            raise ValueError("pool: field='embeddings2' needs a corpus with a second input")
        if x.device.type != 'cuda':
            raise RuntimeError('Prediction.pool reduces on the GPU (there is no CPU fallback)')
        offsets = np.concatenate([[0]] + [corpus._start_host[d] + e for d, e in zip(self.documents.tolist(), self.segment_ends)]).astype(np.int64)
        segment_doc = np.repeat(self.documents, self.n_segments)
        width = 2 if mode.endswith('_std') else 1
        with torch.cuda.device(x.device):
            out = torch.empty((segment_doc.size, width * int(x.shape[1])), dtype=x.dtype, device=x.device)
            if segment_doc.size:
                ops.frame_pool(x, torch.from_numpy(offsets).to(x.device), out, first=mode.split('_')[0], with_std=mode.endswith('_std'))
        return out, segment_doc

    def as_saturated(self, device):
        """-> fp32 [documents, longest, 1] on ``device``: +30 where the tag is 1, -30 elsewhere -- the logits ``evaluate`` feeds its sweeps
        for a hypothesis without a threshold.  From ``tags`` when they were kept; else from the segment ends, which say the same unless
        ``close_last`` added a tail (the last sentence's tag is then not recoverable): ValueError."""
        if self.tags is not None:
            tags = self.tags
        elif self.close_last:
            raise ValueError('as_saturated: under close_last the last end does not say whether the last sentence was tagged; '
                             'predict(..., return_tags=True) keeps the tags')
        else:
            tags = []
            for n, ends in zip(self.lengths.tolist(), self.segment_ends):
                t = np.zeros(n, dtype=np.uint8)
                t[ends - 1] = 1
                tags.append(t)
        return _saturated(tags, int(self.lengths.max()) if len(self) else 0, device)


def _threshold_of(model, threshold):
    th = threshold if threshold is not None else getattr(model, 'th', None)
    if th is None:
        th = FALLBACK_THRESHOLD
    if not th:
        th = 0.5
    return float(th)


def predict(trainer_or_model, corpus, *, batch_size=8, threshold=None, min_segment=1, close_last=True, return_tags=False,
            return_probabilities=False):
    """-> Prediction over every document of ``corpus`` (a ``ResidentCorpus``, labelled or from ``from_documents``), the same on every rank.
    ``trainer_or_model``: a ``NativeTrainer`` (rank, world and process group are its) or a bare tagger / ``TextSegmenter``.
    ``min_segment``: 1 is the threshold rule, bit for bit the tags of the tagger's own forward; m >= 2 the constrained decode (module
    docstring; ValueError for ``BiRnnCrf(decode='viterbi')``).  ``close_last``: a document that does not end on a boundary still ends its
    last segment.  ``return_tags`` / ``return_probabilities``: also read the tags / the tags and the decode probabilities back (for SheikhBiLSTM the
    probability is sigmoid(score), compared with 1 - threshold).  The reported ``threshold`` is 0.5 for the Viterbi path."""
    model, rank, world, pg, merge = _unwrap(trainer_or_model)
    n_docs = len(corpus)
    if n_docs == 0:
        raise ValueError('predict: the corpus has no documents')
    m = int(min_segment)
    if m < 1:
        raise ValueError(f'predict: min_segment={min_segment}; a segment holds at least one sentence')
    viterbi = decodes_by_viterbi(model)                # BiRnnCrf / TransformerCRF in their default decode
    if viterbi and m > 1:
        raise ValueError("predict: min_segment > 1 needs probabilities; BiRnnCrf(decode='viterbi') has a path, not scores "
                         "(decode='marginal' gives them)")
    reported = 0.5 if viterbi else _threshold_of(model, threshold)
    at = 1.0 - reported if isinstance(model, SheikhBiLSTM) else reported
    docs = list(range(rank, n_docs, world))
    dev = model.flat.device
    lengths, ends, tags, probs = [], [], [], []
    return_tags = bool(return_tags or return_probabilities)
    was_training = model.training
    model.eval()
    try:
        if not hasattr(model, 'th'):
            model.th = None                            # SheikhBiLSTM's forward reads it (upstream never sets it before test_step does)
        with torch.cuda.device(dev):
            for s in range(0, len(docs), batch_size):
                idx = docs[s:s + batch_size]
                batch = corpus.batch(idx)
                if viterbi:
                    scores = _saturated(model(batch['src_tokens'], batch['src_lengths'])[1], batch['src_tokens'].shape[1], dev)
                else:
                    scores = _forward(model, batch).detach().to(torch.float32).contiguous()
                B, Lq = int(scores.shape[0]), int(scores.shape[1])
                li = batch['src_lengths'].to(device=dev, dtype=torch.int32).contiguous()
                table = torch.empty(B * (Lq + 1), dtype=torch.int32, device=dev)            # the ends and, behind them, the counts: one copy back
                tag_d = torch.empty((B, Lq), dtype=torch.uint8, device=dev) if return_tags else None
                prob_d = torch.empty((B, Lq), dtype=torch.float32, device=dev) if return_probabilities else None
                ops.segment_decode(scores, li, at, table[:B * Lq].view(B, Lq), table[B * Lq:], min_segment=m, close_last=close_last,
                                   tags=tag_d, prob=prob_d)
                host = table.cpu().numpy()
                seg_end, n_seg = host[:B * Lq].reshape(B, Lq), host[B * Lq:]
                lens = np.minimum(batch['src_lengths'].numpy().astype(np.int64), Lq)
                lengths.append(lens)
                ends += [seg_end[b, :int(n_seg[b])].astype(np.int64) for b in range(B)]
                if return_tags:
                    h = tag_d.cpu().numpy()
                    tags += [h[b, :int(lens[b])].copy() for b in range(B)]
                if return_probabilities:
                    h = prob_d.cpu().numpy()
                    probs += [h[b, :int(lens[b])].copy() for b in range(B)]
    finally:
        model.train(was_training)
    names = getattr(corpus, 'names', None)
    mine = Prediction(reported, m, close_last, docs, None if names is None else [names[d] for d in docs],
                      np.concatenate(lengths) if lengths else np.zeros(0, dtype=np.int64), ends, tags if return_tags else None,
                      probs if return_probabilities else None)
    if merge and world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, mine, group=pg)
        return Prediction.merge(parts)
    return Prediction.merge([mine])


def segment_audio(n_samples, segmentation, sr=16000, interval=1, adaptive=False):
    """-> the (start, end) sample spans the reference's ``BasePredictor.segment_audio`` (predict.py:92-129) cuts a recording of
    ``n_samples`` samples at rate ``sr`` into, given one flag per basic unit, without loading audio.  Uniform units (``adaptive=False``):
    a unit is ``sr * int(interval)`` samples; a set flag closes a span at the unit's end; flags that run out stop the walk; ``(previous
    end, n_samples)`` is ALWAYS appended, also when it is empty.  Adaptive units: 100 units of ``n_samples // 100`` samples; no tail is
    appended, and running out of flags raises IndexError as upstream does (it happens when ``n_samples // 100`` does not divide
    ``n_samples`` and the list has 100 entries: the walk makes a 101st step)."""
    n_samples = int(n_samples)
    spans, previous, unit = [], 0, 0
    if adaptive:
        step = n_samples // 100
        for end in range(step, n_samples + 1, step):
            if segmentation[unit]:
                spans.append((previous, end))
                previous = end
            unit += 1
        return spans
    step = int(sr) * int(interval)
    for end in range(step, n_samples + 1, step):
        if unit >= len(segmentation):
            break
        if segmentation[unit]:
            spans.append((previous, end))
            previous = end
        unit += 1
    spans.append((previous, n_samples))
    return spans
