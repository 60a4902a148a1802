"""The corpus lives in HBM: batches are GATHERED on the device, and every data-parallel rank gathers only its own documents.

The corpora this tagger trains on are tiny next to the memory of the card (RadioNews: 55 documents, 33 179 sentences -- 119 MB in bf16
at D = 1792, 238 MB in fp32, against 288 GB), so the fastest host collater is no host collater:

  * ``ResidentCorpus(dataset, device)`` concatenates the documents of an ``AudioPortionDataset`` (any mode: early or late fusion,
    domains, segments, truncate on or off, CRF pad) into one [total_rows, D] device tensor per input plus a [total_rows] fp32 tensor of
    targets, uploaded ONCE;
  * ``corpus.batch(indices, pad_to=None)`` returns the batch dict a collated batch has after ``DevicePrefetcher``: ``src_tokens``,
    ``src_tokens2`` (or None) and ``tgt_tokens`` built on the device by ``ops.gather_pad`` (csrc/gather.hip: one launch per tensor on the
    current stream, every element written, no memset), ``src_lengths`` (int64), ``id``, ``domain`` and ``src_segments`` on the host
    from tables made at construction.  The only per-call transfer is one asynchronous copy of the B int32 indices out of a small
    pinned ring; nothing synchronises and nothing pageable is copied.  In fp32 the tensors are ``torch.equal`` to
    ``dataset.collater([dataset[i] for i in indices])`` (the reference path, EncoderDataset.py:91-152) moved to the device, with
    ``wire_dtype='bf16'`` the embeddings equal that batch's ``.to(torch.bfloat16)``; repeats in ``indices`` are allowed;
  * ``DocumentShardSampler(lengths, batch_size, rank, world)`` yields ``(local_indices, pad_to)`` per global batch: the documents
    ``global_batch[rank::world]`` (the rule of ``trainer.shard_batch``) and the longest document of the WHOLE global batch, computed from
    the host length table -- every rank pads to the same length without a collective, so ``NativeTrainer._check_same_length`` passes
    and no rank collates documents it then throws away;
  * ``corpus.batch_segments(indices, orders, close_last)`` is ``batch()`` with every document's topic segments in a listed order, and
    ``corpus.augmented('reverse' | 'shuffle')`` an ``AugmentedCorpus``: a view with a reordered twin of every document (segment-order
    augmentation, the reference's ``inverse_augmentation``) made by the gather itself (``ops.gather_segments``, the same file): the same
    bytes moved, no second copy of the corpus, a few hundred more integers in the per-call copy;
  * ``corpus.batch_masked(indices, doc_seeds, mask_probability)`` is ``batch()`` with a random share of every document's negative
    sentences dropped, and ``corpus.masked(mask_probability, seed)`` a ``MaskedCorpus``: a view whose documents are masked anew every
    epoch (negative-sentence masking, the reference's ``--mask_inner_sentences``).  ``ops.mask_plan`` (csrc/mask_plan.hip) draws and
    compacts on the device, ``ops.gather_rows`` builds the tensors from its row table: two more integers per document in the per-call copy;
  * ``corpus.fit_pca(n_components)`` fits a ``pca.PcaReducer`` on the resident rows (the reference's ``--pca_reduce``; moments by
    ``ops.pca_colsum`` / ``ops.pca_gram``, csrc/pca.hip) and ``corpus.projected(reducer)`` is the corpus at width k (``ops.pca_project``):
    every method above reads the width from the matrix and takes it as it is;
  * ``corpus.with_frames(frames, mode, field)`` takes an input from frame-level audio features pooled per sentence on the device
    (``frames.ResidentFrames``, csrc/frame_pool.hip; the reference's six pooled variants): as the first input, as the second, or
    early-fused behind the stored columns;
  * ``ResidentCorpus.from_documents(embeddings, device, names=)`` is an UNLABELLED corpus from a list of [sentences, D] matrices (what
    ``load_dataset_for_inference`` returns): all-zero targets, ``labelled = False``, for ``predict.predict``; ``fit`` and ``evaluate``
    refuse it.

For every tagger but ``SwitchBiLSTM(switch='dense')`` (see ``trainer.shard_batch``), ``corpus.batch(*item)`` on rank r holds the bits of
``shard_batch(collated global batch, r, world)``.  ``NativeTrainer.step`` takes these batches as they are.
"""
import numpy as np
import torch

_WIRE = {'fp32': torch.float32, 'bf16': torch.bfloat16}
_RING_SLOTS = 16
_M64 = (1 << 64) - 1


def _hash32(seed, idx):
    """mts_hash32(seed, idx) of csrc/common.h (the counter hash of the dropout kernels) over uint64 arrays -> uint64 array holding the
    32-bit values; ``seed`` is one value or an array of ``idx``'s shape"""
    seed, idx = np.asarray(seed, dtype=np.uint64), np.asarray(idx, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = seed + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(32)


def mask_doc_seeds(seed, epoch, n_docs, docs=None):
    """uint64 seeds of the masking draws of documents ``docs`` (None: all of them) in ``epoch``:
    (mts_hash32(seed, 2c) << 32) | mts_hash32(seed, 2c + 1) with c = epoch * n_docs + d, in 64-bit wrapping arithmetic"""
    d = np.arange(n_docs, dtype=np.uint64) if docs is None else np.asarray(docs, dtype=np.int64).astype(np.uint64)
    with np.errstate(over='ignore'):
        c2 = (np.uint64((int(epoch) * int(n_docs)) & _M64) + d) * np.uint64(2)
        s = np.uint64(int(seed) & _M64)
        return (_hash32(s, c2) << np.uint64(32)) | _hash32(s, c2 + np.uint64(1))


def _keep_probability(p, who):
    p = float(p)
    if not 0.0 <= p <= 1.0:                                                        # a NaN fails both comparisons
        raise ValueError(f'{who}: mask_probability is the probability that a negative sentence is KEPT and lies in [0, 1], not {p}')
    return p


def _rows_2d(items, what):
    """documents -> list of contiguous fp32 / bf16 [rows, D] host tensors of one width"""
    out = []
    for k, e in enumerate(items):
        t = torch.as_tensor(e)
        if t.dim() != 2:
            raise ValueError(f'ResidentCorpus: {what} of document {k} is {t.dim()}-d; [sentences, D] matrices are expected')
        out.append(t)
    widths = {int(t.shape[1]) for t in out}
    if len(widths) > 1:
        raise ValueError(f'ResidentCorpus: {what} widths differ between documents: {sorted(widths)}')
    return out


class _UnlabelledDocuments:
    """what ``ResidentCorpus.__init__`` reads of a dataset, for a list of documents without labels (``from_documents``)"""
    truncate, tv, minus, segments = False, 0, 1, False

    def __init__(self, embeddings, embeddings2, domain):
        self.embeddings = list(embeddings)
        self.embeddings2 = list(embeddings2) if embeddings2 is not None else []
        self.tgt_dataset = [torch.zeros(int(torch.as_tensor(e).shape[0]) if torch.as_tensor(e).dim() else 0) for e in self.embeddings]
        self.da = domain is not None
        self.domain = list(domain) if domain is not None else [None] * len(self.embeddings)
        if len(self.domain) != len(self.embeddings):
            raise ValueError(f'ResidentCorpus.from_documents: {len(self.embeddings)} documents but {len(self.domain)} domains')

    def __len__(self):
        return len(self.embeddings)


class ResidentCorpus:
    labelled = True                 # False for a corpus of ``from_documents``: fit and evaluate refuse it, predict takes either
    names = None                    # the documents' file names (``from_documents(names=...)``)

    @classmethod
    def from_documents(cls, embeddings, device, wire_dtype='fp32', embeddings2=None, names=None, domain=None):
        """-> an UNLABELLED corpus from a list of [sentences, D] matrices -- what ``datasets.load_dataset_for_inference`` returns next to
        the file names (the reference's predict.py:293-300: AudioPortionDatasetInference over that list).  Targets are all zero, nothing
        is truncated, ``names`` (the file names, or None) is kept as ``corpus.names`` and ``corpus.labelled`` is False.  ``batch``,
        ``projected(reducer)`` and ``with_frames`` work on it as they are; ``fit`` and ``evaluate`` refuse it -- ``predict`` is the pass
        that needs no labels.  ValueError: no documents, a document that is no matrix, widths that differ, names / domains / a second
        input of another length."""
        out = cls(_UnlabelledDocuments(embeddings, embeddings2, domain), device, wire_dtype=wire_dtype)
        if names is not None:
            names = list(names)
            if len(names) != out.n_docs:
                raise ValueError(f'ResidentCorpus.from_documents: {out.n_docs} documents but {len(names)} names')
        out.names, out.labelled = names, False
        return out

    def __init__(self, dataset, device, wire_dtype=None, segments=None):
        """dataset: an AudioPortionDataset; wire_dtype: 'fp32' | 'bf16' | None (the dataset's own); segments: add 'src_segments' to the
        batches (None: as the dataset does)."""
        if wire_dtype is None:
            wire_dtype = 'bf16' if getattr(dataset, 'wire', torch.float32) == torch.bfloat16 else 'fp32'
        if wire_dtype not in _WIRE:
            raise ValueError("wire_dtype must be 'fp32' or 'bf16'")
        self.wire = _WIRE[wire_dtype]
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.truncate, self.tv, self.minus = bool(dataset.truncate), int(dataset.tv), int(dataset.minus)
        self.segments = bool(dataset.segments if segments is None else segments)
        self.da = bool(dataset.da)
        self.domain = list(dataset.domain)
        if len(dataset) == 0:
            raise ValueError('ResidentCorpus: the dataset has no documents')
        emb = _rows_2d(dataset.embeddings, 'embeddings')
        emb2 = _rows_2d(dataset.embeddings2, 'second-input embeddings') if dataset.embeddings2 else None
        tgt = [torch.as_tensor(t).to(torch.float32).reshape(-1) for t in dataset.tgt_dataset]
        rows = np.array([int(t.shape[0]) for t in emb], dtype=np.int64)
        for k, t in enumerate(tgt):
            if int(t.shape[0]) != rows[k]:
                raise ValueError(f'ResidentCorpus: document {k} has {int(rows[k])} sentences but {int(t.shape[0])} targets')
        if emb2 is not None and (len(emb2) != len(emb) or any(int(t.shape[0]) != rows[k] for k, t in enumerate(emb2))):
            raise ValueError('ResidentCorpus: the second input does not have the first input\'s sentences per document')
        self.n_docs = len(emb)
        self.rows = rows                                                           # sentences per document, as stored
        self.lengths = np.minimum(rows, self.tv) if self.truncate else rows.copy()  # what a batch reports as src_lengths
        start = np.zeros(self.n_docs + 1, dtype=np.int64)
        np.cumsum(rows, out=start[1:])
        self.total_rows = int(start[-1])
        # per-document segment ends, what AudioPortionDataset._segments_of makes from the collated batch: the positions just behind
        # the boundary sentences inside the reported length
        self._segment_ends = [(np.flatnonzero(t.numpy()[:int(n)] == 1) + 1).tolist() for t, n in zip(tgt, self.lengths)] if self.segments else None
        # the topic segments of the STORED rows (segment-order augmentation): document d's segment j is rows _seg_bounds[d][j] ..
        # _seg_bounds[d][j + 1]; a segment ends behind a label 1, and what follows the last 1 is the tail
        self._seg_bounds, self._has_tail, self._binary_labels = [], np.zeros(self.n_docs, dtype=bool), True
        for k, t in enumerate(tgt):
            y = t.numpy()
            ones = y == 1
            self._binary_labels = self._binary_labels and bool((ones | (y == 0)).all())
            ends = np.flatnonzero(ones) + 1
            self._has_tail[k] = bool(rows[k]) and not bool(ones[-1])
            self._seg_bounds.append(np.concatenate([[0], ends, [rows[k]] if self._has_tail[k] else []]).astype(np.int64))
        self.n_segments = np.array([b.size - 1 for b in self._seg_bounds], dtype=np.int64)     # segments per document, the tail included
        self._seg_flat = np.concatenate(self._seg_bounds)                                      # the same bounds, one array: batch_segments
        self._seg_base = np.concatenate([[0], np.cumsum(self.n_segments + 1)[:-1]]).astype(np.int64)

        def upload(docs):
            # fp32 first: the values the reference's `merge` writes into its fp32 batch; bf16 is that batch's .to(torch.bfloat16)
            return torch.cat([t.to(torch.float32) for t in docs]).to(self.wire).contiguous().to(self.device)
        self.corpus = upload(emb)
        self.corpus2 = upload(emb2) if emb2 is not None else None
        self.targets = torch.cat(tgt).contiguous().to(self.device)
        self.row_start = torch.from_numpy(start).to(self.device)
        # host copies of the labels and the row table (4 bytes per sentence): the host half of negative-sentence masking draws from them
        self._labels_host = torch.cat(tgt).numpy().copy()
        self._start_host = start
        self._ring = None
        self._turn = 0

    def __len__(self):
        return self.n_docs

    @property
    def nbytes(self):
        """bytes of the resident data (embeddings, second input, targets, row table)"""
        return sum(t.numel() * t.element_size() for t in (self.corpus, self.corpus2, self.targets, self.row_start) if t is not None)

    def sampler(self, batch_size, **kw):
        """a DocumentShardSampler over this corpus (with truncate=True every batch is truncate_value long: no pad_to)"""
        return DocumentShardSampler(self.n_docs if self.truncate else self.lengths, batch_size, **kw)

    # ---- host half ---------------------------------------------------------------------------------------------------------
    def _indices(self, indices):
        ii = np.asarray(indices, dtype=np.int64).reshape(-1)
        if ii.size and (int(ii.min()) < 0 or int(ii.max()) >= self.n_docs):
            raise IndexError(f'ResidentCorpus: document index outside 0 .. {self.n_docs - 1}')
        return ii

    def _padded_length(self, ii, pad_to):
        if self.truncate:
            if pad_to is not None:
                raise ValueError('pad_to cannot be combined with truncate=True (every batch is truncate_value long)')
            return self.tv
        longest = int(self.rows[ii].max())
        if pad_to is None:
            return longest
        if int(pad_to) < longest:
            raise ValueError(f'pad_to {int(pad_to)} is shorter than the longest listed document ({longest})')
        return int(pad_to)

    def _host_fields(self, ii, pad_to):
        Lmax = self._padded_length(ii, pad_to)
        idx = ii.tolist()
        out = {'id': torch.from_numpy(ii.copy()), 'src_lengths': torch.from_numpy(self.lengths[ii].astype(np.int64, copy=True)),
               'domain': [self.domain[i] for i in idx] if self.da else None}
        if self.segments:
            out['src_segments'] = [list(self._segment_ends[i]) for i in idx]
        return out, Lmax

    def host_fields(self, indices, pad_to=None):
        """-> ({'id', 'src_lengths', 'domain'(, 'src_segments')}, padded length) of the batch of documents ``indices``: the host half
        of ``batch()``; touches no GPU.  An empty list gives ({}, 0)."""
        ii = self._indices(indices)
        if ii.size == 0:
            return {}, 0
        return self._host_fields(ii, pad_to)

    # ---- device half -------------------------------------------------------------------------------------------------------
    def _upload_indices(self, ii):
        """the B indices as an int32 device tensor: written into a slot of a pinned ring, one asynchronous copy on the current stream.
        A slot is written again _RING_SLOTS calls later; its copy's event is waited for only if the device is that far behind."""
        B = ii.size
        if self._ring is None:
            self._ring = [[None, None] for _ in range(_RING_SLOTS)]
        slot = self._ring[self._turn % _RING_SLOTS]
        self._turn += 1
        if slot[0] is None or slot[0].numel() < B:
            slot[0] = torch.empty(max(B, 64), dtype=torch.int32).pin_memory()
            slot[1] = torch.cuda.Event()
        elif not slot[1].query():
            slot[1].synchronize()
        slot[0].numpy()[:B] = ii
        dev = torch.empty(B, dtype=torch.int32, device=self.device)
        dev.copy_(slot[0][:B], non_blocking=True)
        slot[1].record()
        return dev

    def batch(self, indices, pad_to=None):
        """the batch dict of documents ``indices`` (module docstring).  {} for an empty list; IndexError for an index outside the corpus;
        ValueError for a pad_to below the longest listed document or together with truncate=True."""
        ii = self._indices(indices)
        if ii.size == 0:
            return {}
        out, Lmax = self._host_fields(ii, pad_to)
        if self.device.type != 'cuda':
            raise RuntimeError('ResidentCorpus.batch gathers on the GPU (there is no CPU fallback); host_fields() is the part that needs none')
        from . import ops
        with torch.cuda.device(self.device):
            B = int(ii.size)
            idx = self._upload_indices(ii)
            out['src_tokens'] = ops.gather_pad(self.corpus, self.row_start, idx,
                                               torch.empty((B, Lmax, self.corpus.shape[1]), dtype=self.wire, device=self.device))
            out['src_tokens2'] = None if self.corpus2 is None else ops.gather_pad(
                self.corpus2, self.row_start, idx, torch.empty((B, Lmax, self.corpus2.shape[1]), dtype=self.wire, device=self.device))
            # pad -1, or 0 for the CRF head (EncoderDataset.py:23)
            out['tgt_tokens'] = ops.gather_pad(self.targets, self.row_start, idx, torch.empty((B, Lmax), dtype=torch.float32, device=self.device),
                                               pad_value=0.0 - self.minus)
        return out

    # ---- segment-order augmentation ------------------------------------------------------------------------------------------
    def _segment_tables(self, ii, orders, close_last):
        """host tables of batch_segments -> (seg_ptr [B + 1], seg_dst [S], seg_src [S], augmented rows [B], close flags [B]) as int64 /
        bool arrays.  Built from the segment table made at construction: O(listed segments), never O(rows)."""
        if not self._binary_labels:
            raise ValueError('ResidentCorpus: segment orders need targets that are 0 or 1 everywhere (a segment ends behind a 1)')
        B = int(ii.size)
        if len(orders) != B:
            raise ValueError(f'batch_segments: {B} documents but {len(orders)} orders')
        close = np.asarray(close_last, dtype=bool).reshape(-1)
        if close.size not in (1, B):
            raise ValueError(f'batch_segments: close_last is one flag or one per document ({B}), not {close.size}')
        close = np.broadcast_to(close, (B,))
        arrs = [np.asarray(o, dtype=np.int64).reshape(-1) for o in orders]
        counts = np.array([a.size for a in arrs], dtype=np.int64)
        if not counts.all():
            d = int(ii[int(np.flatnonzero(counts == 0)[0])])
            raise ValueError(f'batch_segments: the order of document {d} is empty (a zero-length document is not a batch row)')
        o = np.concatenate(arrs)
        doc = np.repeat(ii, counts)                                              # the stored document of every listed segment
        bad = np.flatnonzero((o < 0) | (o >= self.n_segments[doc]))
        if bad.size:
            d = int(doc[bad[0]])
            raise ValueError(f'batch_segments: document {d} has segments 0 .. {int(self.n_segments[d]) - 1}; its order lists {int(o[bad[0]])}')
        key = np.repeat(np.arange(B, dtype=np.int64), counts) * (int(self.n_segments.max()) + 1) + o
        if np.unique(key).size != key.size:
            raise ValueError('batch_segments: an order lists a segment twice')
        at = self._seg_base[doc] + o
        first = self._seg_flat[at]
        ln = self._seg_flat[at + 1] - first
        ptr = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(counts, out=ptr[1:])
        c = np.cumsum(ln)
        before = np.concatenate([[0], c[ptr[1:-1] - 1]])                         # rows listed in front of every document
        return ptr, c - ln - np.repeat(before, counts), first, c[ptr[1:] - 1] - before, close

    def _segment_host_fields(self, ii, tables, pad_to):
        ptr, dst_off, _, rows, close = tables
        lengths = np.minimum(rows, self.tv) if self.truncate else rows
        if self.truncate:
            if pad_to is not None:
                raise ValueError('pad_to cannot be combined with truncate=True (every batch is truncate_value long)')
            Lmax = self.tv
        else:
            Lmax = int(rows.max())
            if pad_to is not None:
                if int(pad_to) < Lmax:
                    raise ValueError(f'pad_to {int(pad_to)} is shorter than the longest augmented document ({Lmax})')
                Lmax = int(pad_to)
        out = {'id': torch.from_numpy(ii.copy()), 'src_lengths': torch.from_numpy(lengths.astype(np.int64, copy=True)),
               'domain': [self.domain[i] for i in ii.tolist()] if self.da else None}
        if self.segments:
            # the positions just behind the augmented labels' ones, inside the reported length: every listed segment's end but the last
            # one's, and the document's own end when close_last
            out['src_segments'] = []
            for k in range(int(ii.size)):
                ends = dst_off[ptr[k] + 1:ptr[k + 1]].tolist() + ([int(rows[k])] if close[k] else [])
                out['src_segments'].append([e for e in ends if e <= int(lengths[k])])
        return out, Lmax

    def batch_segments(self, indices, orders, close_last, pad_to=None):
        """``batch()`` with every document's topic segments in a listed order (segment-order augmentation, the reference's
        ``cross_validation_split(inverse_augmentation=True)``, utils/load_datasets_precomputed.py:71-96, moved into the gather).

        Document d has ``n_segments[d]`` segments: segment j ends behind the j-th label 1, and the rows behind the last 1 are the tail
        (the loader forces the last label to 0, so loaded documents always have one).  ``orders[k]`` is a non-empty sequence of distinct
        segment numbers of document ``indices[k]`` -- a subset is fine -- and ``close_last`` one bool, or one per document.  Row k of the
        batch holds the rows of the listed segments in that order; its labels are 0 except a 1 on the last row of every listed segment,
        and ``close_last`` on the very last row.  ``src_lengths`` are the augmented lengths (cut at truncate_value by a truncate=True
        corpus, as a stored document is), ``src_segments`` the positions behind the augmented labels' ones, ``src_tokens2`` is reordered
        with ``src_tokens``, ``domain`` is the stored document's.  Same keys, dtypes and devices as ``batch()``.

        Everything is validated on the host before a launch: IndexError for an index outside the corpus; ValueError for an empty order,
        a repeated or unknown segment number, a pad_to below the longest augmented document, and a corpus whose targets are not all 0 / 1.
        The tables travel with the indices in ONE asynchronous copy out of the pinned ring; the tensors are built by
        ``ops.gather_segments`` (one launch each, every element written)."""
        ii = self._indices(indices)
        if ii.size == 0:
            return {}
        tables = self._segment_tables(ii, orders, close_last)
        out, Lmax = self._segment_host_fields(ii, tables, pad_to)
        if self.device.type != 'cuda':
            raise RuntimeError('ResidentCorpus.batch_segments gathers on the GPU (there is no CPU fallback)')
        from . import ops
        ptr, dst_off, src_off, rows, close = tables
        with torch.cuda.device(self.device):
            B, S = int(ii.size), int(dst_off.size)
            dev = self._upload_indices(np.concatenate([ii, ptr, rows, close.astype(np.int64), dst_off, src_off]))
            cut = np.cumsum([B, B + 1, B, B, S, S]).tolist()
            idx, seg_ptr, dst_len, close_dev, seg_dst, seg_src = (dev[a:b] for a, b in zip([0] + cut[:-1], cut))

            def gather(corpus, dst, **kw):
                return ops.gather_segments(corpus, self.row_start, idx, seg_ptr, seg_dst, seg_src, dst_len, dst, **kw)
            out['src_tokens'] = gather(self.corpus, torch.empty((B, Lmax, self.corpus.shape[1]), dtype=self.wire, device=self.device))
            out['src_tokens2'] = None if self.corpus2 is None else gather(
                self.corpus2, torch.empty((B, Lmax, self.corpus2.shape[1]), dtype=self.wire, device=self.device))
            out['tgt_tokens'] = gather(self.targets, torch.empty((B, Lmax), dtype=torch.float32, device=self.device),
                                       pad_value=0.0 - self.minus, close_last=close_dev)
        return out

    def augmented(self, mode, seed=0):
        """-> AugmentedCorpus(self, mode, seed): 2 x n_docs virtual documents, every stored one and its twin with the segments reordered"""
        return AugmentedCorpus(self, mode, seed=seed)

    # ---- negative-sentence masking -------------------------------------------------------------------------------------------
    def _mask_plan_host(self, ii, seeds, p):
        """the host's plan of masking documents ``ii`` under ``seeds`` (uint64, one per listed document): the rule of mts_mask_plan
        (include/mts.h) in one vectorised pass over the listed documents' labels -> (kept rows per document [B], the kept rows' indices
        inside their documents, concatenated, where every document's start in that list [B + 1], the kept rows' labels)"""
        B = int(ii.size)
        rows = self.rows[ii]
        ptr = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(rows, out=ptr[1:])
        which = np.repeat(np.arange(B, dtype=np.int64), rows)
        rel = np.arange(int(ptr[-1]), dtype=np.int64) - ptr[which]
        y = self._labels_host[self._start_host[ii][which] + rel]
        keep = (y != 0) | (_hash32(seeds[which], rel) < np.uint64(min(int(p * 4294967296.0), 1 << 32)))
        seen = np.concatenate([[0], np.cumsum(keep)])
        counts = (seen[ptr[1:]] - seen[ptr[:-1]]).astype(np.int64)
        empty = (counts == 0) & (rows > 0)
        if empty.any():                                                   # the empty-draw rule: row 0 of such a document stays
            keep[ptr[:-1][empty]] = True
            counts[empty] = 1
        flat = np.flatnonzero(keep)
        kept_ptr = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(counts, out=kept_ptr[1:])
        return counts, rel[flat], kept_ptr, y[flat]

    def _masked_segment_ends(self, counts, kept_ptr, kept_labels):
        """src_segments of masked documents: the positions just behind the kept rows that are boundaries, inside the reported length"""
        lengths = np.minimum(counts, self.tv) if self.truncate else counts
        return [(np.flatnonzero(kept_labels[int(s):int(s) + int(n)] == 1) + 1).tolist() for s, n in zip(kept_ptr[:-1], lengths)]

    def _masked_host_fields(self, ii, counts, segment_ends, pad_to):
        lengths = np.minimum(counts, self.tv) if self.truncate else counts
        if self.truncate:
            if pad_to is not None:
                raise ValueError('pad_to cannot be combined with truncate=True (every batch is truncate_value long)')
            Lmax = self.tv
        else:
            Lmax = int(counts.max())
            if pad_to is not None:
                if int(pad_to) < Lmax:
                    raise ValueError(f'pad_to {int(pad_to)} is shorter than the longest masked document ({Lmax})')
                Lmax = int(pad_to)
        out = {'id': torch.from_numpy(ii.copy()), 'src_lengths': torch.from_numpy(lengths.astype(np.int64, copy=True)),
               'domain': [self.domain[i] for i in ii.tolist()] if self.da else None}
        if self.segments:
            out['src_segments'] = [list(s) for s in segment_ends]
        return out, Lmax

    def batch_masked(self, indices, doc_seeds, mask_probability, pad_to=None, lengths=None, segment_ends=None, return_plan=False):
        """``batch()`` of documents ``indices`` with a random share of their negative sentences dropped (negative-sentence masking, the
        reference's ``--mask_inner_sentences``, utils/load_datasets_precomputed.py:174-185, moved into the gather).

        Row r of document ``indices[k]`` stays when its label is not 0 or when ``mts_hash32(doc_seeds[k], r) < mask_probability * 2^32``:
        ``mask_probability`` is the probability that a negative sentence is KEPT (the reference's code, not its help text); a document
        none of whose rows stays keeps row 0.  The kept rows move up in order; embeddings, second input and labels travel together and the
        labels are not rewritten.  ``doc_seeds``: one uint64 per listed document (``mask_doc_seeds``).  ``src_lengths`` are the kept
        lengths (cut at truncate_value by a truncate=True corpus, as a stored document is), ``src_segments`` the positions behind the
        kept boundaries inside them.  Same keys, dtypes and devices as ``batch()``.

        ``lengths`` (and ``segment_ends`` for a segments=True corpus): the kept rows per listed document (and their 'src_segments') when
        the caller already has them -- MaskedCorpus does, from its plan of the epoch, and then nothing O(sentences) runs on the host here.
        Without them they are computed from the host copy of the listed documents' labels.  The device never reports them back in this
        path; ``return_plan=True`` returns ``(batch, src_row, kept)`` with the device's int32 plan [B, Lmax] and counts [B] next to it.

        One ``ops.mask_plan`` launch and one ``ops.gather_rows`` launch per tensor on the current stream; the seeds travel with the indices
        in ONE asynchronous copy out of the pinned ring.  ValueError for a mask_probability outside [0, 1], a seed list of another length
        and a pad_to below the longest masked document; IndexError for an index outside the corpus."""
        ii = self._indices(indices)
        p = _keep_probability(mask_probability, 'batch_masked')
        if ii.size == 0:
            return ({}, None, None) if return_plan else {}
        B = int(ii.size)
        seeds = np.ascontiguousarray(np.asarray(doc_seeds, dtype=np.uint64).reshape(-1))
        if seeds.size != B:
            raise ValueError(f'batch_masked: {B} documents but {seeds.size} seeds')
        if lengths is None:
            counts, _, kept_ptr, kept_labels = self._mask_plan_host(ii, seeds, p)
            segment_ends = self._masked_segment_ends(counts, kept_ptr, kept_labels) if self.segments else None
        else:
            counts = np.asarray(lengths, dtype=np.int64).reshape(-1)
            if counts.size != B or (self.segments and (segment_ends is None or len(segment_ends) != B)):
                raise ValueError(f'batch_masked: lengths (and segment_ends of a segments=True corpus) are one per listed document ({B})')
        out, Lmax = self._masked_host_fields(ii, counts, segment_ends, pad_to)
        if self.device.type != 'cuda':
            raise RuntimeError('ResidentCorpus.batch_masked gathers on the GPU (there is no CPU fallback)')
        from . import ops
        with torch.cuda.device(self.device):
            # the seeds first: their 8-byte alignment is the allocation's
            dev = self._upload_indices(np.concatenate([seeds.view(np.int32).astype(np.int64), ii]))
            seed_dev, idx = dev[:2 * B].view(torch.int64), dev[2 * B:]
            src_row, kept = ops.mask_plan(self.targets, self.row_start, idx, seed_dev, p,
                                          torch.empty((B, Lmax), dtype=torch.int32, device=self.device),
                                          torch.empty(B, dtype=torch.int32, device=self.device))

            def gather(corpus, dst, **kw):
                return ops.gather_rows(corpus, self.row_start, idx, src_row, dst, **kw)
            out['src_tokens'] = gather(self.corpus, torch.empty((B, Lmax, self.corpus.shape[1]), dtype=self.wire, device=self.device))
            out['src_tokens2'] = None if self.corpus2 is None else gather(
                self.corpus2, torch.empty((B, Lmax, self.corpus2.shape[1]), dtype=self.wire, device=self.device))
            out['tgt_tokens'] = gather(self.targets, torch.empty((B, Lmax), dtype=torch.float32, device=self.device), pad_value=0.0 - self.minus)
        return (out, src_row, kept) if return_plan else out

    def masked(self, mask_probability=0.9, seed=0):
        """-> MaskedCorpus(self, mask_probability, seed): the n_docs documents with negative sentences dropped, drawn anew every epoch"""
        return MaskedCorpus(self, mask_probability, seed=seed)

    # ---- PCA projection --------------------------------------------------------------------------------------------------------
    def fit_pca(self, n_components=167, field='embeddings', return_moments=False):
        """-> pca.PcaReducer fitted on ALL rows of this corpus' first (``field='embeddings'``) or second (``'embeddings2'``) input (the
        reference's ``--pca_reduce``: sklearn's PCA(n_components) on the training split, EncoderDataset.py:49-70; it projects the first
        input only).  On the device: ``ops.pca_colsum`` -> centre = fp32(colsum / N) -> ``ops.pca_gram``; on the host
        ``pca.pca_from_moments``, once, from the 8 D^2 bytes read back.  ``return_moments=True``: -> (reducer, {'n', 'colsum', 'center',
        'gram'} as NumPy).  The same corpus gives the same reducer bit for bit, on every rank.
        ValueError: an n_components that is no integer or lies outside 1 .. min(N, D), N < 2, an unknown field, 'embeddings2' without
        a second input; RuntimeError on a CPU-device corpus (there is no CPU fallback)."""
        from .pca import check_n_components, pca_from_moments
        if field not in ('embeddings', 'embeddings2'):
            raise ValueError(f"fit_pca: field is 'embeddings' or 'embeddings2', not {field!r}")
        x = self.corpus if field == 'embeddings' else self.corpus2
        if x is None:
            raise ValueError("fit_pca: field='embeddings2' needs a corpus with a second input")
        n, D = int(x.shape[0]), int(x.shape[1])
        k = check_n_components(n_components, n, D, 'fit_pca')
        if self.device.type != 'cuda':
            raise RuntimeError('ResidentCorpus.fit_pca computes the moments on the GPU (there is no CPU fallback)')
        from . import ops
        with torch.cuda.device(self.device):
            colsum = ops.pca_colsum(x).cpu().numpy()
            center = (colsum / n).astype(np.float32)
            gram = ops.pca_gram(x, torch.from_numpy(center).to(self.device)).cpu().numpy()
        reducer = pca_from_moments(n, colsum, center, gram, k)
        return (reducer, {'n': n, 'colsum': colsum, 'center': center, 'gram': gram}) if return_moments else reducer

    def projected(self, reducer, reducer2=None):
        """-> a ResidentCorpus whose ``corpus`` is ``reducer.transform(self.corpus)``: [total_rows, k] in the wire dtype (bf16: rounded
        once); ``corpus2`` likewise under ``reducer2``, else as it is.  Targets, the row table, the host tables, segments and domains
        are SHARED with this corpus; the index ring is fresh.  Every batch method reads the width from the matrix.
        ValueError when a reducer was fitted on another width, or reducer2 is given without a second input."""
        import copy
        if reducer.n_features_in_ != int(self.corpus.shape[1]):
            raise ValueError(f'projected: the reducer was fitted on width {reducer.n_features_in_}, the corpus has {int(self.corpus.shape[1])}')
        if reducer2 is not None:
            if self.corpus2 is None:
                raise ValueError('projected: reducer2 needs a corpus with a second input')
            if reducer2.n_features_in_ != int(self.corpus2.shape[1]):
                raise ValueError(f'projected: reducer2 was fitted on width {reducer2.n_features_in_}, the second input has {int(self.corpus2.shape[1])}')
        out = copy.copy(self)
        out._ring, out._turn = None, 0
        out.corpus = reducer.transform(self.corpus)
        if reducer2 is not None:
            out.corpus2 = reducer2.transform(self.corpus2)
        return out

    # ---- sentence pooling of frame-level features ----------------------------------------------------------------------------
    def with_frames(self, frames, mode, field='embeddings'):
        """-> a ResidentCorpus that takes one input from ``frames`` (a ``frames.ResidentFrames``) pooled in ``mode`` (one of
        ``frames.POOL_MODES``; the reference's _mean, _max, _mean_std, _max_std, _last, _delta_gap, extract_embeddings.py:644-667) by
        ``frames.pool`` (csrc/frame_pool.hip), in this corpus' wire dtype:
          * ``field='embeddings'``: the pooled matrix replaces the first input;
          * ``field='embeddings2'``: it is the second input (a text-only corpus becomes a late-fusion corpus);
          * ``field='append'``: early fusion -- a new [total_rows, D0 + W] first input whose left block is the stored one and whose right
            block the kernel writes in place (its ld_out is the new width): no concatenated temporary.
        Like ``projected``: targets, the row table, the host tables, segments and domains are SHARED with this corpus, the index ring is
        fresh, and every batch method reads the width from the matrix.
        ValueError: an unknown mode or field, frames on another device, documents or sentences per document that are not this corpus';
        RuntimeError on a CPU-device corpus (there is no CPU fallback)."""
        import copy
        from .frames import pooled_width
        W = pooled_width(mode, frames.D)
        if field not in ('embeddings', 'embeddings2', 'append'):
            raise ValueError(f"with_frames: field is 'embeddings', 'embeddings2' or 'append', not {field!r}")
        if frames.n_docs != self.n_docs:
            raise ValueError(f'with_frames: the frames hold {frames.n_docs} documents, the corpus {self.n_docs}')
        bad = np.flatnonzero(frames.sentences != self.rows)
        if bad.size:
            d = int(bad[0])
            raise ValueError(f'with_frames: document {d} has {int(self.rows[d])} sentences in the corpus but {int(frames.sentences[d])} in the frames')
        if frames.device != self.device:
            raise ValueError(f'with_frames: the frames are on {frames.device}, the corpus on {self.device}')
        if self.device.type != 'cuda':
            raise RuntimeError('ResidentCorpus.with_frames pools on the GPU (there is no CPU fallback)')
        out = copy.copy(self)
        out._ring, out._turn = None, 0
        with torch.cuda.device(self.device):
            if field == 'append':
                D0 = int(self.corpus.shape[1])
                wide = torch.empty((self.total_rows, D0 + W), dtype=self.wire, device=self.device)
                wide[:, :D0].copy_(self.corpus)
                frames.pool(mode, out=wide[:, D0:])
                out.corpus = wide
            elif field == 'embeddings':
                out.corpus = frames.pool(mode, out_dtype=self.wire)
            else:
                out.corpus2 = frames.pool(mode, out_dtype=self.wire)
        return out

    def with_prosodic(self, audio, field='embeddings'):
        """-> a ResidentCorpus that takes one input from ``audio.prosodic()`` (an ``audio.ResidentAudio``; the reference's 167-wide
        ``prosodic`` sentence vector, csrc/prosody.hip) in this corpus' wire dtype; ``field`` and what is shared as in ``with_frames``
        ('append' writes the 167 columns in place behind the stored ones).  ValueError: an unknown field, audio on another device,
        documents or sentences per document that are not this corpus'; RuntimeError on a CPU-device corpus."""
        import copy
        if field not in ('embeddings', 'embeddings2', 'append'):
            raise ValueError(f"with_prosodic: field is 'embeddings', 'embeddings2' or 'append', not {field!r}")
        if audio.n_docs != self.n_docs:
            raise ValueError(f'with_prosodic: the audio holds {audio.n_docs} documents, the corpus {self.n_docs}')
        bad = np.flatnonzero(audio.sentences != self.rows)
        if bad.size:
            d = int(bad[0])
            raise ValueError(f'with_prosodic: document {d} has {int(self.rows[d])} sentences in the corpus but {int(audio.sentences[d])} in the audio')
        if audio.device != self.device:
            raise ValueError(f'with_prosodic: the audio is on {audio.device}, the corpus on {self.device}')
        if self.device.type != 'cuda':
            raise RuntimeError('ResidentCorpus.with_prosodic runs on the GPU (there is no CPU fallback)')
        out = copy.copy(self)
        out._ring, out._turn = None, 0
        with torch.cuda.device(self.device):
            if field == 'append':
                D0 = int(self.corpus.shape[1])
                wide = torch.empty((self.total_rows, D0 + audio.PROSODIC_WIDTH), dtype=self.wire, device=self.device)
                wide[:, :D0].copy_(self.corpus)
                audio.prosodic(out=wide[:, D0:])
                out.corpus = wide
            elif field == 'embeddings':
                out.corpus = audio.prosodic(out_dtype=self.wire)
            else:
                out.corpus2 = audio.prosodic(out_dtype=self.wire)
        return out


class AugmentedCorpus:
    """A view of a ResidentCorpus with ``2 * n_docs`` virtual documents: index v < n_docs is stored document v, bit for bit what
    ``corpus.batch`` gives; index v >= n_docs is the TWIN of document v - n_docs, the same sentences with their topic segments in another
    order, made in the gather (``ResidentCorpus.batch_segments``).  Nothing is copied: the resident bytes stay what they were.

      * ``mode='reverse'``: the reference's inverse_augmentation (utils/load_datasets_precomputed.py:71-96) -- the closed segments in
        descending order, the tail (the rows behind the last boundary) left out, the last label 1.  Fixed per document.
      * ``mode='shuffle'``: ``np.random.default_rng([seed, epoch, d]).permutation(n_segments[d])`` over ALL segments, the tail included,
        the last label 0: the length stays, and so does the loader's rule that a document ends on a 0.  The same on every rank without
        a collective and different every epoch (``set_epoch``; the view's sampler sets it).

    Two deviations from the reference, on purpose: (1) a document without a closed segment (no label 1) has an EMPTY reversed twin
    upstream; here its 'reverse' twin is the unaugmented document (order [0], last label 0), because no kernel of the training step has
    been shown to take a zero-length document.  (2) The upstream loop stops after the first 11 list entries and runs on into the twins
    it has just appended; here every document has exactly one twin.

    ``lengths`` (what a batch reports, known without drawing an order), ``host_fields`` (no GPU), ``batch`` and ``sampler`` mirror the
    corpus'; ``'id'`` holds the virtual indices, ``'domain'`` the stored document's."""

    def __init__(self, corpus, mode, seed=0):
        if mode not in ('reverse', 'shuffle'):
            raise ValueError("AugmentedCorpus: mode must be 'reverse' or 'shuffle'")
        if not corpus._binary_labels:
            raise ValueError('AugmentedCorpus: the corpus holds targets that are not 0 / 1 (a segment ends behind a 1)')
        self.corpus, self.mode, self.seed, self.epoch = corpus, mode, int(seed), 0
        self.n_docs = corpus.n_docs
        self._closed = corpus.n_segments - corpus._has_tail                         # closed segments per document
        if mode == 'reverse':
            twin_rows = np.array([b[c] if c else b[-1] for b, c in zip(corpus._seg_bounds, self._closed)], dtype=np.int64)
        else:
            twin_rows = corpus.rows
        self.rows = np.concatenate([corpus.rows, twin_rows])
        self.lengths = np.minimum(self.rows, corpus.tv) if corpus.truncate else self.rows.copy()

    def __len__(self):
        return 2 * self.n_docs

    def set_epoch(self, epoch):
        """the epoch of the 'shuffle' draws"""
        self.epoch = int(epoch)

    def order(self, v):
        """-> (segment order, close_last) of virtual document v"""
        d = v % self.n_docs
        K, closed = int(self.corpus.n_segments[d]), int(self._closed[d])
        if v < self.n_docs:
            return np.arange(K), closed == K                  # the stored document: every segment in place, its own last label
        if self.mode == 'shuffle':
            return np.random.default_rng([self.seed, self.epoch, d]).permutation(K), False
        if closed == 0:
            return np.zeros(1, dtype=np.int64), False         # deviation (1)
        return np.arange(closed - 1, -1, -1), True

    def _virtual(self, indices):
        vv = np.asarray(indices, dtype=np.int64).reshape(-1)
        if vv.size and (int(vv.min()) < 0 or int(vv.max()) >= 2 * self.n_docs):
            raise IndexError(f'AugmentedCorpus: document index outside 0 .. {2 * self.n_docs - 1}')
        return vv

    def _orders(self, vv):
        pairs = [self.order(v) for v in vv.tolist()]
        return [o for o, _ in pairs], [c for _, c in pairs]

    def host_fields(self, indices, pad_to=None):
        """the host half of ``batch()``: ({'id', 'src_lengths', 'domain'(, 'src_segments')}, padded length); touches no GPU"""
        vv = self._virtual(indices)
        if vv.size == 0:
            return {}, 0
        if int(vv.max()) < self.n_docs:
            return self.corpus.host_fields(vv, pad_to)
        ii = vv % self.n_docs
        out, Lmax = self.corpus._segment_host_fields(ii, self.corpus._segment_tables(ii, *self._orders(vv)), pad_to)
        out['id'] = torch.from_numpy(vv.copy())
        return out, Lmax

    def batch(self, indices, pad_to=None):
        """the batch dict of virtual documents ``indices``: ``corpus.batch`` when all of them are stored documents, one
        ``corpus.batch_segments`` call otherwise (a stored document in it goes through with its segments in place)"""
        vv = self._virtual(indices)
        if vv.size == 0:
            return {}
        if int(vv.max()) < self.n_docs:
            return self.corpus.batch(vv, pad_to)
        out = self.corpus.batch_segments(vv % self.n_docs, *self._orders(vv), pad_to=pad_to)
        out['id'] = torch.from_numpy(vv.copy())
        return out

    def sampler(self, batch_size, **kw):
        """a DocumentShardSampler over the virtual documents whose ``set_epoch`` also sets the epoch of this view's 'shuffle' draws"""
        return _AugmentedSampler(self, 2 * self.n_docs if self.corpus.truncate else self.lengths, batch_size, **kw)


class MaskedCorpus:
    """A view of a ResidentCorpus whose ``n_docs`` documents have a random share of their NEGATIVE sentences dropped (negative-sentence
    masking; reference: ``--mask_inner_sentences`` / ``--mask_probability``, utils/load_datasets_precomputed.py:174-185), made by the plan
    kernel and the gather (``ResidentCorpus.batch_masked``) and drawn anew every epoch.  Nothing is copied and nothing is uploaded again.

    ``mask_probability`` is the probability that a negative sentence is KEPT -- the reference's code (`rand() > mask_probability and not
    label` drops) and ``datasets.load_dataset_from_precomputed``'s reading of it, not the reference's help text: 1.0 keeps everything, 0.0
    keeps the boundaries alone.  Document d's draw in an epoch hangs on ``mask_doc_seeds(seed, epoch, n_docs)[d]`` only: every rank and
    the host regenerate it without a collective.  A document none of whose rows is kept keeps row 0 (the reference would make an empty one).

    ``set_epoch(e)`` makes the epoch's host plan once -- one vectorised pass of the device's hash over the corpus' host labels, O(sentences)
    per EPOCH -- and keeps it until the epoch changes: ``rows`` / ``lengths`` (what a batch reports; cut at truncate_value by a
    truncate=True corpus), the ``src_segments`` and the ``pad_to`` of the view's sampler come from it, so a step does nothing
    O(sentences) on the host and reads nothing back from the device.  ``host_fields`` (no GPU), ``batch``, ``sampler``, ``__len__`` and
    ``lengths`` mirror the corpus'; ``'id'`` and ``'domain'`` are the stored document's."""

    def __init__(self, corpus, mask_probability=0.9, seed=0):
        self.mask_probability = _keep_probability(mask_probability, 'MaskedCorpus')
        self.corpus, self.seed, self.epoch = corpus, int(seed), None
        self.n_docs = corpus.n_docs
        self.set_epoch(0)

    def __len__(self):
        return self.n_docs

    def set_epoch(self, epoch):
        """the epoch of the draws; the host plan is made here, once per epoch"""
        epoch = int(epoch)
        if epoch == self.epoch:
            return
        c = self.corpus
        self.doc_seeds = mask_doc_seeds(self.seed, epoch, self.n_docs)
        self.rows, self._kept_rel, self._kept_ptr, kept_labels = c._mask_plan_host(np.arange(self.n_docs, dtype=np.int64), self.doc_seeds,
                                                                                   self.mask_probability)
        self.lengths = np.minimum(self.rows, c.tv) if c.truncate else self.rows.copy()
        self._segment_ends = c._masked_segment_ends(self.rows, self._kept_ptr, kept_labels) if c.segments else None
        self.epoch = epoch

    def kept_rows(self, d):
        """the host plan of document d in this epoch: the indices of its kept rows, ascending (what the device's src_row lists)"""
        return self._kept_rel[int(self._kept_ptr[d]):int(self._kept_ptr[d + 1])].copy()

    def _plan_of(self, ii):
        return self.rows[ii], [self._segment_ends[i] for i in ii.tolist()] if self._segment_ends is not None else None

    def host_fields(self, indices, pad_to=None):
        """the host half of ``batch()``: ({'id', 'src_lengths', 'domain'(, 'src_segments')}, padded length); touches no GPU"""
        ii = self.corpus._indices(indices)
        if ii.size == 0:
            return {}, 0
        return self.corpus._masked_host_fields(ii, *self._plan_of(ii), pad_to)

    def batch(self, indices, pad_to=None):
        """the batch dict of the masked documents ``indices`` in this epoch: one ``corpus.batch_masked`` call with the plan's lengths"""
        ii = self.corpus._indices(indices)
        if ii.size == 0:
            return {}
        counts, ends = self._plan_of(ii)
        return self.corpus.batch_masked(ii, self.doc_seeds[ii], self.mask_probability, pad_to=pad_to, lengths=counts, segment_ends=ends)

    def sampler(self, batch_size, **kw):
        """a DocumentShardSampler over the masked documents whose ``set_epoch`` also moves this view to the epoch and takes ``pad_to``
        from the epoch's masked lengths: every rank pads a global batch to the same length without a collective"""
        return _MaskedSampler(self, batch_size, **kw)


class DocumentShardSampler:
    """Rank-local batch sampler for data-parallel training from a ResidentCorpus.

    ``lengths``: sentences per document (ResidentCorpus.lengths), or just the number of documents -- ``pad_to`` is then None, what a
    truncate=True corpus wants.  ``batch_size`` is the GLOBAL batch size.  Iterating yields ``(local_indices, pad_to)`` per global
    batch: ``global_batch[rank::world]`` and the longest document of the whole global batch.  Every rank with the same seed and epoch
    (``set_epoch``) draws the same permutation, so ``len()`` and ``pad_to`` agree on every rank without a collective.  The last, smaller
    global batch is kept unless ``drop_last``; a global batch with fewer documents than ``world`` is dropped on EVERY rank (a rank
    without documents cannot take part in the step's collectives): ``dropped_documents`` counts those.  world == 1: a plain batch
    sampler, pad_to = the batch's own maximum."""

    def __init__(self, lengths, batch_size, rank=0, world=1, shuffle=True, seed=0, drop_last=False):
        if isinstance(lengths, (int, np.integer)):
            self.n, self.lengths = int(lengths), None
        else:
            self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
            self.n = int(self.lengths.size)
        self.batch_size, self.rank, self.world = int(batch_size), int(rank), int(world)
        if self.batch_size < 1 or self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError('DocumentShardSampler: need batch_size >= 1, world >= 1 and 0 <= rank < world')
        self.shuffle, self.seed, self.drop_last, self.epoch = bool(shuffle), int(seed), bool(drop_last), 0
        full, rest = divmod(self.n, self.batch_size)
        self._n_batches, self.dropped_documents = full, 0
        if full and self.batch_size < self.world:                  # every global batch is too small to give each rank a document
            self._n_batches, self.dropped_documents = 0, full * self.batch_size
        if rest and not self.drop_last:
            if rest >= self.world:
                self._n_batches += 1
            else:
                self.dropped_documents += rest

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self._n_batches

    def permutation(self):
        """the epoch's document order: the same on every rank"""
        if not self.shuffle:
            return np.arange(self.n, dtype=np.int64)
        return np.random.default_rng([self.seed, self.epoch]).permutation(self.n).astype(np.int64)

    def global_batches(self):
        perm = self.permutation()
        for k in range(0, self.n, self.batch_size):
            g = perm[k:k + self.batch_size]
            if g.size < self.world or (self.drop_last and g.size < self.batch_size):
                continue
            yield g

    def __iter__(self):
        for g in self.global_batches():
            pad_to = int(self.lengths[g].max()) if self.lengths is not None else None
            yield g[self.rank::self.world].tolist(), pad_to


class _AugmentedSampler(DocumentShardSampler):
    """AugmentedCorpus.sampler: DocumentShardSampler over the virtual documents; the epoch also reaches the view's 'shuffle' draws"""

    def __init__(self, view, lengths, batch_size, **kw):
        super().__init__(lengths, batch_size, **kw)
        self.view = view
        view.set_epoch(self.epoch)

    def set_epoch(self, epoch):
        super().set_epoch(epoch)
        self.view.set_epoch(epoch)


class _MaskedSampler(DocumentShardSampler):
    """MaskedCorpus.sampler: the epoch also reaches the view, and ``pad_to`` follows the epoch's masked lengths"""

    def __init__(self, view, batch_size, **kw):
        super().__init__(view.n_docs if view.corpus.truncate else view.lengths, batch_size, **kw)
        self.view = view
        self.set_epoch(self.epoch)

    def set_epoch(self, epoch):
        super().set_epoch(epoch)
        self.view.set_epoch(epoch)
        if self.lengths is not None:
            self.lengths = self.view.lengths
