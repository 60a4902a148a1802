"""Sentence pooling of frame-level audio features on the device.

The reference's extractor keeps, per document, the frame-level encoder output of every sentence (``_no_reduction/<file>.pkl``) and writes
six pooled variants of it (extract_embeddings.py:644-667): ``_mean``, ``_max``, ``_mean_std``, ``_max_std``, ``_last`` and
``_delta_gap``; its run scripts train on one of them, so the variant is an axis of its experiments.  Here the frames are uploaded ONCE and
pooled in HBM by csrc/frame_pool.hip (``ops.frame_pool``: the reductions, ``ops.frame_edges``: the two gathers), in any of the six modes:

  * ``load_frames(directory, files)`` reads the extractor's pickles;
  * ``ResidentFrames(docs, device, wire_dtype)`` holds the flat [total_frames, D] matrix and the sentence table on the device;
  * ``frames.pool(mode)`` is the [total_sentences, W] matrix of one variant (W = 2 D for the two ``_std`` modes, else D);
  * ``ResidentCorpus.with_frames(frames, mode, field)`` (resident.py) hands it to the corpus as its first input, as its second input, or
    early-fused behind the text columns, so that ``fit``, ``evaluate``, ``cross_validate``, ``fit_pca``, ``augmented`` and ``masked``
    take it unchanged.

What each mode is, per sentence of n frames e[0] .. e[n - 1] and per column: 'mean' the arithmetic mean; 'max' the largest value; 'mean_std'
/ 'max_std' that followed by the population standard deviation (the root of the mean squared deviation about the mean); 'last' e[n - 1];
'delta_gap' the first frame of the document's next sentence minus e[n - 1], and e[n - 1] itself for a document's last sentence.  The
arithmetic (fp32, the order of the sums) is stated in include/mts.h.  Two deviations from the reference, on purpose: a non-finite value is
refused at upload (NumPy would carry a NaN through ``max``), and the sums run in the kernels' fixed order, not in NumPy's pairwise one.
"""
import os
import pickle

import numpy as np
import torch

POOL_MODES = ('mean', 'max', 'mean_std', 'max_std', 'last', 'delta_gap')
_WIRE = {'fp32': torch.float32, 'bf16': torch.bfloat16}
_CHECK_ROWS = 1 << 16                      # frames per slice of the upload's finiteness check


def pooled_width(mode, D):
    """columns of ``pool(mode)`` for frames of width D"""
    if mode not in POOL_MODES:
        raise ValueError(f'pooling mode is one of {POOL_MODES}, not {mode!r}')
    return 2 * int(D) if mode.endswith('_std') else int(D)


def load_frames(directory, files):
    """-> a list over documents of a list over sentences of [n_frames, D] arrays, read from ``<directory>/<file>.pkl`` as the reference's
    extractor writes them: a pickled object array, or a list, of per-sentence matrices.  A 1-d entry is ONE frame and becomes (1, D), as
    upstream reshapes it (extract_embeddings.py:591-604).  Pickles run code when they are loaded: read only files you wrote."""
    docs = []
    for name in files:
        with open(os.path.join(directory, f'{name}.pkl'), 'rb') as f:
            obj = pickle.load(f)
        sentences = []
        for e in obj:
            a = np.asarray(e)
            sentences.append(a.reshape(1, -1) if a.ndim == 1 else a)
        docs.append(sentences)
    return docs


class ResidentFrames:
    """The frame-level features of a corpus in HBM: ``frames`` [total_frames, D] (fp32 or bf16, ONE upload), ``frame_start`` (int64
    [total_sentences + 1]: sentence s is frames frame_start[s] .. frame_start[s + 1]) and ``doc_last`` (uint8 [total_sentences]: 1 on the
    last sentence of a document).  Host tables: ``sentences`` (sentences per document), ``frame_counts`` (frames per sentence),
    ``n_docs``, ``total_sentences``, ``total_frames``, ``D``.  With a CPU device only the host tables exist, as for ResidentCorpus.

    ValueError, naming the document and the sentence: a sentence without frames (upstream's ``np.max`` raises there), an entry that is no
    [n, D] matrix, widths that differ.  ValueError for a non-finite value, found by one pass on the device at upload."""

    def __init__(self, docs, device, wire_dtype='fp32'):
        if wire_dtype not in _WIRE:
            raise ValueError("wire_dtype must be 'fp32' or 'bf16'")
        self.wire = _WIRE[wire_dtype]
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if len(docs) == 0:
            raise ValueError('ResidentFrames: no documents')
        parts, counts, sentences, D = [], [], [], None
        for d, doc in enumerate(docs):
            if len(doc) == 0:
                raise ValueError(f'ResidentFrames: document {d} has no sentences')
            sentences.append(len(doc))
            for s, e in enumerate(doc):
                a = e.detach().cpu().to(torch.float32).numpy() if isinstance(e, torch.Tensor) else np.asarray(e, dtype=np.float32)
                if a.ndim != 2:
                    raise ValueError(f'ResidentFrames: sentence {s} of document {d} is {a.ndim}-d; [frames, D] matrices are expected')
                if a.shape[0] == 0:
                    raise ValueError(f'ResidentFrames: sentence {s} of document {d} has no frames')
                if D is None:
                    D = int(a.shape[1])
                if int(a.shape[1]) != D or D < 1:
                    raise ValueError(f'ResidentFrames: sentence {s} of document {d} has width {int(a.shape[1])}, the sentences before it {D}')
                parts.append(a)
                counts.append(int(a.shape[0]))
        self.D = D
        self.n_docs = len(sentences)
        self.sentences = np.asarray(sentences, dtype=np.int64)
        self.frame_counts = np.asarray(counts, dtype=np.int64)
        self.total_sentences = int(self.sentences.sum())
        start = np.zeros(self.total_sentences + 1, dtype=np.int64)
        np.cumsum(self.frame_counts, out=start[1:])
        self.total_frames = int(start[-1])
        self._start_host = start
        last = np.zeros(self.total_sentences, dtype=np.uint8)
        last[np.cumsum(self.sentences) - 1] = 1
        self._last_host = last
        self.frames = self.frame_start = self.doc_last = None
        if self.device.type != 'cuda':
            return
        flat = torch.from_numpy(np.concatenate(parts)) if len(parts) > 1 else torch.from_numpy(np.ascontiguousarray(parts[0]))
        del parts
        self.frames = flat.to(self.wire).contiguous().to(self.device)        # fp32 first; bf16 is that matrix' .to(torch.bfloat16)
        self.frame_start = torch.from_numpy(start).to(self.device)
        self.doc_last = torch.from_numpy(last).to(self.device)
        self._refuse_non_finite()

    @classmethod
    def from_device(cls, frames, frame_start, sentences):
        """-> ResidentFrames that ADOPTS device tensors another stage made (``audio.ResidentAudio.mfcc``): ``frames`` a contiguous fp32 /
        bf16 [total_frames, D] device matrix, ``frame_start`` the int64 [total_sentences + 1] table (device or host; ascending from 0 to
        total_frames) and ``sentences`` the sentences per document.  Nothing is copied but the small table; the host tables and
        ``doc_last`` are built from it and the finiteness check of the constructor runs.  ValueError: a matrix of another dtype, layout
        or place, a table that does not fit it, a document without sentences, a sentence without frames."""
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dim() == 2 and frames.is_contiguous()
                and frames.dtype in _WIRE.values() and frames.shape[1] >= 1):
            raise ValueError('ResidentFrames.from_device: frames must be a contiguous fp32 / bf16 [total_frames, D] device matrix')
        sentences = np.asarray(sentences, dtype=np.int64).reshape(-1)
        if sentences.size == 0 or (sentences < 1).any():
            raise ValueError('ResidentFrames.from_device: every document needs at least one sentence')
        start = (frame_start.detach().cpu().numpy() if isinstance(frame_start, torch.Tensor) else np.asarray(frame_start)).astype(np.int64)
        if start.ndim != 1 or start.size != int(sentences.sum()) + 1 or start[0] != 0 or int(start[-1]) != int(frames.shape[0]):
            raise ValueError(f'ResidentFrames.from_device: frame_start must run from 0 to {int(frames.shape[0])} over '
                             f'{int(sentences.sum())} sentences')
        counts = np.diff(start)
        if (counts < 1).any():
            raise ValueError(f'ResidentFrames.from_device: sentence {int(np.flatnonzero(counts < 1)[0])} of the table has no frames')
        self = cls.__new__(cls)
        self.wire, self.device, self.D = frames.dtype, frames.device, int(frames.shape[1])
        self.n_docs, self.sentences, self.frame_counts = int(sentences.size), sentences, counts
        self.total_sentences, self.total_frames = int(sentences.sum()), int(start[-1])
        self._start_host = start
        last = np.zeros(self.total_sentences, dtype=np.uint8)
        last[np.cumsum(sentences) - 1] = 1
        self._last_host = last
        self.frames = frames
        on_device = isinstance(frame_start, torch.Tensor) and frame_start.device == frames.device and frame_start.dtype == torch.int64
        self.frame_start = frame_start.contiguous() if on_device else torch.from_numpy(start).to(frames.device)
        self.doc_last = torch.from_numpy(last).to(frames.device)
        self._refuse_non_finite()
        return self

    def _refuse_non_finite(self):
        """one pass over the resident matrix in slices (the check's temporary stays small); the first offender is named"""
        for a in range(0, self.total_frames, _CHECK_ROWS):
            ok = torch.isfinite(self.frames[a:a + _CHECK_ROWS])
            if not bool(ok.all()):
                f = a + int(torch.nonzero(~ok.all(dim=1))[0])
                s = int(np.searchsorted(self._start_host, f, side='right')) - 1
                d = int(np.searchsorted(np.cumsum(self.sentences), s, side='right'))
                first = int(np.cumsum(self.sentences)[d - 1]) if d else 0
                raise ValueError(f'ResidentFrames: frame {f - int(self._start_host[s])} of sentence {s - first} of document {d} holds a value '
                                 'that is not finite (refused here: NumPy would carry a NaN through max)')

    def __len__(self):
        return self.n_docs

    @property
    def nbytes(self):
        """bytes of the resident data (frames, sentence table, flags); 0 on a CPU device"""
        return sum(t.numel() * t.element_size() for t in (self.frames, self.frame_start, self.doc_last) if t is not None)

    def width(self, mode):
        """columns of ``pool(mode)``"""
        return pooled_width(mode, self.D)

    def pool(self, mode, out=None, out_dtype=None):
        """-> [total_sentences, W] on the device: the sentences pooled in ``mode`` (one of POOL_MODES; W = 2 D for 'mean_std' and
        'max_std', else D), one launch on the current stream.  ``out``: a [total_sentences, W] fp32 / bf16 device tensor with unit column
        stride and any row stride -- a column block of a wider matrix, whose other columns are not touched -- else a new tensor of
        ``out_dtype`` (torch.float32 | torch.bfloat16; default: the frames' own).  A bf16 result is the fp32 one rounded once.
        ValueError: an unknown mode, an ``out`` of another shape; RuntimeError on a CPU device (there is no CPU fallback)."""
        W = self.width(mode)
        if self.device.type != 'cuda':
            raise RuntimeError('ResidentFrames.pool reduces on the GPU (there is no CPU fallback)')
        if out is None:
            out = torch.empty((self.total_sentences, W), dtype=self.wire if out_dtype is None else out_dtype, device=self.device)
        elif tuple(out.shape) != (self.total_sentences, W) or (W > 1 and out.stride(1) != 1) or out.device != self.device:
            raise ValueError(f'pool: out must be [{self.total_sentences}, {W}] on {self.device} with unit column stride, not '
                             f'{tuple(out.shape)} with strides {tuple(out.stride())} on {out.device}')
        elif out_dtype is not None and out.dtype != out_dtype:
            raise ValueError(f'pool: out is {out.dtype}, out_dtype {out_dtype}')
        from . import ops
        with torch.cuda.device(self.device):
            if mode in ('last', 'delta_gap'):
                ops.frame_edges(self.frames, self.frame_start, self.doc_last, out, mode)
            else:
                ops.frame_pool(self.frames, self.frame_start, out, first=mode.split('_')[0], with_std=mode.endswith('_std'))
        return out
