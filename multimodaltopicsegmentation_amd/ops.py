"""Tensor-level wrappers over the C ABI (include/mts.h).  torch is used for device memory and streams only:
every function enqueues hand-written HIP kernels on torch's current stream through raw device pointers.
"""
import ctypes
import math

import torch

from . import _lib as L
from ._lib import check, lib, ptr, stream_ptr, dtype_code

_ws_cache = {}

TIMER = None   # set to a KernelTimer() to time individual launches with HIP events on the launch stream (bench.py)


class KernelTimer:
    """Per-launch HIP-event timing (torch.cuda.Event on torch's current stream = the stream the kernels run on)."""

    def __init__(self, only=None):
        """only: optional predicate on the tag -- every event pair costs a few microseconds of stream time, so the timed region
        of bench.py brackets just the launches its roofline line needs."""
        self.records = {}          # tag -> list of (start_event, end_event)
        self.only = only

    def begin(self, tag):
        if self.only is not None and not self.only(tag):
            return None
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.setdefault(tag, []).append((s, e))
        s.record()
        return e

    def summary(self):
        """tag -> (launches, total_ms); call after torch.cuda.synchronize()."""
        return {t: (len(v), sum(s.elapsed_time(e) for s, e in v)) for t, v in self.records.items()}


_pending_end = [None]     # end event of the bracket in progress (one at a time: launches are issued from one host thread)


@ctypes.CFUNCTYPE(None)
def _mid_hook():
    """called by mts_gemm between its GEMM launch and its split-K reduce launch (mts_gemm_set_mid_hook): the bracket ends HERE, so that a
    timed weight-gradient GEMM reports the GEMM kernel alone -- what a rocprofv3 kernel trace lists under that symbol"""
    e = _pending_end[0]
    if e is not None:
        e.record()
        _pending_end[0] = None


_hook_installed = [False]


class _timed:
    def __init__(self, tag):
        self.tag = tag

    def __enter__(self):
        self.e = TIMER.begin(self.tag) if TIMER is not None else None
        if self.e is not None and self.tag[0] == 'gemm':
            if not _hook_installed[0]:
                lib.mts_gemm_set_mid_hook(ctypes.cast(_mid_hook, ctypes.c_void_p))
                _hook_installed[0] = True
            _pending_end[0] = self.e

    def __exit__(self, *a):
        if self.e is not None:
            if self.tag[0] == 'gemm':
                if _pending_end[0] is None:            # the hook recorded it
                    return False
                _pending_end[0] = None
            self.e.record()
        return False


def _scratch(nbytes, device, tag):
    """Grow-only scratch buffers keyed by (device, tag): never reallocated inside a steady-state step."""
    # one buffer per (device, purpose, HIP stream): kernels launched on different streams may run concurrently
    key = (str(device), tag, torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == 'cuda' else 0)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


_side_streams = {}


def side_stream(device, idx=0):
    """One of a SMALL fixed pool of side HIP streams per device, shared by every model of the process.  HIP maps streams onto a
    handful of hardware queues (GPU_MAX_HW_QUEUES, 8 here) in creation order: a process that builds several taggers, each with
    side streams of its own, ends up with two streams that should overlap on one queue (the late-fusion line of bench.py's
    other_configs ran 8.5 ms in such a process against 7.6 alone)."""
    key = (str(torch.device(device)), int(idx))
    s = _side_streams.get(key)
    if s is None:
        s = _side_streams[key] = torch.cuda.Stream(device=device)
    return s


_plan_cache = {}


def gemm(layout, A, B, out, *, M, N, K, lda=None, ldb=None, ldc=None, bias=None, residual=None, aux=None, gelu=False,
         colscale=None, ncols_scaled=0, accumulate=False, relu=False):
    """C[M,N] = op(A) op(B) (+ epilogue).  A/B share a dtype (fp32 or bf16); out is fp32 or that dtype."""
    a_dt = dtype_code(A.dtype)
    assert B.dtype == A.dtype
    c_dt = dtype_code(out.dtype)
    epi = 0
    if bias is not None:
        epi |= L.EPI_BIAS
    if residual is not None:
        epi |= L.EPI_RESIDUAL
    if gelu:
        epi |= L.EPI_GELU
    if relu:
        epi |= L.EPI_RELU
    if colscale is not None:
        epi |= L.EPI_COLSCALE
    if accumulate:
        epi |= L.EPI_ACCUM
    lda = lda if lda is not None else A.stride(0)
    ldb = ldb if ldb is not None else B.stride(0)
    ldc = ldc if ldc is not None else out.stride(0)
    ws, ws_bytes = None, 0
    if layout in (L.TN, L.TT) and c_dt == L.F32 and K >= 2048:
        if a_dt == L.BF16:
            ws_bytes = 8192 + min(16, max(1, K // 1024)) * M * N * 4   # arrival tickets of the in-launch combine + up to 16 split-K partial planes
        elif -(-M // 128) * -(-N // 128) <= 128:                       # the fp32 kernel only splits K when it has at most 128 output tiles
            ws_bytes = min(16, 256 // (-(-M // 128) * -(-N // 128)), max(1, K // 512)) * M * N * 4
        if ws_bytes:
            ws = _scratch(ws_bytes, A.device, 'splitk')
    key = (layout, a_dt, c_dt, M, N, K)
    with _timed(('gemm', *key, _plan_cache.get(key, 0))):
        check(lib.mts_gemm(stream_ptr(), a_dt, c_dt, layout, M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), ldc, ptr(bias),
                           ptr(residual), residual.stride(0) if residual is not None else 0, ptr(aux),
                           aux.stride(0) if aux is not None else 0, epi, float(colscale or 1.0), int(ncols_scaled),
                           ptr(ws), ws_bytes))
    if a_dt == L.BF16 and key not in _plan_cache:       # which kernel the cost model picked (128 | 224 | 256): timer label
        t = ctypes.c_int(0)
        lib.mts_gemm_last_plan(ctypes.byref(t), None)
        _plan_cache[key] = t.value
    return out


def linear_fwd(x, w, b, out, **kw):
    """out[M,N] = x[M,K] w[N,K]^T + b."""
    return gemm(L.NT, x, w, out, M=x.shape[0], N=w.shape[0], K=x.shape[1], bias=b, **kw)


def linear_dgrad(dy, w, out, **kw):
    """out[M,K] = dy[M,N] w[N,K]."""
    return gemm(L.NN, dy, w, out, M=dy.shape[0], N=w.shape[1], K=dy.shape[1], **kw)


def linear_wgrad(dy, x, out, **kw):
    """out[N,K] (fp32) = dy[M,N]^T x[M,K]."""
    return gemm(L.TN, dy, x, out, M=dy.shape[1], N=x.shape[1], K=dy.shape[0], **kw)


def wgrad_pair_supported(dy1, x1):
    """Can the two weight gradients dy1^T x1 and (their twin of the same shape) go out as one launch?  (include/mts.h mts_wgrad_pair)"""
    return dy1.dtype == torch.bfloat16 and dy1.is_cuda and lib.mts_wgrad_pair_workspace(dy1.shape[1], x1.shape[1], dy1.shape[0]) > 0


def wgrad_pair(dy1, x1, out1, dy2, x2, out2_t, accumulate=False):
    """out1[M, N] (fp32) = dy1[K, M]^T x1[K, N]  and  out2_t[N, M] = (dy2[K, M]^T x2[K, N])^T  in ONE launch + two fixed-order reduces."""
    K, M = dy1.shape
    N = x1.shape[1]
    assert dy2.shape == dy1.shape and x2.shape == x1.shape and dy2.stride(0) == dy1.stride(0) and x2.stride(0) == x1.stride(0)
    assert tuple(out1.shape) == (M, N) and out2_t.shape[0] == N and out2_t.shape[1] >= M
    nbytes = lib.mts_wgrad_pair_workspace(M, N, K)
    ws = _scratch(nbytes, dy1.device, 'wgrad_pair')
    with _timed(('wgrad_pair', M, N, K)):
        check(lib.mts_wgrad_pair(stream_ptr(), M, N, K, ptr(dy1), ptr(x1), ptr(out1), out1.stride(0), ptr(dy2), ptr(x2), ptr(out2_t), out2_t.stride(0),
                                 dy1.stride(0), x1.stride(0), 1 if accumulate else 0, ptr(ws), nbytes))


def colsum(x, out, accumulate=False):
    M, N = x.shape
    ws = _scratch(lib.mts_colsum_workspace(N), x.device, 'colsum')
    check(lib.mts_colsum(stream_ptr(), dtype_code(x.dtype), M, N, ptr(x), x.stride(0), ptr(out), int(accumulate), ptr(ws)))
    return out


def cast(src, dst):
    check(lib.mts_cast(stream_ptr(), dtype_code(dst.dtype), ptr(src), ptr(dst), src.numel()))
    return dst


def cast_concat(x1, x2, dst):
    """dst[r] = act-dtype(x1[r] | x2[r]) for two fp32 matrices of equal row count (K-split input of the recurrent taggers)."""
    check(lib.mts_cast_concat(stream_ptr(), dtype_code(dst.dtype), x1.shape[0], x1.shape[1], x2.shape[1], ptr(x1), ptr(x2), ptr(dst)))
    return dst


def gather_pad(corpus, row_start, doc_index, dst, pad_value=0.0):
    """dst [B, Lmax, D] (or [B, Lmax] from a 1-d corpus: the targets) = the padded batch of documents ``doc_index`` (int32 [B], on the
    device) of a device-resident corpus [total_rows, D] whose document d is rows row_start[d] .. row_start[d + 1] (int64 [n_docs + 1],
    on the device): include/mts.h mts_gather_pad.  Every element of dst is written; an index outside the corpus gives an all-pad
    document.  fp32 -> fp32, bf16 -> bf16 or fp32 -> bf16 (round to nearest even)."""
    B, Lmax = int(dst.shape[0]), int(dst.shape[1])
    D = 1 if corpus.dim() == 1 else int(corpus.shape[1])
    assert dst.numel() == B * Lmax * D and dst.is_contiguous() and corpus.is_contiguous()
    assert row_start.dtype == torch.int64 and row_start.is_contiguous() and row_start.numel() >= 2
    assert doc_index.dtype == torch.int32 and doc_index.is_contiguous() and doc_index.numel() == B
    assert corpus.device == dst.device == row_start.device == doc_index.device
    check(lib.mts_gather_pad(stream_ptr(), dtype_code(corpus.dtype), dtype_code(dst.dtype), B, Lmax, D, ptr(corpus), ptr(row_start),
                             row_start.numel() - 1, ptr(doc_index), ptr(dst), float(pad_value)))
    return dst


def gather_segments(corpus, row_start, doc_index, seg_ptr, seg_dst, seg_src, dst_len, dst, pad_value=0.0, close_last=None):
    """gather_pad with the documents' segments in a listed order (include/mts.h mts_gather_segments): destination document b is the row
    ranges j = seg_ptr[b] .. seg_ptr[b + 1] - 1 of stored document doc_index[b], range j landing at destination row seg_dst[j] and read from
    the document's row seg_src[j] onwards, dst_len[b] rows in all; everything else is pad.  All tables int32 on the device.  close_last
    (int32 [B], 1-d fp32 corpus only: the targets) applies the label rule: 1 on the last row of every listed segment, close_last[b] on the
    document's last row.  Every element of dst is written."""
    B, Lmax = int(dst.shape[0]), int(dst.shape[1])
    D = 1 if corpus.dim() == 1 else int(corpus.shape[1])
    assert dst.numel() == B * Lmax * D and dst.is_contiguous() and corpus.is_contiguous()
    assert row_start.dtype == torch.int64 and row_start.is_contiguous() and row_start.numel() >= 2
    tables = [doc_index, seg_ptr, seg_dst, seg_src, dst_len] + ([close_last] if close_last is not None else [])
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.device == dst.device for t in tables)
    assert doc_index.numel() == B and seg_ptr.numel() == B + 1 and dst_len.numel() == B and seg_dst.numel() == seg_src.numel()
    assert close_last is None or close_last.numel() == B
    assert corpus.device == dst.device == row_start.device
    check(lib.mts_gather_segments(stream_ptr(), dtype_code(corpus.dtype), dtype_code(dst.dtype), B, Lmax, D, ptr(corpus), ptr(row_start),
                                  row_start.numel() - 1, ptr(doc_index), ptr(seg_ptr), ptr(seg_dst), ptr(seg_src), seg_dst.numel(),
                                  ptr(dst_len), ptr(close_last), ptr(dst), float(pad_value)))
    return dst


def mask_plan(targets, row_start, doc_index, doc_seed, keep_probability, src_row, kept):
    """the plan of a batch of masked documents (include/mts.h mts_mask_plan): for batch row b, the rows of document doc_index[b] (int32 [B])
    that negative-sentence masking keeps -- a row whose fp32 target is not 0, or whose hash under doc_seed[b] (int64 [B] holding the uint64
    bits) falls below keep_probability * 2^32; row 0 when none does -- are listed in order in src_row[b] (int32 [B, Lmax], -1 behind them)
    and counted in kept[b] (int32 [B], not clipped to Lmax).  Every element of both is written.  -> (src_row, kept)"""
    B, Lmax = int(src_row.shape[0]), int(src_row.shape[1])
    assert targets.dtype == torch.float32 and targets.dim() == 1 and targets.is_contiguous()
    assert row_start.dtype == torch.int64 and row_start.is_contiguous() and row_start.numel() >= 2
    assert doc_index.dtype == torch.int32 and doc_index.is_contiguous() and doc_index.numel() == B
    assert doc_seed.dtype == torch.int64 and doc_seed.is_contiguous() and doc_seed.numel() == B
    assert src_row.dtype == torch.int32 and src_row.is_contiguous() and kept.dtype == torch.int32 and kept.is_contiguous() and kept.numel() == B
    assert targets.device == row_start.device == doc_index.device == doc_seed.device == src_row.device == kept.device
    check(lib.mts_mask_plan(stream_ptr(), B, Lmax, ptr(targets), ptr(row_start), row_start.numel() - 1, ptr(doc_index), ptr(doc_seed),
                            float(keep_probability), ptr(src_row), ptr(kept)))
    return src_row, kept


def gather_rows(corpus, row_start, doc_index, src_row, dst, pad_value=0.0):
    """gather_pad with a row table in front of the source row (include/mts.h mts_gather_rows): dst[b, t] = row src_row[b, t] (int32
    [B, Lmax], on the device) of document doc_index[b]; a negative entry or one outside the document gives a pad row.  Every element of dst
    is written."""
    B, Lmax = int(dst.shape[0]), int(dst.shape[1])
    D = 1 if corpus.dim() == 1 else int(corpus.shape[1])
    assert dst.numel() == B * Lmax * D and dst.is_contiguous() and corpus.is_contiguous()
    assert row_start.dtype == torch.int64 and row_start.is_contiguous() and row_start.numel() >= 2
    assert doc_index.dtype == torch.int32 and doc_index.is_contiguous() and doc_index.numel() == B
    assert src_row.dtype == torch.int32 and src_row.is_contiguous() and tuple(src_row.shape) == (B, Lmax)
    assert corpus.device == dst.device == row_start.device == doc_index.device == src_row.device
    check(lib.mts_gather_rows(stream_ptr(), dtype_code(corpus.dtype), dtype_code(dst.dtype), B, Lmax, D, ptr(corpus), ptr(row_start),
                              row_start.numel() - 1, ptr(doc_index), ptr(src_row), ptr(dst), float(pad_value)))
    return dst


def _pca_matrix(x):
    assert x.dim() == 2 and x.is_contiguous() and x.is_cuda, 'a contiguous [rows, D] device matrix is expected'
    return int(x.shape[0]), int(x.shape[1])


def pca_colsum(x, out=None):
    """column sums of the fp32 / bf16 matrix x [rows, D] in fp64 (include/mts.h mts_pca_colsum) -> out (fp64 [D], every element written)"""
    rows, D = _pca_matrix(x)
    if out is None:
        out = torch.empty(D, dtype=torch.float64, device=x.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == D and out.device == x.device
    check(lib.mts_pca_colsum(stream_ptr(), dtype_code(x.dtype), rows, D, ptr(x), ptr(out)))
    return out


def pca_gram(x, center, out=None):
    """G = sum_r (x_r - center)(x_r - center)^T of the fp32 / bf16 matrix x [rows, D] about the fp32 centre [D] (include/mts.h mts_pca_gram):
    centred in fp32, multiplied on the fp32 matrix cores, summed in fp64 across slices of 1024 rows -> out (fp64 [D, D], every element
    written, exactly symmetric)"""
    rows, D = _pca_matrix(x)
    if out is None:
        out = torch.empty((D, D), dtype=torch.float64, device=x.device)
    assert center.dtype == torch.float32 and center.is_contiguous() and center.numel() == D
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == D * D and out.device == x.device == center.device
    check(lib.mts_pca_gram(stream_ptr(), dtype_code(x.dtype), rows, D, ptr(x), ptr(center), ptr(out)))
    return out


def pca_project(x, center, w, y=None):
    """y[r, j] = sum_d fl32(x[r, d] - center[d]) w[j, d] (include/mts.h mts_pca_project): x fp32 / bf16 [rows, D], center fp32 [D], w fp32
    [k, D] -> y [rows, k] (x's dtype unless given: fp32 -> fp32, bf16 -> bf16, fp32 -> bf16; one rounding; every element written)"""
    rows, D = _pca_matrix(x)
    assert w.dim() == 2 and w.dtype == torch.float32 and w.is_contiguous() and int(w.shape[1]) == D
    k = int(w.shape[0])
    if y is None:
        y = torch.empty((rows, k), dtype=x.dtype, device=x.device)
    assert center.dtype == torch.float32 and center.is_contiguous() and center.numel() == D
    assert y.is_contiguous() and y.numel() == rows * k and y.device == x.device == center.device == w.device
    check(lib.mts_pca_project(stream_ptr(), dtype_code(x.dtype), dtype_code(y.dtype), rows, D, k, ptr(x), ptr(center), ptr(w), ptr(y)))
    return y


def _frame_args(frames, frame_start, out, width):
    """the checks the two frame entry points share -> (n_sent, D, ld_out); ``out`` is [n_sent, width] with unit column stride and any
    row stride >= width (a column block of a wider matrix)"""
    assert frames.dim() == 2 and frames.is_contiguous() and frames.is_cuda, 'a contiguous [total_frames, D] device matrix is expected'
    assert frame_start.dtype == torch.int64 and frame_start.dim() == 1 and frame_start.is_contiguous() and frame_start.numel() >= 2
    n_sent, D = frame_start.numel() - 1, int(frames.shape[1])
    assert out.dim() == 2 and tuple(out.shape) == (n_sent, width * D) and (out.stride(1) == 1 or out.shape[1] == 1)
    ld_out = int(out.stride(0)) if n_sent > 1 else max(int(out.stride(0)), width * D)
    assert ld_out >= width * D
    assert frames.device == frame_start.device == out.device
    return n_sent, D, ld_out


def frame_pool(frames, frame_start, out, first='mean', with_std=False):
    """the pooled statistics of every sentence of a frame matrix (include/mts.h mts_frame_pool): frames fp32 / bf16 [total_frames, D],
    sentence s = rows frame_start[s] .. frame_start[s + 1] (int64 [n_sent + 1], on the device).  ``first`` ('mean' | 'max' | None) goes
    to out[:, :D], the population standard deviation (``with_std``) to the D columns behind it.  out: fp32 / bf16 [n_sent, D or 2 D],
    unit column stride, any row stride (a column block of a wider matrix: the rest of it is not touched).  Every element of out is
    written."""
    code = {None: L.POOL_NONE, 'mean': L.POOL_MEAN, 'max': L.POOL_MAX}[first]
    n_sent, D, ld_out = _frame_args(frames, frame_start, out, (first is not None) + bool(with_std))
    check(lib.mts_frame_pool(stream_ptr(), dtype_code(frames.dtype), dtype_code(out.dtype), n_sent, D, code, int(bool(with_std)), ptr(frames),
                             int(frames.shape[0]), ptr(frame_start), ptr(out), ld_out))
    return out


def frame_edges(frames, frame_start, doc_last, out, mode='last'):
    """the two gathers of sentence pooling (include/mts.h mts_frame_edges): 'last' is every sentence's last frame, 'delta_gap' the next
    sentence's first frame minus it, and the last frame itself where doc_last[s] (uint8 [n_sent], on the device; may be None for 'last')
    marks the last sentence of a document.  out as in frame_pool, [n_sent, D]."""
    code = {'last': L.EDGE_LAST, 'delta_gap': L.EDGE_DELTA_GAP}[mode]
    n_sent, D, ld_out = _frame_args(frames, frame_start, out, 1)
    assert doc_last is not None or mode == 'last'
    if doc_last is not None:
        assert doc_last.dtype == torch.uint8 and doc_last.is_contiguous() and doc_last.numel() == n_sent and doc_last.device == out.device
    check(lib.mts_frame_edges(stream_ptr(), dtype_code(frames.dtype), dtype_code(out.dtype), n_sent, D, code, ptr(frames), int(frames.shape[0]),
                              ptr(frame_start), ptr(doc_last), ptr(out), ld_out))
    return out


def mel_frames(wave, sent_start, sent_len, frame_start, total_frames, window, twiddle, mel_first, mel_ptr, mel_w, hop, mel=None):
    """the mel power spectrogram of every sentence of a resident waveform (include/mts.h mts_mel_frames): wave fp32 [total_samples];
    sentence s is its sent_len[s] samples from sent_start[s] and owns the rows frame_start[s] .. frame_start[s + 1] of mel (all int64, on
    the device).  window fp32 [n_fft], twiddle fp32 [n_fft, 2], the packed mel filters mel_first int32 [n_mels], mel_ptr int32
    [n_mels + 1], mel_w fp32 [nnz].  -> mel fp32 [total_frames, n_mels], every element written."""
    n_sent, n_fft, n_mels = sent_start.numel(), window.numel(), mel_first.numel()
    assert wave.dim() == 1 and wave.dtype == torch.float32 and wave.is_contiguous() and wave.is_cuda
    for t in (sent_start, sent_len, frame_start):
        assert t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous() and t.device == wave.device
    assert sent_len.numel() == n_sent and frame_start.numel() == n_sent + 1
    for t in (window, twiddle, mel_w):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.device == wave.device
    for t in (mel_first, mel_ptr):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and t.device == wave.device
    assert twiddle.numel() == 2 * n_fft and mel_ptr.numel() == n_mels + 1
    total_frames = int(total_frames)
    if mel is None:
        mel = torch.empty((max(total_frames, 0), n_mels), dtype=torch.float32, device=wave.device)
    assert mel.dtype == torch.float32 and mel.is_contiguous() and mel.numel() == max(total_frames, 0) * n_mels and mel.device == wave.device
    check(lib.mts_mel_frames(stream_ptr(), n_sent, n_fft, int(hop), n_mels, ptr(wave), wave.numel(), ptr(sent_start), ptr(sent_len),
                             ptr(frame_start), total_frames, ptr(window), ptr(twiddle), ptr(mel_first), ptr(mel_ptr), ptr(mel_w), mel_w.numel(),
                             ptr(mel)))
    return mel


def mfcc_frames(mel, frame_start, dct, out):
    """MFCC and delta frames from the mel powers (include/mts.h mts_mfcc_frames): mel fp32 [total_frames, n_mels], frame_start int64
    [n_sent + 1], dct fp32 [n_mfcc, n_mels].  out: fp32 / bf16 [total_frames, 2 n_mfcc], unit column stride, any row stride (a column block
    of a wider matrix: the rest of it is not touched); columns [0, n_mfcc) the MFCC, the rest the delta.  Every element of out is
    written."""
    assert mel.dim() == 2 and mel.dtype == torch.float32 and mel.is_contiguous() and mel.is_cuda
    assert frame_start.dtype == torch.int64 and frame_start.dim() == 1 and frame_start.is_contiguous() and frame_start.numel() >= 2
    assert dct.dim() == 2 and dct.dtype == torch.float32 and dct.is_contiguous() and int(dct.shape[1]) == int(mel.shape[1])
    total_frames, n_mels = int(mel.shape[0]), int(mel.shape[1])
    n_sent, n_mfcc = frame_start.numel() - 1, int(dct.shape[0])
    assert out.dim() == 2 and tuple(out.shape) == (total_frames, 2 * n_mfcc) and out.stride(1) == 1
    ld_out = int(out.stride(0)) if total_frames > 1 else max(int(out.stride(0)), 2 * n_mfcc)
    assert mel.device == frame_start.device == dct.device == out.device
    nbytes = int(lib.mts_mfcc_frames_workspace(n_sent, total_frames, n_mfcc))
    work = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=mel.device)
    check(lib.mts_mfcc_frames(stream_ptr(), dtype_code(out.dtype), n_sent, n_mels, n_mfcc, ptr(mel), total_frames, ptr(frame_start), ptr(dct),
                              ptr(work), nbytes, ptr(out), ld_out))
    return out


def _dev_tensor(t, dtype, numel, like):
    assert t.dtype == dtype and t.is_contiguous() and t.numel() == numel and t.device == like.device, (t.dtype, tuple(t.shape), numel)
    return t


def yin_frames(wave, sent_start, sent_len, frame_start, total_frames, min_period, max_period, frame_length=2048, win_length=1024, hop=512):
    """the cumulative-mean-normalised difference function of every frame of a resident waveform and its parabolic shifts (include/mts.h
    mts_yin_frames); the sentence table as in mel_frames.  -> (cmnd, shift), both fp32 [total_frames, max_period - min_period + 1]."""
    n_sent, total_frames, n_lags = sent_start.numel(), int(total_frames), int(max_period) - int(min_period) + 1
    assert wave.dim() == 1 and wave.dtype == torch.float32 and wave.is_contiguous() and wave.is_cuda
    _dev_tensor(sent_start, torch.int64, n_sent, wave), _dev_tensor(sent_len, torch.int64, n_sent, wave)
    _dev_tensor(frame_start, torch.int64, n_sent + 1, wave)
    cmnd = torch.empty((max(total_frames, 0), max(n_lags, 0)), dtype=torch.float32, device=wave.device)
    shift = torch.empty_like(cmnd)
    check(lib.mts_yin_frames(stream_ptr(), n_sent, int(frame_length), int(win_length), int(hop), int(min_period), int(max_period), ptr(wave),
                             wave.numel(), ptr(sent_start), ptr(sent_len), ptr(frame_start), total_frames, ptr(cmnd), ptr(shift)))
    return cmnd, shift


def pyin_observe(cmnd, shift, tabs, voiced_prob=None, logobs=None):
    """pYIN's observation model per frame (include/mts.h mts_pyin_observe): cmnd / shift fp32 [F, n_lags]; ``tabs`` the device tables of
    ``audio.pyin_tables`` (with its scalars).  -> (voiced_prob fp32 [F], logobs fp64 [F, 2 n_bins]), every element written."""
    assert cmnd.dim() == 2 and cmnd.dtype == torch.float32 and cmnd.is_contiguous() and cmnd.is_cuda
    F, n_lags = int(cmnd.shape[0]), int(cmnd.shape[1])
    _dev_tensor(shift, torch.float32, F * n_lags, cmnd)
    n_bins, n_thr, n_boltz = int(tabs['n_bins']), tabs['thresholds'].numel(), tabs['boltz_fact'].numel()
    _dev_tensor(tabs['thresholds'], torch.float64, n_thr, cmnd), _dev_tensor(tabs['beta'], torch.float64, n_thr, cmnd)
    _dev_tensor(tabs['beta_head'], torch.float64, n_thr + 1, cmnd), _dev_tensor(tabs['boltz_exp'], torch.float64, n_boltz, cmnd)
    assert tabs['boltz_fact'].dtype == torch.float64 and tabs['boltz_fact'].device == cmnd.device
    if voiced_prob is None:
        voiced_prob = torch.empty(F, dtype=torch.float32, device=cmnd.device)
    if logobs is None:
        logobs = torch.empty((F, 2 * n_bins), dtype=torch.float64, device=cmnd.device)
    _dev_tensor(voiced_prob, torch.float32, F, cmnd), _dev_tensor(logobs, torch.float64, F * 2 * n_bins, cmnd)
    check(lib.mts_pyin_observe(stream_ptr(), F, n_lags, int(tabs['min_period']), n_bins, float(tabs['sr']), float(tabs['fmin']),
                               float(tabs['bins_per_octave']), ptr(cmnd), ptr(shift), ptr(tabs['thresholds']), ptr(tabs['beta']),
                               ptr(tabs['beta_head']), n_thr, ptr(tabs['boltz_fact']), ptr(tabs['boltz_exp']), n_boltz,
                               float(tabs['no_trough_prob']), float(tabs['log_floor']), ptr(voiced_prob), ptr(logobs)))
    return voiced_prob, logobs


def pyin_viterbi(logobs, frame_start, tabs, f0=None, voiced=None, state=None):
    """the fp64 Viterbi of every sentence over its frames' log-observations (include/mts.h mts_pyin_viterbi): logobs fp64 [F, 2 n_bins],
    frame_start int64 [n_sent + 1].  -> (state int32 [F], f0 fp32 [F], NaN where unvoiced, voiced uint8 [F]).  The int16 backpointers
    [F, 2 n_bins] are a temporary of this call."""
    assert logobs.dim() == 2 and logobs.dtype == torch.float64 and logobs.is_contiguous() and logobs.is_cuda
    F, S = int(logobs.shape[0]), int(logobs.shape[1])
    n_bins, n_sent = int(tabs['n_bins']), frame_start.numel() - 1
    assert S == 2 * n_bins
    _dev_tensor(frame_start, torch.int64, n_sent + 1, logobs)
    _dev_tensor(tabs['lsrc'], torch.float64, 4 * n_bins, logobs), _dev_tensor(tabs['linit'], torch.float64, S, logobs)
    _dev_tensor(tabs['freqs'], torch.float32, n_bins, logobs)
    assert tabs['ltri'].dtype == torch.float64 and tabs['ltri'].is_contiguous() and tabs['ltri'].device == logobs.device
    state = torch.empty(F, dtype=torch.int32, device=logobs.device) if state is None else state
    f0 = torch.empty(F, dtype=torch.float32, device=logobs.device) if f0 is None else f0
    voiced = torch.empty(F, dtype=torch.uint8, device=logobs.device) if voiced is None else voiced
    _dev_tensor(state, torch.int32, F, logobs), _dev_tensor(f0, torch.float32, F, logobs), _dev_tensor(voiced, torch.uint8, F, logobs)
    back = torch.empty((max(F, 1), S), dtype=torch.int16, device=logobs.device)
    check(lib.mts_pyin_viterbi(stream_ptr(), n_sent, n_bins, tabs['ltri'].numel(), ptr(logobs), F, ptr(frame_start), ptr(tabs['ltri']),
                               ptr(tabs['lsrc']), ptr(tabs['linit']), float(tabs['log_floor']), ptr(tabs['freqs']), ptr(back), ptr(state),
                               ptr(f0), ptr(voiced)))
    return state, f0, voiced


def yin_pick(cmnd, shift, min_period, sr, trough_threshold=0.1, f0=None):
    """the plain-YIN f0 of every frame (include/mts.h mts_yin_pick): cmnd / shift fp32 [F, n_lags] -> f0 fp32 [F]"""
    assert cmnd.dim() == 2 and cmnd.dtype == torch.float32 and cmnd.is_contiguous() and cmnd.is_cuda
    F, n_lags = int(cmnd.shape[0]), int(cmnd.shape[1])
    _dev_tensor(shift, torch.float32, F * n_lags, cmnd)
    f0 = torch.empty(F, dtype=torch.float32, device=cmnd.device) if f0 is None else f0
    _dev_tensor(f0, torch.float32, F, cmnd)
    check(lib.mts_yin_pick(stream_ptr(), F, n_lags, int(min_period), float(sr), float(trough_threshold), ptr(cmnd), ptr(shift), ptr(f0)))
    return f0


def frame_delta(x, frame_start):
    """the Savitzky-Golay slope of width 9 along the frames of every sentence (include/mts.h mts_frame_delta; the delta of mfcc_frames):
    x fp32 [F, D], frame_start int64 [n_sent + 1] -> fp32 [F, D]; 0 for a sentence of fewer than 9 frames"""
    assert x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous() and x.is_cuda
    n_sent = frame_start.numel() - 1
    _dev_tensor(frame_start, torch.int64, n_sent + 1, x)
    out = torch.empty_like(x)
    check(lib.mts_frame_delta(stream_ptr(), n_sent, int(x.shape[1]), ptr(x), int(x.shape[0]), ptr(frame_start), ptr(out)))
    return out


def prosodic_stats(f0, voiced_prob, prev_f0, frame_start, doc_first, out, jump_col):
    """the six scalar columns and pitch_jump of the prosodic sentence vector (include/mts.h mts_prosodic_stats): f0 (the pYIN track, NaN
    where unvoiced), voiced_prob, prev_f0 (the plain-YIN track) fp32 [F]; frame_start int64 [n_sent + 1]; doc_first uint8 [n_sent].  out:
    fp32 / bf16 [n_sent, > jump_col], unit column stride; columns 0 .. 5 and jump_col are written, nothing else."""
    assert f0.dim() == 1 and f0.dtype == torch.float32 and f0.is_contiguous() and f0.is_cuda
    F, n_sent = f0.numel(), frame_start.numel() - 1
    _dev_tensor(voiced_prob, torch.float32, F, f0), _dev_tensor(prev_f0, torch.float32, F, f0)
    _dev_tensor(frame_start, torch.int64, n_sent + 1, f0), _dev_tensor(doc_first, torch.uint8, n_sent, f0)
    assert out.dim() == 2 and int(out.shape[0]) == n_sent and int(out.shape[1]) > int(jump_col) and out.stride(1) == 1 and out.device == f0.device
    ld_out = int(out.stride(0)) if n_sent > 1 else max(int(out.stride(0)), int(jump_col) + 1)
    check(lib.mts_prosodic_stats(stream_ptr(), dtype_code(out.dtype), n_sent, ptr(f0), ptr(voiced_prob), ptr(prev_f0), F, ptr(frame_start),
                                 ptr(doc_first), ptr(out), ld_out, int(jump_col)))
    return out


def w2v_wave_stats(wave, sent_start, sent_len, stats=None):
    """(mean, 1 / sqrt(var + 1e-7)) of every sentence's samples (include/mts.h mts_w2v_wave_stats) -> fp32 [n_sent, 2]"""
    assert wave.dim() == 1 and wave.dtype == torch.float32 and wave.is_contiguous() and wave.is_cuda
    n_sent = sent_start.numel()
    _dev_tensor(sent_start, torch.int64, n_sent, wave), _dev_tensor(sent_len, torch.int64, n_sent, wave)
    stats = torch.empty((n_sent, 2), dtype=torch.float32, device=wave.device) if stats is None else stats
    _dev_tensor(stats, torch.float32, 2 * n_sent, wave)
    check(lib.mts_w2v_wave_stats(stream_ptr(), n_sent, ptr(wave), wave.numel(), ptr(sent_start), ptr(sent_len), ptr(stats)))
    return stats


def w2v_conv0_stats(wave, sent_start, sent_len, wave_stats, w, stride, eps=1e-5):
    """the GroupNorm statistics of conv layer 0 on the normalised samples (include/mts.h mts_w2v_conv0_stats): w fp32 [C, kernel]
    -> (gmean, grstd), both fp32 [n_sent, C]; the conv output itself is never stored"""
    n_sent, (C, kernel) = sent_start.numel(), w.shape
    _dev_tensor(wave_stats, torch.float32, 2 * n_sent, wave), _dev_tensor(w, torch.float32, C * kernel, wave)
    gmean = torch.empty((n_sent, C), dtype=torch.float32, device=wave.device)
    grstd = torch.empty_like(gmean)
    check(lib.mts_w2v_conv0_stats(stream_ptr(), n_sent, int(C), int(kernel), int(stride), ptr(wave), wave.numel(), ptr(sent_start), ptr(sent_len),
                                  ptr(wave_stats), ptr(w), float(eps), ptr(gmean), ptr(grstd)))
    return gmean, grstd


def w2v_conv0(wave, sent_start, sent_len, wave_stats, w, stride, gmean, grstd, gamma, beta, block_start, total_rows, out):
    """conv layer 0 + GroupNorm + GELU into the sentences' row blocks (include/mts.h mts_w2v_conv0): block_start int64 [n_sent + 1] in
    multiples of 64; out fp32 / bf16 [>= total_rows, C], contiguous; every row below total_rows is written (0 behind a sentence's frames)"""
    n_sent, (C, kernel) = sent_start.numel(), w.shape
    _dev_tensor(block_start, torch.int64, n_sent + 1, wave)
    _dev_tensor(gmean, torch.float32, n_sent * C, wave), _dev_tensor(grstd, torch.float32, n_sent * C, wave)
    _dev_tensor(gamma, torch.float32, C, wave), _dev_tensor(beta, torch.float32, C, wave)
    assert out.dim() == 2 and out.is_contiguous() and int(out.shape[1]) == C and int(out.shape[0]) >= int(total_rows) and out.device == wave.device
    check(lib.mts_w2v_conv0(stream_ptr(), dtype_code(out.dtype), n_sent, int(C), int(kernel), int(stride), ptr(wave), wave.numel(), ptr(sent_start),
                            ptr(sent_len), ptr(wave_stats), ptr(w), ptr(gmean), ptr(grstd), ptr(gamma), ptr(beta), ptr(block_start), int(total_rows),
                            ptr(out)))
    return out


def w2v_regroup(x, src_row0, pad_start, rows_p, G, Kp, out=None):
    """x [*, H] -> group-major, zero-padded [G, rows_p, H / G] (include/mts.h mts_w2v_regroup); every element of out is written"""
    assert x.dim() == 2 and x.is_contiguous() and x.is_cuda
    n_sent, H = src_row0.numel(), int(x.shape[1])
    _dev_tensor(src_row0, torch.int64, n_sent, x), _dev_tensor(pad_start, torch.int64, n_sent + 1, x)
    if out is None:
        out = torch.empty((int(G), int(rows_p), H // max(int(G), 1)), dtype=x.dtype, device=x.device)
    assert out.is_contiguous() and out.dtype == x.dtype and out.numel() == int(rows_p) * H and out.device == x.device
    check(lib.mts_w2v_regroup(stream_ptr(), dtype_code(x.dtype), n_sent, H, int(G), int(Kp), ptr(x), ptr(src_row0), ptr(pad_start), int(rows_p),
                              ptr(out)))
    return out


def w2v_rows(src, src_row0, dst_start, dst, res=None, res_row0=None):
    """dst[dst_start[s] + t] = src[src_row0[s] + t] (+ res[res_row0[s] + t]) (include/mts.h mts_w2v_rows): compaction, residual and cast"""
    assert src.dim() == 2 and src.is_contiguous() and src.is_cuda and dst.dim() == 2 and dst.is_contiguous() and dst.shape[1] == src.shape[1]
    n_sent, D = src_row0.numel(), int(src.shape[1])
    _dev_tensor(src_row0, torch.int64, n_sent, src), _dev_tensor(dst_start, torch.int64, n_sent + 1, src)
    if res is not None:
        assert res.dim() == 2 and res.is_contiguous() and res.dtype == src.dtype and int(res.shape[1]) == D and res.device == src.device
        _dev_tensor(res_row0, torch.int64, n_sent, src)
    check(lib.mts_w2v_rows(stream_ptr(), dtype_code(src.dtype), dtype_code(dst.dtype), n_sent, D, ptr(src), ptr(src_row0), ptr(res), ptr(res_row0),
                           ptr(dst_start), int(dst.shape[0]), ptr(dst)))
    return dst


def w2v_pos_conv(x, src_row0, dst_start, tile_start, n_tiles, w, bias, G, Kp, y):
    """y[dst_start[s] + t] = x[src_row0[s] + t] + gelu(grouped conv + bias) on the matrix cores (include/mts.h mts_w2v_pos_conv): bf16 x
    [*, H] and y [total_frames, H]; w bf16 [G, H / G, K_p * H / G]; tile_start int32 [n_sent + 1]"""
    assert x.dim() == 2 and x.is_contiguous() and x.is_cuda and x.dtype == torch.bfloat16 == y.dtype == w.dtype
    n_sent, H = src_row0.numel(), int(x.shape[1])
    _dev_tensor(src_row0, torch.int64, n_sent, x), _dev_tensor(dst_start, torch.int64, n_sent + 1, x), _dev_tensor(tile_start, torch.int32, n_sent + 1, x)
    _dev_tensor(w, torch.bfloat16, H * (H // max(int(G), 1)) * int(Kp), x), _dev_tensor(bias, torch.float32, H, x)
    assert y.dim() == 2 and y.is_contiguous() and int(y.shape[1]) == H and y.device == x.device
    with _timed(('w2v_pos_conv', int(n_tiles), H, int(G), int(Kp))):
        check(lib.mts_w2v_pos_conv(stream_ptr(), n_sent, H, int(G), int(Kp), ptr(x), ptr(src_row0), ptr(dst_start), ptr(tile_start), int(n_tiles), ptr(w),
                                   ptr(bias), ptr(y)))
    return y


def text_embed(ids, pos, word, position, type_row, gamma, beta, eps, out):
    """out[i, :H] = LayerNorm(word[ids[i]] + position[pos[i]] + type_row) (include/mts.h mts_text_embed): ids / pos int32 [n_tokens] on the
    device, pos already holding the position table's row; the tables fp32 / bf16 [vocab, H], [n_pos, H], [H]; gamma / beta fp32 [H]; out
    [n_tokens, >= H] in the tables' dtype with unit column stride (columns behind H are not touched).  The kernel trusts the ids: the
    caller has checked them against the tables."""
    n_tokens, (vocab, H), n_pos = ids.numel(), (int(d) for d in word.shape), int(position.shape[0])
    _dev_tensor(ids, torch.int32, n_tokens, word), _dev_tensor(pos, torch.int32, n_tokens, word)
    _dev_tensor(position, word.dtype, n_pos * H, word), _dev_tensor(type_row, word.dtype, H, word)
    _dev_tensor(gamma, torch.float32, H, word), _dev_tensor(beta, torch.float32, H, word)
    assert word.is_cuda and word.is_contiguous() and out.dim() == 2 and out.dtype == word.dtype and out.device == word.device
    assert int(out.shape[0]) == n_tokens and int(out.shape[1]) >= H and out.stride(1) == 1
    with _timed(('text_embed', n_tokens, H)):
        check(lib.mts_text_embed(stream_ptr(), dtype_code(word.dtype), n_tokens, H, ptr(ids), ptr(pos), ptr(word), vocab, ptr(position), n_pos,
                                 ptr(type_row), ptr(gamma), ptr(beta), float(eps), ptr(out), int(out.stride(0))))
    return out


def sent_attn_fwd(qkv, row0, lengths, max_len, D, heads, ctx):
    """Full self-attention over packed short sequences on one wave per (sentence, head) (include/mts.h mts_sent_attn_fwd): qkv bf16
    [rows, 3 D] with q already scaled, sentence s = rows row0[s] .. row0[s] + lengths[s] - 1 (int32 [n_sent] each, on the device), ctx bf16
    [rows, D].  NotImplementedError where the kernel does not cover (fp32, a head dim that is no multiple of 32 or above 128, max_len
    above 64): nothing is written then."""
    n_sent = row0.numel()
    assert qkv.dim() == 2 and qkv.is_cuda and qkv.is_contiguous() and int(qkv.shape[1]) == 3 * D
    assert ctx.dim() == 2 and ctx.is_contiguous() and ctx.dtype == qkv.dtype and ctx.device == qkv.device and tuple(ctx.shape) == (int(qkv.shape[0]), D)
    _dev_tensor(row0, torch.int32, n_sent, qkv), _dev_tensor(lengths, torch.int32, n_sent, qkv)
    with _timed(('sent_attn_fwd', n_sent, int(max_len), D, heads)):
        check(lib.mts_sent_attn_fwd(stream_ptr(), dtype_code(qkv.dtype), n_sent, D, heads, ptr(qkv), ptr(row0), ptr(lengths), int(max_len), ptr(ctx)))
    return ctx


def embed_layernorm_fwd(x, pos, pos_offset, type0, gamma, beta, eps, y, pre, mean, rstd, row_src=None, x2=None):
    """row_src (int32 [n_rows], optional): packed batch -- output row r is sentence row_src[r] = b*L + i of x.
    x2 (fp32 [B, L, D2], optional): K-split input -- the row is x[b, i] | x2[b, i] and the concatenation is never materialised."""
    B, Lq, D = x.shape
    if x.dtype == torch.bfloat16:
        assert x2 is None and y.dtype == torch.bfloat16
        check(lib.mts_embed_layernorm_fwd_x16(stream_ptr(), B, Lq, D, ptr(x), ptr(pos), pos_offset, ptr(type0), ptr(gamma), ptr(beta), eps, ptr(y),
                                              ptr(pre), ptr(mean), ptr(rstd), ptr(row_src), row_src.numel() if row_src is not None else 0))
        return
    if x2 is not None:
        check(lib.mts_embed_layernorm_fwd2(stream_ptr(), dtype_code(y.dtype), B, Lq, D, x2.shape[2], ptr(x), ptr(x2), ptr(pos), pos_offset,
                                           ptr(type0), ptr(gamma), ptr(beta), eps, ptr(y), ptr(pre), ptr(mean), ptr(rstd), ptr(row_src),
                                           row_src.numel() if row_src is not None else 0))
        return
    check(lib.mts_embed_layernorm_fwd(stream_ptr(), dtype_code(y.dtype), B, Lq, D, ptr(x), ptr(pos), pos_offset, ptr(type0),
                                      ptr(gamma), ptr(beta), eps, ptr(y), ptr(pre), ptr(mean), ptr(rstd), ptr(row_src),
                                      row_src.numel() if row_src is not None else 0))


def layernorm_fwd(x, gamma, beta, eps, y, mean, rstd, head_w=None, head_b=None, scores=None):
    """y may be None with a fused head: only the scores and the statistics are produced."""
    rows, D = x.shape
    n_out = head_w.shape[0] if head_w is not None else 0
    check(lib.mts_layernorm_fwd(stream_ptr(), dtype_code(x.dtype), rows, D, ptr(x), ptr(gamma), ptr(beta), eps, ptr(y),
                                ptr(mean), ptr(rstd), ptr(head_w), ptr(head_b), n_out, ptr(scores)))


def layernorm_bwd(x, dy, gamma, mean, rstd, dx, dgamma, dbeta, dxsum=None, dlogit=None, head_w=None, beta=None, dhead_w=None, dhead_b=None):
    """dhead_w / dhead_b (with beta): the fused head's parameter gradients come out of the same pass (n_out <= 2)."""
    rows, D = x.shape
    ws = _scratch(lib.mts_layernorm_bwd_workspace(D), x.device, 'ln_bwd')
    n_out = head_w.shape[0] if head_w is not None else 0
    check(lib.mts_layernorm_bwd(stream_ptr(), dtype_code(x.dtype), rows, D, ptr(x), ptr(dy), ptr(dlogit), ptr(head_w), n_out,
                                ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dgamma), ptr(dbeta), ptr(dxsum), ptr(ws),
                                ptr(beta), ptr(dhead_w), ptr(dhead_b)))


def loss_tail_supported(dtype, D, n_out):
    return dtype in (torch.float32, torch.bfloat16) and bool(lib.mts_layernorm_loss_tail_supported(dtype_code(dtype), D, n_out))


def layernorm_loss_tail(kind, x, gamma, beta, eps, head_w, head_b, targets, lengths, alpha, gamma_f, grad_scale, scores, loss_out, dx, dgamma,
                        dbeta, dxsum, dhead_w, dhead_b, batch_shape, row_src=None):
    """The last layer's LayerNorm + head + loss + their backward in one pass over x = s2 [rows, D] (see include/mts.h)."""
    rows, D = x.shape
    B, Lq = batch_shape
    ws = _scratch(lib.mts_layernorm_bwd_workspace(D), x.device, 'ln_bwd')
    with _timed(('ln_tail', rows, D, head_w.shape[0])):
        check(lib.mts_layernorm_loss_tail(stream_ptr(), dtype_code(x.dtype), rows, D, ptr(x), ptr(gamma), ptr(beta), eps, ptr(head_w), ptr(head_b),
                                          head_w.shape[0], kind, B, Lq, targets.shape[1], ptr(targets), ptr(lengths), float(alpha), float(gamma_f),
                                          float(grad_scale), ptr(row_src), row_src.numel() if row_src is not None else 0, ptr(scores),
                                          ptr(loss_out), ptr(dx), ptr(dgamma), ptr(dbeta), ptr(dxsum), ptr(dhead_w), ptr(dhead_b), ptr(ws)))


def embed_layernorm_bwd(pre, dh, gamma, mean, rstd, B, Lq, dgamma, dbeta, dtype0, dpos, pos_offset, row0=None, lengths=None):
    """Embedding block backward in one pass: dgamma / dbeta / dtype0 and rows pos_offset .. pos_offset + Lq - 1 of dpos are
    overwritten; the pre-LayerNorm gradient is never stored."""
    rows, D = pre.shape
    nb = lib.mts_embed_layernorm_bwd_workspace(B, Lq, D)
    ws = _scratch(nb, pre.device, 'emb_bwd')
    check(lib.mts_embed_layernorm_bwd(stream_ptr(), dtype_code(pre.dtype), B, Lq, D, ptr(pre), ptr(dh), ptr(gamma), ptr(mean), ptr(rstd),
                                      ptr(dgamma), ptr(dbeta), ptr(dtype0), ptr(dpos), pos_offset, ptr(row0),
                                      ptr(lengths) if row0 is not None else None, rows if row0 is not None else 0, ptr(ws), nb))


def embed_bwd(dpre, B, Lq, dpos, pos_offset, row0=None, lengths=None):
    D = dpre.shape[-1]
    check(lib.mts_embed_bwd(stream_ptr(), dtype_code(dpre.dtype), B, Lq, D, ptr(dpre), ptr(dpos), pos_offset, ptr(row0),
                            ptr(lengths) if row0 is not None else None))


def dropout_fwd(x, y, p, seed, mask=None, residual=None):
    """y = dropout(x) (+ residual); mask (uint8, same numel) records the kept elements for the backward."""
    check(lib.mts_dropout_fwd(stream_ptr(), dtype_code(x.dtype), x.numel(), ptr(x), ptr(residual), ptr(y), ptr(mask), float(p), int(seed)))


def dropout_bwd(dy, dx, mask, p):
    check(lib.mts_dropout_bwd(stream_ptr(), dtype_code(dy.dtype), dy.numel(), ptr(dy), ptr(dx), ptr(mask), float(p)))


def gelu_bwd(u, dy):
    check(lib.mts_gelu_bwd(stream_ptr(), dtype_code(u.dtype), u.numel(), ptr(u), ptr(dy)))


def relu_bwd(u, dy):
    check(lib.mts_relu_bwd(stream_ptr(), dtype_code(u.dtype), u.numel(), ptr(u), ptr(dy)))


def ffn_supported(dtype, M, D, F):
    return bool(lib.mts_ffn_supported(dtype_code(dtype), M, D, F)) if dtype in (torch.float32, torch.bfloat16) else False


def ffn_fwd(a1, w1, b1, w2, b2, u, f, s2, relu=False):
    """Fused feed-forward block (F = 256): u, f [M, F] and s2 [M, D] are views of buffers with room for ceil(M / 64) * 64 rows."""
    M, D = a1.shape
    with _timed(('ffn_fwd', M, D, w1.shape[0])):
        check(lib.mts_ffn_fwd(stream_ptr(), M, D, w1.shape[0], ptr(a1), ptr(w1), ptr(b1), ptr(w2), ptr(b2), int(relu), ptr(u), ptr(f), ptr(s2)))


def ffn_bwd_data(ds2, w1, w2, u, du, da1, relu=False):
    M, D = ds2.shape
    with _timed(('ffn_bwd', M, D, w1.shape[0])):
        check(lib.mts_ffn_bwd_data(stream_ptr(), M, D, w1.shape[0], ptr(ds2), ptr(w1), ptr(w2), ptr(u), int(relu), ptr(du), ptr(da1)))


def band_slots(radius):
    return lib.mts_band_slots(radius)


def band_attn_fwd(qkv, lengths, B, Lq, D, heads, radius, ctx, probs, row0=None, drop_p=0.0, drop_seed=0):
    """row0 (int32 [B], optional): packed batch -- document b owns rows row0[b] .. row0[b] + lengths[b] - 1 of qkv / ctx / probs."""
    with _timed(('band_fwd', B, Lq, D, heads, radius)):
        check(lib.mts_band_attn_fwd(stream_ptr(), dtype_code(qkv.dtype), B, Lq, D, heads, radius, ptr(qkv), ptr(lengths), ptr(ctx), ptr(probs),
                                    ptr(row0), float(drop_p), int(drop_seed)))


def band_attn_bwd(qkv, lengths, probs, dctx, B, Lq, D, heads, radius, dqkv, dscores, dbias=None, row0=None, drop_p=0.0, drop_seed=0):
    """dbias (fp32 [3D], optional): column sums of dqkv = q/k/v bias gradients, fused into the kernels' output stage."""
    q_scale = 1.0 / math.sqrt(D // heads)
    ws = _scratch(lib.mts_band_attn_bwd_workspace(B, Lq, D), qkv.device, 'band_bwd') if dbias is not None else None
    with _timed(('band_bwd', B, Lq, D, heads, radius)):
        check(lib.mts_band_attn_bwd(stream_ptr(), dtype_code(qkv.dtype), B, Lq, D, heads, radius, q_scale, ptr(qkv), ptr(lengths),
                                    ptr(probs), ptr(dctx), ptr(dqkv), ptr(dscores), ptr(dbias), ptr(ws), ptr(row0),
                                    qkv.shape[0] if row0 is not None else 0, float(drop_p), int(drop_seed)))


def full_attn_fwd(qkv, lengths, B, Lq, D, heads, ctx, lse, row0=None, drop_p=0.0, drop_seed=0):
    """Full self-attention over every valid key of each document; lse (fp32 [rows, heads]) receives the per-row log-sum-exp.
    row0 (int32 [B], optional): packed batch, as for band_attn_fwd."""
    with _timed(('full_fwd', B, Lq, D, heads)):
        check(lib.mts_full_attn_fwd(stream_ptr(), dtype_code(qkv.dtype), B, Lq, D, heads, ptr(qkv), ptr(lengths), ptr(ctx), ptr(lse),
                                    ptr(row0), float(drop_p), int(drop_seed)))


def full_attn_bwd(qkv, lengths, lse, ctx, dctx, B, Lq, D, heads, dqkv, dbias=None, row0=None, drop_p=0.0, drop_seed=0):
    """Backward of full_attn_fwd from its saved ctx and lse; dbias (fp32 [3D], optional): column sums of dqkv."""
    q_scale = 1.0 / math.sqrt(D // heads)
    ws = _scratch(lib.mts_full_attn_bwd_workspace(B, Lq, D, heads), qkv.device, 'full_bwd')
    with _timed(('full_bwd', B, Lq, D, heads)):
        check(lib.mts_full_attn_bwd(stream_ptr(), dtype_code(qkv.dtype), B, Lq, D, heads, q_scale, ptr(qkv), ptr(lengths), ptr(lse),
                                    ptr(ctx), ptr(dctx), ptr(dqkv), ptr(dbias), ptr(ws), ptr(row0),
                                    qkv.shape[0] if row0 is not None else 0, float(drop_p), int(drop_seed)))


def t5_local_attn_fwd(qkv, lengths, B, Lq, heads, radius, table, bucket_of_offset, ctx, lse, drop_p=0.0, drop_seed=0):
    """LongT5 local attention (include/mts.h): qkv [B*Lq, 3*heads*64], table fp32 [buckets, heads], bucket_of_offset int32 [2r+1];
    lse (fp32 [B*Lq, heads]) receives the per-row log-sum-exp."""
    with _timed(('t5_fwd', B, Lq, heads, radius)):
        check(lib.mts_t5_local_attn_fwd(stream_ptr(), dtype_code(qkv.dtype), B, Lq, heads, 64, radius, ptr(qkv), ptr(lengths), ptr(table),
                                        table.shape[0], ptr(bucket_of_offset), ptr(ctx), ptr(lse), float(drop_p), int(drop_seed)))


def t5_local_attn_bwd(qkv, lengths, B, Lq, heads, radius, table, bucket_of_offset, lse, ctx, dctx, dqkv, dtable, drop_p=0.0, drop_seed=0):
    """Backward of t5_local_attn_fwd: dqkv (every row written) and dtable fp32 [buckets, heads] (overwritten)."""
    ws = _scratch(lib.mts_t5_local_attn_bwd_workspace(B, Lq, heads, radius), qkv.device, 't5_bwd')
    with _timed(('t5_bwd', B, Lq, heads, radius)):
        check(lib.mts_t5_local_attn_bwd(stream_ptr(), dtype_code(qkv.dtype), B, Lq, heads, 64, radius, ptr(qkv), ptr(lengths), ptr(table),
                                        table.shape[0], ptr(bucket_of_offset), ptr(lse), ptr(ctx), ptr(dctx), ptr(dqkv), ptr(dtable),
                                        ptr(ws), float(drop_p), int(drop_seed)))


def rmsnorm_fwd(x, w, eps, y, rstd):
    rows, D = x.shape
    check(lib.mts_rmsnorm_fwd(stream_ptr(), dtype_code(x.dtype), rows, D, ptr(x), ptr(w), float(eps), ptr(y), ptr(rstd)))


def rmsnorm_bwd(x, dy, w, rstd, dx, dw, dres=None):
    """dx = RMSNorm backward (+ dres; dx may be dres itself); dw fp32 [D] overwritten."""
    rows, D = x.shape
    ws = _scratch(lib.mts_rmsnorm_bwd_workspace(rows, D), x.device, 'rms_bwd')
    check(lib.mts_rmsnorm_bwd(stream_ptr(), dtype_code(x.dtype), rows, D, ptr(x), ptr(dy), ptr(dres), ptr(w), ptr(rstd), ptr(dx), ptr(dw),
                              ptr(ws)))


def pair_score_fwd(F, G, B, Lq, scores):
    """scores[b, t] = F[b, t] . G[b, t + 1] for t < Lq - 1, 1.0 at t = Lq - 1 (include/mts.h).  F, G: [B*Lq, H] views in the activation
    dtype (row strides free: the two halves of one buffer); scores fp32 [B, Lq]."""
    H = F.shape[1]
    with _timed(('pair_fwd', B, Lq, H)):
        check(lib.mts_pair_score_fwd(stream_ptr(), dtype_code(F.dtype), B, Lq, H, ptr(F), F.stride(0), ptr(G), G.stride(0), ptr(scores)))


def pair_score_bwd(F, G, dscores, B, Lq, dF, dG):
    """Backward of pair_score_fwd: every row of dF and dG is overwritten (dscores[b, Lq - 1] is never read)."""
    H = F.shape[1]
    with _timed(('pair_bwd', B, Lq, H)):
        check(lib.mts_pair_score_bwd(stream_ptr(), dtype_code(F.dtype), B, Lq, H, ptr(F), F.stride(0), ptr(G), G.stride(0), ptr(dscores),
                                     ptr(dF), dF.stride(0), ptr(dG), dG.stride(0)))


def gate_merge_fwd(a, h1, h2, m):
    """m = z h1 + (1 - z) h2 with z = sigmoid(a) (include/mts.h "Gated merge").  a, h1, h2, m: [rows, W] views in the activation dtype
    (row strides free, columns contiguous); m is overwritten."""
    rows, W = a.shape
    with _timed(('gate_fwd', rows, W)):
        check(lib.mts_gate_merge_fwd(stream_ptr(), dtype_code(a.dtype), rows, W, ptr(a), a.stride(0), ptr(h1), h1.stride(0), ptr(h2), h2.stride(0),
                                     ptr(m), m.stride(0)))
    return m


def gate_merge_bwd(a, h1, h2, dm, da, dh1, dh2):
    """Backward of gate_merge_fwd: da = dm (h1 - h2) z (1 - z), dh1 = dm z, dh2 = dm - dm z, all three overwritten (z recomputed from a)."""
    rows, W = a.shape
    with _timed(('gate_bwd', rows, W)):
        check(lib.mts_gate_merge_bwd(stream_ptr(), dtype_code(a.dtype), rows, W, ptr(a), a.stride(0), ptr(h1), h1.stride(0), ptr(h2), h2.stride(0),
                                     ptr(dm), dm.stride(0), ptr(da), da.stride(0), ptr(dh1), dh1.stride(0), ptr(dh2), dh2.stride(0)))


class SegmentTable:
    """Host tables of the cosine auxiliary segment loss (include/mts.h "Cosine auxiliary segment loss"), int32 numpy arrays:
    seg [n_seg, 8], pair [n_pair, 4], row_map [B * L]."""

    def __init__(self, seg, pair, row_map, B, L):
        self.seg, self.pair, self.row_map, self.B, self.L = seg, pair, row_map, B, L
        self.n_seg, self.n_pair = int(seg.shape[0]), int(pair.shape[0])


def segment_table(segments, lengths, B, L):
    """Host side of the cosine auxiliary loss: ``segments[b]`` = the segment ends of document b (models/CRF.py:23-69) -> SegmentTable.

    Per document with ends s_0 < s_1 < ..: the listed segments [0, s_0), [s_0, s_1), .. and the tail [s_last, lengths[b]) (maybe empty);
    a positive pair for every listed segment of more than one row, a negative pair (segment, next segment) for every listed segment.
    Pairs are numbered as upstream concatenates them: every positive pair in document order, then every negative pair.  A document with
    an empty list has no segment and no pair.  Entries of ``segments`` past B are ignored; fewer than B raise IndexError, as upstream.
    Every list must be strictly ascending with 0 < s <= lengths[b] (clamped to L): anything else is a ValueError -- upstream, Python
    slicing silently yields empty or clipped slices there (DESIGN.md "Cosine auxiliary segment loss")."""
    import numpy as np
    B, L = int(B), int(L)
    if isinstance(segments, torch.Tensor):
        segments = segments.tolist()
    if isinstance(segments, (str, bytes)) or not hasattr(segments, '__len__') or not hasattr(segments, '__getitem__'):
        raise ValueError(f'segments must be a sequence of lists of segment ends, one per document; got {type(segments).__name__}')
    if lengths is None:
        lens = [L] * B
    else:
        lens = [int(v) for v in (lengths.tolist() if hasattr(lengths, 'tolist') else lengths)]
        if len(lens) != B:
            raise ValueError(f'lengths has {len(lens)} entries for a batch of {B} documents')
    if len(segments) < B:
        raise IndexError('list index out of range')                   # segment_indeces[batch_index], models/CRF.py:34
    n = np.clip(np.asarray(lens, dtype=np.int64), 0, L)
    docs = []
    for b in range(B):
        d = segments[b]
        arr = np.asarray(d.tolist() if hasattr(d, 'tolist') else d)
        if arr.size and (arr.ndim != 1 or arr.dtype.kind not in 'iu' or any(isinstance(v, bool) for v in d)):
            raise ValueError(f'segments[{b}] must be a flat list of integers; got {list(d)!r}')
        docs.append(arr.astype(np.int64).reshape(-1))
    counts = np.array([a.size for a in docs], dtype=np.int64)
    K = int(counts.sum())
    ends = np.concatenate(docs) if K else np.zeros(0, dtype=np.int64)
    doc = np.repeat(np.arange(B, dtype=np.int64), counts)
    first = np.zeros(K, dtype=bool)
    first[(np.cumsum(counts) - counts)[counts > 0]] = True            # the first listed end of its document
    begins = np.where(first, 0, np.concatenate(([0], ends[:-1]))) if K else ends
    bad = ~((begins < ends) & (ends <= n[doc]))
    if bad.any():
        b = int(doc[np.flatnonzero(bad)[0]])
        raise ValueError(f'segments[{b}] = {docs[b].tolist()} must be strictly ascending with 0 < s <= {int(n[b])} (the length of document {b})')
    # segment order: a document's listed segments, then its tail (last end .. length: the last negative pair's partner, maybe empty)
    has = counts > 0
    rank = np.cumsum(has) - has                                       # documents with a list in front of document b
    S = K + int(has.sum())
    seg = np.zeros((S, 8), dtype=np.int32)
    seg[:, 4:7] = -1
    at = np.arange(K, dtype=np.int64) + rank[doc]                     # where listed segment i goes
    seg[at, 0], seg[at, 1], seg[at, 2] = doc, begins, ends
    hd = np.flatnonzero(has)
    tail = np.cumsum(counts)[hd] + rank[hd]
    seg[tail, 0], seg[tail, 1], seg[tail, 2], seg[tail, 3] = hd, ends[np.cumsum(counts)[hd] - 1] if K else 0, n[hd], 1
    # pairs as upstream concatenates them: every positive pair (listed segments of more than one row), then every negative pair
    pos = at[(ends - begins) > 1]
    npos = pos.size
    pair = np.zeros((npos + K, 4), dtype=np.int32)
    pair[:npos, 0], pair[:npos, 1], pair[:npos, 2] = pos, pos, 1
    pair[npos:, 0], pair[npos:, 1], pair[npos:, 2] = at, at + 1, -1
    seg[pos, 4] = np.arange(npos)
    seg[at, 5] = seg[at + 1, 6] = npos + np.arange(K)
    # row map in one vector pass: row doc * L + begin + k of segment s -> 2 s + (k & 1)
    row_map = np.full(B * L, -1, dtype=np.int32)
    n_rows = (seg[:, 2] - seg[:, 1]).astype(np.int64)
    if n_rows.sum():
        sid = np.repeat(np.arange(S, dtype=np.int64), n_rows)
        k = np.arange(int(n_rows.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_rows) - n_rows, n_rows)
        row_map[np.repeat(seg[:, 0].astype(np.int64) * L + seg[:, 1], n_rows) + k] = (2 * sid + (k & 1)).astype(np.int32)
    return SegmentTable(seg, pair, row_map, B, L)


class _DeviceSegmentTable:
    def __init__(self, tab, device):
        import numpy as np
        self.n_seg, self.n_pair, self.B, self.L = tab.n_seg, tab.n_pair, tab.B, tab.L
        flat = torch.from_numpy(np.concatenate([tab.seg.ravel(), tab.pair.ravel(), tab.row_map])).to(device)      # one upload
        a, b = tab.seg.size, tab.seg.size + tab.pair.size
        self.seg, self.pair, self.row_map = flat[:a], flat[a:b], flat[b:]


def segment_tables(segments, lengths, B, L, device):
    """segment_table on the device: validated and built on the host for every call (vector passes: well under a millisecond at
    64 x 256), then one small upload."""
    return _DeviceSegmentTable(segment_table(segments, lengths, B, L), device)


def segment_cosine_fwd(x, tab, loss_out, pair_cos=None):
    """loss_out fp32 [2] = {mean cosine-embedding term over tab's pairs, n_pair} (include/mts.h).  x: [B*L, W] view in the activation
    dtype (row stride free); tab: segment_tables(...).  -> the workspace, which segment_cosine_bwd needs untouched."""
    W = x.shape[1]
    assert x.shape[0] == tab.B * tab.L and x.stride(1) == 1
    ws = _scratch(lib.mts_segment_cosine_workspace(tab.n_seg, tab.n_pair, W), x.device, 'segcos')
    with _timed(('segcos_fwd', tab.B, tab.L, W)):
        check(lib.mts_segment_cosine_fwd(stream_ptr(), dtype_code(x.dtype), tab.B, tab.L, W, ptr(x), x.stride(0), tab.n_seg, ptr(tab.seg),
                                         tab.n_pair, ptr(tab.pair), ptr(loss_out), ptr(pair_cos), ptr(ws)))
    return ws


def segment_cosine_bwd(tab, scale, dx, ws, accumulate=True):
    """dx[r] (+)= scale * d(sum of the pair terms)/dx[r]; rows in no segment: untouched (accumulate) or written 0."""
    W = dx.shape[1]
    assert dx.shape[0] == tab.B * tab.L and dx.stride(1) == 1
    with _timed(('segcos_bwd', tab.B, tab.L, W)):
        check(lib.mts_segment_cosine_bwd(stream_ptr(), dtype_code(dx.dtype), tab.B, tab.L, W, tab.n_seg, ptr(tab.seg), tab.n_pair, ptr(tab.pair),
                                         ptr(tab.row_map), float(scale), int(accumulate), ptr(dx), dx.stride(0), ptr(ws)))


def tagger_loss(kind, scores, targets, lengths, alpha, gamma, loss_out, dscores, row_src=None, batch_shape=None):
    """scores [B, L, n_out]; or, for a packed batch, [n_rows, n_out] with row_src (int32 [n_rows]) and batch_shape = (B, L)."""
    if row_src is None:
        B, Lq, n_out = scores.shape
    else:
        (B, Lq), n_out = batch_shape, scores.shape[-1]
    nb = lib.mts_tagger_loss_workspace(B, Lq)
    ws = _scratch(nb, scores.device, 'loss')
    check(lib.mts_tagger_loss(stream_ptr(), kind, B, Lq, targets.shape[1], n_out, ptr(scores), ptr(targets), ptr(lengths),
                              float(alpha), float(gamma), ptr(loss_out), ptr(dscores), ptr(ws), nb, ptr(row_src),
                              row_src.numel() if row_src is not None else 0))


def greedy_decode(scores, lengths, threshold, tags_out):
    B, Lq, n_out = scores.shape
    check(lib.mts_greedy_decode(stream_ptr(), B, Lq, n_out, ptr(scores), ptr(lengths), float(threshold), ptr(tags_out)))


def segment_decode(scores, lengths, threshold, seg_end, n_seg, min_segment=1, close_last=True, tags=None, prob=None):
    """boundary tags, probabilities and the segment table of every document in one launch (include/mts.h mts_segment_decode): scores fp32
    [B, L, n_out], lengths int32 [B] or None.  ``min_segment == 1``: tag = prob > threshold, greedy_decode's bits; ``>= 2``: the best
    boundary set whose segments all hold at least that many sentences, exact in integers.  seg_end int32 [B, Smax]: the exclusive ends of
    the segments in order (the tail's, the document's length, under ``close_last``), -1 behind; n_seg int32 [B]: their number, not
    clipped to Smax; tags uint8 [B, L] and prob fp32 [B, L] are optional.  Every element of every output is written.
    -> (seg_end, n_seg)"""
    assert scores.dim() == 3 and scores.dtype == torch.float32 and scores.is_contiguous()
    B, Lq, n_out = scores.shape
    assert lengths is None or (lengths.dtype == torch.int32 and lengths.numel() == B and lengths.is_contiguous() and lengths.device == scores.device)
    assert seg_end.dtype == torch.int32 and seg_end.dim() == 2 and seg_end.shape[0] == B and seg_end.is_contiguous()
    assert n_seg.dtype == torch.int32 and n_seg.numel() == B and n_seg.is_contiguous()
    assert tags is None or (tags.dtype == torch.uint8 and tags.numel() == B * Lq and tags.is_contiguous() and tags.device == scores.device)
    assert prob is None or (prob.dtype == torch.float32 and prob.numel() == B * Lq and prob.is_contiguous() and prob.device == scores.device)
    assert scores.device == seg_end.device == n_seg.device
    check(lib.mts_segment_decode(stream_ptr(), B, Lq, n_out, ptr(scores), ptr(lengths), float(threshold), int(min_segment),
                                 int(bool(close_last)), int(seg_end.shape[1]), ptr(tags), ptr(prob), ptr(seg_end), ptr(n_seg)))
    return seg_end, n_seg


def _sweep_operands(scores, targets, lengths, thresholds, counts_out, width):
    """the argument checks the two sweep kernels share -> (B, L, n_out, T)"""
    B, Lq, n_out = scores.shape
    T = thresholds.numel()
    assert scores.dtype == torch.float32 and targets.dtype == torch.float32 and thresholds.dtype == torch.float32
    assert scores.is_contiguous() and targets.is_contiguous() and thresholds.is_contiguous() and targets.shape[0] == B
    assert lengths is None or (lengths.dtype == torch.int32 and lengths.numel() == B and lengths.is_contiguous())
    assert counts_out.dtype == torch.int32 and counts_out.is_contiguous() and counts_out.numel() == B * T * width
    return B, Lq, n_out, T


def threshold_sweep(scores, targets, lengths, thresholds, counts_out, end_boundary=False):
    """counts_out int32 [B, T, 6] = {pk_err, wd_err, windows, tp, fp, fn} of every document x threshold (include/mts.h): scores fp32
    [B, L, n_out], targets fp32 [B, Lt >= L], lengths int32 [B] or None, thresholds fp32 [T] on the device.  The decision is
    greedy_decode's ``prob > threshold``, bit for bit."""
    B, Lq, n_out, T = _sweep_operands(scores, targets, lengths, thresholds, counts_out, 6)
    check(lib.mts_threshold_sweep(stream_ptr(), B, Lq, targets.shape[1], n_out, ptr(scores), ptr(targets), ptr(lengths), T, ptr(thresholds),
                                  int(bool(end_boundary)), ptr(counts_out)))


def winpr_sweep(scores, targets, lengths, thresholds, counts_out, end_boundary=False, k=10):
    """counts_out int32 [B, T, 3] = {TP, FP, FN} of WinPR(reference=tags, hypothesis=target, k) for every document x threshold
    (include/mts.h); operands as threshold_sweep; k in 1..64."""
    B, Lq, n_out, T = _sweep_operands(scores, targets, lengths, thresholds, counts_out, 3)
    check(lib.mts_winpr_sweep(stream_ptr(), B, Lq, targets.shape[1], n_out, ptr(scores), ptr(targets), ptr(lengths), T, ptr(thresholds),
                              int(bool(end_boundary)), int(k), ptr(counts_out)))


def bootstrap_sums(values, samples, seed=0, out=None):
    """-> float64 [M, samples] on the device: sums[m, s] = the sequential float64 sum of values[m, i_0 .. i_{n-1}], the n indices of
    resample s drawn with replacement by the counter hash of (seed, s * n + j) and shared by the M rows (include/mts.h).  values: float64
    [M, n] (or [n]) on the device; n 1..2^20, M 1..16, samples 1..2^22.  One launch."""
    if values.dim() == 1:
        values = values.view(1, -1)
    assert values.dim() == 2 and values.dtype == torch.float64 and values.is_contiguous() and values.device.type == 'cuda'
    M, n = values.shape
    S = int(samples)
    if out is None:
        out = torch.empty(M, max(S, 0), dtype=torch.float64, device=values.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == M * max(S, 0) and out.device == values.device
    check(lib.mts_bootstrap_sums(stream_ptr(), n, M, S, ptr(values), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out)))
    return out


def head_fwd(x, w, b, scores):
    rows, D = x.shape
    check(lib.mts_head_fwd(stream_ptr(), dtype_code(x.dtype), rows, D, w.shape[0], ptr(x), x.stride(0), ptr(w), ptr(b), ptr(scores)))


def head_bwd_params(x, dscores, dw, db):
    rows, D = x.shape
    ws = _scratch(lib.mts_layernorm_bwd_workspace(D), x.device, 'ln_bwd')
    check(lib.mts_head_bwd_params(stream_ptr(), dtype_code(x.dtype), rows, D, dw.shape[0], ptr(x), x.stride(0), ptr(dscores),
                                  ptr(dw), ptr(db), ptr(ws)))


def head_bwd_data(dscores, w, dx, accumulate=False):
    rows, D = dx.shape
    check(lib.mts_head_bwd_data(stream_ptr(), dtype_code(dx.dtype), rows, D, w.shape[0], ptr(dscores), ptr(w), ptr(dx),
                                dx.stride(0), int(accumulate)))


def switch_doc_maps(domains, B=None):
    """Host side of the domain-switched heads (include/mts.h): the three document maps of a batch's ``domains`` as int lists.

    models/CRF.py:1124-1139: idx1 = the documents whose domain is truthy (head 0 = classification_1), idx2 = the rest (head 1 =
    classification_2), both in batch order; ``regroup`` writes out[idx1[k]] = head_1(h)[k] and out[idx2[k]] = head_2(h)[k], so document
    i is scored from the encoder rows of document rank(i), its position inside its own group.  On a single-domain batch rank(i) = i.
    -> (doc_src [B], doc_head [B], doc_tgt [2 * B] = for head k and document r the one document of head k that reads r, or -1).
    ValueError for anything that is not a sequence of B entries, each 0 / 1 / a bool."""
    if isinstance(domains, torch.Tensor):
        domains = domains.tolist()
    if isinstance(domains, (str, bytes)) or not hasattr(domains, '__len__') or not hasattr(domains, '__iter__'):
        raise ValueError(f'domains must be a sequence of 0 / 1 / bool, one per document; got {type(domains).__name__}')
    doms = list(domains)
    if B is not None and len(doms) != B:
        raise ValueError(f'domains has {len(doms)} entries for a batch of {B} documents')
    for d in doms:
        if isinstance(d, bool) or (hasattr(d, '__index__') and not isinstance(d, float) and int(d) in (0, 1)):
            continue
        raise ValueError(f'domains entries must be 0, 1 or a bool; got {d!r}')
    n = len(doms)
    src, head, tgt = [0] * n, [0] * n, [-1] * (2 * n)
    rank = [0, 0]
    for i, d in enumerate(doms):
        k = 0 if d else 1
        src[i], head[i] = rank[k], k
        tgt[k * n + rank[k]] = i
        rank[k] += 1
    return src, head, tgt


_SWITCH_MAPS_CACHE = {}


def switch_maps(domains, B, device):
    """switch_doc_maps on the device (int32): one small upload per distinct (domains, device), none per step."""
    if isinstance(domains, torch.Tensor):
        domains = domains.tolist()
    try:
        key = (tuple((type(d), d) for d in domains), int(B), str(torch.device(device)))
        hit = _SWITCH_MAPS_CACHE.get(key)
    except TypeError:
        key = hit = None
    if hit is None:
        src, head, tgt = switch_doc_maps(domains, B)
        up = torch.tensor([src, head, tgt[:B], tgt[B:]], dtype=torch.int32).reshape(4, B).to(device)
        hit = (up[0], up[1], up[2:].reshape(-1))
        if key is not None:
            if len(_SWITCH_MAPS_CACHE) > 64:
                _SWITCH_MAPS_CACHE.clear()
            _SWITCH_MAPS_CACHE[key] = hit
    return hit


def _switch_check(who, act, B, Lq, w):
    """The operands mts_switch_head_* does not cover, refused here as ValueError before anything is launched."""
    rows, D = act.shape
    if rows != B * Lq:
        raise ValueError(f'{who}: {rows} rows for a batch of {B} x {Lq}')
    if D % 4 or act.stride(0) % 4 or act.stride(1) != 1:
        raise ValueError(f'{who}: D = {D} and the row stride {act.stride(0)} must be multiples of 4 (4-element vectors), columns contiguous')
    if act.data_ptr() % (4 * act.element_size()):
        raise ValueError(f'{who}: the {act.dtype} operand must be aligned to a 4-element vector ({4 * act.element_size()} bytes)')
    if w.dim() != 3 or w.shape[0] != 2 or not 1 <= w.shape[1] <= 4 or w.shape[2] != D or not w.is_contiguous() or w.dtype != torch.float32:
        raise ValueError(f'{who}: head weights must be contiguous fp32 [2, n_out <= 4, {D}], got {tuple(w.shape)}')


def switch_head_fwd(x, w, b, domains, B, Lq, scores):
    """scores[b, t, c] = x[doc_src[b], t, :] . w[doc_head[b], c, :] + b[doc_head[b], c] (include/mts.h).  x: [B*Lq, D] act dtype (row
    stride free), w fp32 [2, n_out, D], b fp32 [2, n_out], domains: the batch's host list, scores fp32 [B*Lq, n_out]."""
    _switch_check('switch_head_fwd', x, B, Lq, w)
    src, head, _ = switch_maps(domains, B, x.device)
    check(lib.mts_switch_head_fwd(stream_ptr(), dtype_code(x.dtype), B, Lq, x.shape[1], w.shape[1], ptr(x), x.stride(0), ptr(w), ptr(b),
                                  ptr(src), ptr(head), ptr(scores)))


def switch_head_bwd_params(x, dscores, domains, B, Lq, dw, db):
    """dw fp32 [2, n_out, D], db fp32 [2, n_out]: OVERWRITTEN; the head no document uses with exact zeros."""
    _switch_check('switch_head_bwd_params', x, B, Lq, dw)
    src, head, _ = switch_maps(domains, B, x.device)
    ws = _scratch(lib.mts_switch_head_bwd_workspace(x.shape[1]), x.device, 'switch_bwd')
    check(lib.mts_switch_head_bwd_params(stream_ptr(), dtype_code(x.dtype), B, Lq, x.shape[1], dw.shape[1], ptr(x), x.stride(0), ptr(dscores),
                                         ptr(src), ptr(head), ptr(dw), ptr(db), ptr(ws)))


def switch_head_bwd_data(dscores, w, domains, B, Lq, dx):
    """dx[r, t, :] = sum_k sum_c dscores[doc_tgt[k][r], t, c] w[k, c, :]: every row OVERWRITTEN, rows no document reads with zeros."""
    _switch_check('switch_head_bwd_data', dx, B, Lq, w)
    _, _, tgt = switch_maps(domains, B, dx.device)
    check(lib.mts_switch_head_bwd_data(stream_ptr(), dtype_code(dx.dtype), B, Lq, dx.shape[1], w.shape[1], ptr(dscores), ptr(w), ptr(tgt),
                                       ptr(dx), dx.stride(0)))


def lstm_workspace(dtype, B, Lq, H, ndir, device, tag='lstm'):
    return _scratch(lib.mts_lstm_workspace(dtype_code(dtype), B, Lq, H, ndir), device, tag)


def lstm_fwd(xproj, w_hh, b_hh, lengths, B, Lq, H, ndir, out, gates, cells):
    ws = lstm_workspace(xproj.dtype, B, Lq, H, ndir, xproj.device)
    check(lib.mts_lstm_fwd(stream_ptr(), dtype_code(xproj.dtype), B, Lq, H, ndir, ptr(xproj), ptr(w_hh), ptr(b_hh), ptr(lengths), ptr(out),
                           ptr(gates), ptr(cells), ptr(ws)))


def lstm_bwd(w_hh, lengths, out, gates, cells, dout, B, Lq, H, ndir, dxproj, dw_hh, ws=None):
    if ws is None:
        ws = lstm_workspace(out.dtype, B, Lq, H, ndir, out.device)
    check(lib.mts_lstm_bwd(stream_ptr(), dtype_code(out.dtype), B, Lq, H, ndir, ptr(w_hh), ptr(lengths), ptr(out), ptr(gates),
                           ptr(cells), ptr(dout), ptr(dxproj), ptr(dw_hh), ptr(ws)))


def crf_nll(feats, tags, lengths, trans, loss_out, dfeats=None, dtrans=None):
    B, Lq, C = feats.shape
    ws = _scratch(lib.mts_crf_workspace(B, Lq, C), feats.device, 'crf')
    check(lib.mts_crf_nll(stream_ptr(), B, Lq, C, ptr(feats), ptr(tags), tags.shape[1], ptr(lengths), ptr(trans), ptr(loss_out),
                          ptr(dfeats), ptr(dtrans), ptr(ws)))


def crf_viterbi(feats, lengths, trans, best_score, paths):
    B, Lq, C = feats.shape
    ws = _scratch(B * Lq * C * 4, feats.device, 'crf_bp')
    check(lib.mts_crf_viterbi(stream_ptr(), B, Lq, C, ptr(feats), ptr(lengths), ptr(trans), ptr(best_score), ptr(paths), ptr(ws)))


def crf_marginals(feats, lengths, trans, scores, cls=1, logz=None):
    """scores fp32 [B, L] (every element OVERWRITTEN): the clamped logit of P(y_t = cls | x), 0 past a document's length; logz fp32 [B]."""
    B, Lq, C = feats.shape
    ws = _scratch(lib.mts_crf_workspace(B, Lq, C), feats.device, 'crf')
    check(lib.mts_crf_marginals(stream_ptr(), B, Lq, C, int(cls), ptr(feats), ptr(lengths), ptr(trans), ptr(scores), ptr(logz), ptr(ws)))


# ---- the CRF on packed rows (include/mts.h): feats fp32 [n_rows, C], document b in rows row0[b] .. row0[b] + len_b - 1; B and L (the
# longest document the kernels walk) come with ``shape``; row0 = None is the padded layout ([B * L, C] rows)
def crf_nll_packed(feats, tags, lengths, trans, loss_out, shape, row0=None, dfeats=None, dtrans=None):
    (B, Lq), (n_rows, C) = shape, feats.shape
    ws = _scratch(lib.mts_crf_workspace(B, Lq, C), feats.device, 'crf')
    check(lib.mts_crf_nll_packed(stream_ptr(), B, Lq, C, ptr(feats), ptr(tags), tags.shape[1], ptr(lengths), ptr(trans), ptr(loss_out),
                                 ptr(dfeats), ptr(dtrans), ptr(ws), ptr(row0), n_rows))


def crf_viterbi_packed(feats, lengths, trans, best_score, paths, row0=None):
    """paths int32 [B, L] (-1 past a document's length), best_score fp32 [B]"""
    (B, Lq), (n_rows, C) = paths.shape, feats.shape
    ws = _scratch(max(n_rows, 1) * C * 4, feats.device, 'crf_bp')
    check(lib.mts_crf_viterbi_packed(stream_ptr(), B, Lq, C, ptr(feats), ptr(lengths), ptr(trans), ptr(best_score), ptr(paths), ptr(ws),
                                     ptr(row0), n_rows))


def crf_marginals_packed(feats, lengths, trans, scores, shape, row0=None, cls=1, logz=None):
    """scores fp32 [n_rows]: the clamped logit of P(y_t = cls | x) of every packed row"""
    (B, Lq), (n_rows, C) = shape, feats.shape
    ws = _scratch(lib.mts_crf_workspace(B, Lq, C), feats.device, 'crf')
    check(lib.mts_crf_marginals_packed(stream_ptr(), B, Lq, C, int(cls), ptr(feats), ptr(lengths), ptr(trans), ptr(scores), ptr(logz), ptr(ws),
                                       ptr(row0), n_rows))


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale=1.0, bf16_copy=None):
    check(lib.mts_adam_step(stream_ptr(), param.numel(), ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), lr, beta1, beta2,
                            eps, step, grad_scale, ptr(bf16_copy)))


def sgd_step(param, grad, buf, lr, momentum, weight_decay, first_step, grad_scale=1.0, bf16_copy=None):
    check(lib.mts_sgd_step(stream_ptr(), param.numel(), ptr(param), ptr(grad), ptr(buf), lr, momentum, weight_decay,
                           int(first_step), grad_scale, ptr(bf16_copy)))


def grad_norm_workspace(device):
    """fp32 workspace for grad_norm (the per-workgroup partial sums)."""
    return torch.empty(lib.mts_grad_norm_workspace() // 4, dtype=torch.float32, device=device)


def grad_norm(grad, spans, grad_scale, workspace, out):
    """out (0-d or 1-element fp32 DEVICE tensor) = || grad_scale * grad ||_2 over spans [(a, b), ...] of the flat fp32 gradient;
    no host synchronisation, bitwise reproducible (include/mts.h: mts_grad_norm).  Every a must be a multiple of 4 elements."""
    assert grad.dtype == torch.float32 and grad.is_contiguous() and out.dtype == torch.float32 and workspace.dtype == torch.float32
    assert workspace.numel() * 4 >= lib.mts_grad_norm_workspace()
    if not any(b > a for a, b in spans):
        out.zero_()
        return out
    begin = (ctypes.c_size_t * len(spans))(*[a for a, _ in spans])
    end = (ctypes.c_size_t * len(spans))(*[b for _, b in spans])
    check(lib.mts_grad_norm(stream_ptr(), ptr(grad), len(spans), begin, end, grad_scale, ptr(workspace), ptr(out)))
    return out


def adam_step_clipped(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale=1.0, bf16_copy=None, total_norm=None,
                      max_norm=0.0, clip_value=0.0, clip_coef_out=None):
    """adam_step on the clipped gradient: total_norm (device scalar from grad_norm) + max_norm = clip_grad_norm_, or clip_value =
    clip_grad_value_; clip_coef_out (device scalar, optional) receives the norm mode's coefficient."""
    check(lib.mts_adam_step_clipped(stream_ptr(), param.numel(), ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), lr, beta1, beta2,
                                    eps, step, grad_scale, ptr(bf16_copy), ptr(total_norm), max_norm, clip_value, ptr(clip_coef_out)))


def sgd_step_clipped(param, grad, buf, lr, momentum, weight_decay, first_step, grad_scale=1.0, bf16_copy=None, total_norm=None,
                     max_norm=0.0, clip_value=0.0, clip_coef_out=None):
    """sgd_step on the clipped gradient (the weight decay is added after clipping); arguments as adam_step_clipped."""
    check(lib.mts_sgd_step_clipped(stream_ptr(), param.numel(), ptr(param), ptr(grad), ptr(buf), lr, momentum, weight_decay,
                                   int(first_step), grad_scale, ptr(bf16_copy), ptr(total_norm), max_norm, clip_value, ptr(clip_coef_out)))


def scale_(x, scale):
    """x *= scale in place (fp32, contiguous)."""
    if scale != 1.0:
        assert x.dtype == torch.float32 and x.is_contiguous()
        check(lib.mts_scale(stream_ptr(), x.numel(), ptr(x), float(scale)))
    return x


def lstm_bwd_recurrence(w_hh, lengths, out, gates, cells, dout, B, Lq, H, ndir, dxproj, ws):
    """first half of lstm_bwd (the recurrence); ws: a workspace of lstm_workspace() size that lstm_bwd_whh gets again, untouched"""
    check(lib.mts_lstm_bwd_recurrence(stream_ptr(), dtype_code(out.dtype), B, Lq, H, ndir, ptr(w_hh), ptr(lengths), ptr(out), ptr(gates),
                                      ptr(cells), ptr(dout), ptr(dxproj), ptr(ws)))


def lstm_bwd_whh(lengths, out, dxproj, B, Lq, H, ndir, dw_hh, ws):
    """second half: h_{t-1} and dW_hh (any stream that is ordered behind the recurrence)"""
    check(lib.mts_lstm_bwd_whh(stream_ptr(), dtype_code(out.dtype), B, Lq, H, ndir, ptr(lengths), ptr(out), ptr(dxproj), ptr(dw_hh), ptr(ws)))
