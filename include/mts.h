/*
 * mts.h -- C ABI of the MI355X-native sentence-boundary tagger hot path (libmts_hip.so).
 *
 * Drop-in boundary: the reference (Ighina/MultimodalTopicSegmentation) is pure Python; its "operator
 * interface" for this path is the duck-type between models/lightning_model.py::TextSegmenter and the
 * tagger object it owns (models/CRF.py: .loss(xs, lengths, tags) -> scalar, .forward(xs, lengths) ->
 * (scores, tags), models/CRF.py:274-369, :371-479, :508-610) plus the batch dict of
 * EncoderDataset.py:91-152.  There is no FFI in the reference, so this header defines the C entry
 * points a ctypes binding on the reference side would call (INTEGRATION.md shows that binding).  Each
 * entry point names the reference code it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host; no ownership is transferred, the
 *    caller allocates outputs and workspaces (through torch, hipMalloc, ...);
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises;
 *  - row-major tensors, leading dimensions in ELEMENTS;
 *  - return value: 0 = MTS_OK, otherwise an mts_status; mts_last_error() gives a message (thread local);
 *  - Threads: every entry point may be called from any host thread, concurrently, on different streams.  The library keeps no
 *    mutable process-wide state that influences results or kernel choice: mts_last_error() and the tuning switches of
 *    mts_set_option() are PER HOST THREAD (a switch set by one thread applies to the calls that thread issues, and only
 *    those -- note that torch's autograd runs backward nodes on its own thread), mts_gemm_last_plan() reports the calling
 *    thread's most recent mts_gemm.  The only shared words are the record of the dynamic-LDS limit already set per
 *    (kernel, device) (atomics, appended under a mutex) and the sticky device-error word of mts_async_status();
 *  - "act dtype" = the arithmetic/storage type of activations: MTS_F32 (parity mode, fp32 everywhere) or
 *    MTS_BF16 (bf16 storage + MFMA, fp32 accumulate/statistics).  Parameters and gradients are always fp32.
 */
#ifndef MTS_H
#define MTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MTS_OK = 0,
  MTS_ERR_INVALID = 1,      /* bad argument (shape, alignment, enum) */
  MTS_ERR_UNSUPPORTED = 2,  /* valid but outside what the kernels cover */
  MTS_ERR_LAUNCH = 3,       /* HIP runtime error at launch */
  MTS_ERR_WORKSPACE = 4,    /* workspace too small */
  MTS_ERR_TIMEOUT = 5       /* an EARLIER launch reported a device-side timeout (see mts_async_status): its results are invalid */
} mts_status;

typedef enum { MTS_F32 = 0, MTS_BF16 = 1 } mts_dtype;

/* loss kinds: models/CRF.py:294-312 */
typedef enum { MTS_LOSS_CE = 0, MTS_LOSS_BCE = 1, MTS_LOSS_FOCAL = 2 } mts_loss_kind;

/* GEMM operand layouts.  C[M,N] = op(A) * op(B):
 *   MTS_NT : A is [M,K] (K contiguous), B is [N,K] (K contiguous)   -- y = x W^T        (forward)
 *   MTS_NN : A is [M,K] (K contiguous), B is [K,N] (N contiguous)   -- dx = dy W        (data grad)
 *   MTS_TN : A is [K,M] (M contiguous), B is [K,N] (N contiguous)   -- dW = dy^T x      (weight grad)
 *   MTS_TT : A is [K,M] (M contiguous), B is [N,K] (K contiguous)   -- dW = dy^T x for a caller that holds x^T: one
 *            operand less goes through the transposing LDS reads (measured +6 % on the wide weight gradients)            */
typedef enum { MTS_NT = 0, MTS_NN = 1, MTS_TN = 2, MTS_TT = 3 } mts_gemm_layout;

/* epilogue flags for mts_gemm */
#define MTS_EPI_BIAS      1u   /* += bias[n]  (fp32 [N])                                  */
#define MTS_EPI_RESIDUAL  2u   /* += residual[m,n]  (act dtype, ld = ldr)                 */
#define MTS_EPI_GELU      4u   /* C = gelu_erf(acc); pre-activation stored to `aux` if non-null */
#define MTS_EPI_COLSCALE  8u   /* columns n < ncols_scaled are multiplied by colscale (q / sqrt(hd)) */
#define MTS_EPI_ACCUM    16u   /* C += result (fp32 C only) */
#define MTS_EPI_RELU     32u   /* C = max(acc, 0); pre-activation stored to `aux` if non-null (legacy layer's FFN,
                                * models/RestrictedTransformerLayer.py:308); exclusive with MTS_EPI_GELU */

const char* mts_last_error(void);
/* version / build info: "mts-hip <n> gfx950" */
const char* mts_version(void);
/* tuning / A-B switches: "gemm_variant" = 0 | 1 (generic epilogue in the 256x224 kernel) | 5 (its K loop with the barrier at the end of the K-tile for every layout) ; "gemm_f32_mfma" = 1
 * (fp32 GEMM on v_mfma_f32_16x16x4_f32) | 0 (VALU kernel, bitwise the same results) ; "gemm_tile" = 0 (cost model) | 128 | 224 | 256 ; "gemm_glds" = 1 (LDS-DMA staging) | 0 (register
 * staging) ; "gemm_splits" = 0 (cost model) | n ; "gemm_order" = 1 (L2-blocked tile order) | 0 ; "gemm_chain" = 0 | 1 (split-K
 * of the 128x128 kernel accumulates in place) ; "gemm_deep" = 1 (four-buffer copy pipeline of the 128x128 kernel for grids of at
 * most one workgroup per CU) | 0 ; "band_mfma" = 1 | 0 ; "band_fused_bwd" = 1 (bf16 band attention backward in one pass where it applies:
 * radius <= 15, head dim <= 224) | 0 (two kernels) ; "lstm_parts" = 4 (CU-quad recurrences at H = 256, bf16 and fp32) | 2 (CU pair, bf16) ;
 * "full_mfma" = 1 | 0 (bf16 full attention on the matrix-core kernels where head dim % 32 == 0 and <= 256, else generic) ;
 * "t5_mfma" = 1 | 0 (bf16 LongT5 local attention on the matrix-core kernels, else generic) ;
 * "lstm_pair_spin_limit" = re-polls before a CU-pair LSTM workgroup gives
 * up on its partner (-1 = default 2^22; tests use 0) ; "lstm_pair_max_pairs" = CU pairs per recurrence launch (1..64, default 64) */
int mts_set_option(const char* key, int value);
/* Device-side errors that cannot be known at launch time, polled WITHOUT synchronising (a pinned host word the kernels write
 * with a system-scope store): 0, or MTS_ERR_TIMEOUT when a CU-pair LSTM launch gave up waiting for its partner workgroup since the
 * last poll (mts_last_error() says which).  mts_lstm_fwd / mts_lstm_bwd poll first themselves, so a training loop sees the error
 * at the next step at the latest; a host that has synchronised (decode, checkpoint) calls this.  Reading clears. */
int mts_async_status(void);
/* tile width (128 | 224 | 256; 225 / 226 = the 224-wide tile on the four-wave data-gradient kernel / the one-tile-per-workgroup forward kernel, symbols
 * of their own in a kernel trace) and K split the
 * cost model chose for the calling thread's most recent bf16 mts_gemm (bench / profiling labels) */
int mts_gemm_last_plan(int* tile, int* splits);
/* Measurement aid (per host thread; NULL clears it): fn() is called between the GEMM launch and the split-K reduce launch of every bf16 mts_gemm,
 * so that an event bracket can time the GEMM kernel by itself. */
int mts_gemm_set_mid_hook(void (*fn)(void));
/* Two weight gradients of ONE shape in one launch (bf16 operands, fp32 results; the fused feed-forward block's dW1 and dW2, whose 8 output tiles each
 * fill half the chip at best when launched alone):  C1[M, N] (+)= A1[K, M]^T B1[K, N]  and  C2t[N, M] (+)= (A2[K, M]^T B2[K, N])^T -- the second one
 * is STORED TRANSPOSED (dW2 = ds2^T f is computed as f^T ds2, the shape of dW1).  A1 / A2 share lda, B1 / B2 share ldb.  Split-K slabs + fixed-order
 * reduces as mts_gemm (bitwise reproducible); workspace >= mts_wgrad_pair_workspace(M, N, K) bytes (0: shape not covered: M % 256, N % 224, K % 64 --
 * MTS_ERR_UNSUPPORTED, the caller issues two mts_gemm calls instead).  Replaces the backward of modeling_longformer.py:1113-1131 (parameter part). */
size_t mts_wgrad_pair_workspace(int M, int N, int K);
int mts_wgrad_pair(void* stream, int M, int N, int K, const void* A1, const void* B1, float* C1, int ldc1, const void* A2, const void* B2,
                   float* C2t, int ldc2t, int lda, int ldb, int accumulate, void* workspace, size_t workspace_bytes);
/* The planner by itself (pure host code, no device call): the tile width and K split mts_gemm WOULD use for this call under the
 * calling thread's options; workspace_bytes = 0 means "no split-K workspace".  tile / splits may be NULL. */
int mts_gemm_plan(int a_dtype, int c_dtype, int layout, int M, int N, int K, unsigned epilogue, size_t workspace_bytes,
                  int* tile, int* splits);

/* ---------------------------------------------------------------------------------------------
 * Dense projection GEMM (MFMA for bf16, exact-fp32 VALU kernel for parity mode).
 * Replaces: nn.Linear inside HF Longformer (modeling_longformer.py:504-506, :1069, :1114, :1128),
 * the LSTM input projection inside aten::lstm (models/NeuralArchitectures.py:113) and the tagger
 * heads (models/CRF.py:299-310, :554-566); plus their autograd backward.
 * a_dtype: dtype of A and B (and residual/aux); c_dtype: dtype of C (MTS_F32 or a_dtype).
 * workspace (optional, workspace_bytes, 16-byte aligned): scratch for split-K partial tiles of weight-gradient shapes
 * (fp32 C, no epilogue besides MTS_EPI_ACCUM); without it such shapes run unsplit.  bf16 operands: the first 8192 bytes
 * hold the arrival tickets of the in-launch combine (zeroed by the call itself), the partial planes follow -- a call that
 * may split K into S slices wants 8192 + S * M * N * 4 bytes.  Partials are summed in slice order whichever slice adds
 * them (the last one to arrive, inside the launch, or a reduce launch), so results are bitwise reproducible.
 * ------------------------------------------------------------------------------------------- */
int mts_gemm(void* stream, int a_dtype, int c_dtype, int layout, int M, int N, int K,
             const void* A, int lda, const void* B, int ldb, void* C, int ldc,
             const float* bias, const void* residual, int ldr, void* aux, int ldaux,
             unsigned epilogue, float colscale, int ncols_scaled, void* workspace, size_t workspace_bytes);

/* column sums of an [M,N] activation matrix into fp32 out[N] (bias gradients); deterministic two-stage
 * reduction through `partial` (mts_colsum_workspace(N) bytes). */
size_t mts_colsum_workspace(int N);
int mts_colsum(void* stream, int dtype, int M, int N, const void* X, int ldx, float* out, int accumulate,
               void* partial);

/* fp32 -> act dtype copy (weights to bf16), n elements */
int mts_cast(void* stream, int dst_dtype, const float* src, void* dst, size_t n);
/* K-SPLIT INPUT.  Early fusion in the reference is a host-side torch.cat of the text and audio embedding matrices of a document
 * (utils/load_datasets_precomputed.py:158-161).  The *2 / _concat entry points take the two fp32 matrices separately
 * (src1 [rows, D1] | src2 [rows, D2], D1 and D2 multiples of 4) so that the concatenated batch never exists: dst [rows, D1+D2] in the
 * act dtype for the recurrent taggers' first projection ... */
int mts_cast_concat(void* stream, int dst_dtype, size_t rows, int D1, int D2, const float* src1, const float* src2, void* dst);
/* HOST-SIDE COLLATION (no device call, no stream).  Replaces the `merge` closure of AudioPortionDataset.collater (EncoderDataset.py:20-27,
 * :103-109): B ragged documents docs[b] = [doc_rows[b], D] (src_dtype MTS_F32 | MTS_BF16, row-major, contiguous) -> dst [B, Lmax, D] in
 * dst_dtype, rows past min(doc_rows[b], Lmax) = pad_value (0 for the embeddings, -1 / 0 for the targets: EncoderDataset.py:23; the
 * reference's truncate = "pad / cut to exactly Lmax").  The one pass that pads also
 * narrows fp32 -> bf16 (round to nearest even) where the dtypes differ, and is split over `nthreads` host threads (a persistent pool inside the library).  dst may be pinned
 * memory: the batch is then ready for an asynchronous host-to-device copy as it stands (prefetch.DevicePrefetcher sends it unstaged). */
int mts_collate_pad(int src_dtype, int dst_dtype, int B, int Lmax, int D, const void* const* docs, const int64_t* doc_rows, void* dst,
                    float pad_value, int nthreads);
/* DEVICE-SIDE COLLATION from a corpus resident in HBM (resident.ResidentCorpus): the same batch as mts_collate_pad, gathered by a list
 * of document indices, so that a training step needs neither a host pass nor a host-to-device copy of the batch.
 *   dst[b, i, :] = corpus[row_start[d] + i, :]  for i < min(row_start[d + 1] - row_start[d], Lmax),  d = doc_index[b];
 *   every other element of dst = pad_value.  The kernel writes EVERY element of dst (no memset in front of it).
 * F32 -> F32 and BF16 -> BF16 copy bits; F32 -> BF16 rounds to nearest even and keeps a NaN quiet (sign and high payload kept, quiet
 * bit set: the bits of mts_collate_pad and of torch's .to(torch.bfloat16) on the device; torch's HOST conversion agrees on everything
 * but a NaN, for which its vector loop and its scalar tail give different bits); BF16 -> F32 is MTS_ERR_UNSUPPORTED.  The targets take the same entry point with D = 1, F32 -> F32
 * and pad_value -1 or 0.  All element offsets are 64-bit (B * Lmax * D may exceed 2^31).  A doc_index outside 0 .. n_docs - 1 gives an
 * all-pad document and no address is formed from it; row_start itself is trusted (ascending, row_start[n_docs] = total_rows).
 * One launch, plain vector stores, no atomics, no workspace; 16-byte accesses when the row's byte length and both base addresses are
 * multiples of 16, exact narrower ones otherwise (D = 770 in fp32, D = 1).  corpus and dst aligned to their element size.
 * MTS_ERR_INVALID before any device work: unknown dtypes, B < 0, Lmax < 1, D < 1, n_docs < 1, and with B > 0 a null corpus, row_start,
 * doc_index or dst.  B == 0 returns MTS_OK without a launch. */
int mts_gather_pad(void* stream, int src_dtype, int dst_dtype, int B, int Lmax, int D,
                   const void* corpus,          /* device [total_rows, D], row-major, contiguous */
                   const int64_t* row_start,    /* device [n_docs + 1], ascending, row_start[0] = 0 */
                   int n_docs,
                   const int32_t* doc_index,    /* device [B], repeats allowed */
                   void* dst,                   /* device [B, Lmax, D] in dst_dtype */
                   float pad_value);
/* SEGMENT-ORDER GATHER (resident.AugmentedCorpus; reference: the inverse_augmentation of cross_validation_split,
 * utils/load_datasets_precomputed.py:71-96, done in the gather instead of at load time).  mts_gather_pad with one more table in front of
 * the source row: destination document b is a list of row ranges of stored document d = doc_index[b], its "listed segments"
 * j = seg_ptr[b] .. seg_ptr[b + 1] - 1.  Listed segment j holds the destination rows seg_dst[j] <= t < seg_dst[j + 1] (the document's last
 * one: t < dst_len[b]) and copies them from the document's rows seg_src[j] onwards, both offsets relative to the document's first row:
 *   dst[b, t, :] = corpus[row_start[d] + seg_src[j] + (t - seg_dst[j]), :]  for t < min(dst_len[b], Lmax), j = the LAST listed segment of b
 *   with seg_dst[j] <= t;  every other element of dst = pad_value.  seg_dst ascends inside a document and starts at 0.
 * A row is written as pad, and no source address is formed for it, when doc_index[b] is outside 0 .. n_docs - 1, when no listed segment
 * holds it (seg_dst of the first one above t, or an empty list), or when its source row falls outside [row_start[d], row_start[d + 1]):
 * table CONTENTS are ordinary input, MTS_OK whatever they hold (seg_ptr is clamped to 0 .. n_listed); only the table SIZES are trusted, as
 * row_start is.  Dtypes, rounding, access widths, alignment, 64-bit offsets, "every element of dst written once by a plain vector store,
 * one launch, no memset, no atomics, no workspace" are those of mts_gather_pad -- the two share their copy units, width selection and copy
 * loop in csrc/gather.hip.  Rows of 64 or more access units: one wave owns four consecutive destination rows and finds their segment with
 * scalar loads (a binary search over the document's seg_dst for the first row, a forward walk for the rest); thinner rows: one lane per
 * destination unit, each lane searching for its own row.
 * close_last (may be NULL): the LABEL RULE for the targets, D = 1 and F32 -> F32 only (MTS_ERR_INVALID otherwise).  Of the rows copied, the
 * last row of every listed segment is written as 1.0 whatever the source holds, and the document's last row (t = dst_len[b] - 1, when
 * it is inside Lmax) as close_last[b] ? 1.0 : 0.0.
 * MTS_ERR_INVALID before any device work: what mts_gather_pad refuses, n_listed < 0, and with B > 0 a null seg_ptr or dst_len, or with
 * n_listed > 0 a null seg_dst or seg_src.  B == 0 returns MTS_OK without a launch. */
int mts_gather_segments(void* stream, int src_dtype, int dst_dtype, int B, int Lmax, int D,
                        const void* corpus,          /* device [total_rows, D], row-major, contiguous */
                        const int64_t* row_start,    /* device [n_docs + 1], ascending, row_start[0] = 0 */
                        int n_docs,
                        const int32_t* doc_index,    /* device [B], repeats allowed */
                        const int32_t* seg_ptr,      /* device [B + 1]: listed segments of document b */
                        const int32_t* seg_dst,      /* device [n_listed]: first destination row, ascending per document */
                        const int32_t* seg_src,      /* device [n_listed]: first source row inside the stored document */
                        int n_listed,
                        const int32_t* dst_len,      /* device [B]: rows of destination document b before the cut at Lmax */
                        const int32_t* close_last,   /* device [B] or NULL: the label rule */
                        void* dst,                   /* device [B, Lmax, D] in dst_dtype */
                        float pad_value);
/* NEGATIVE-SENTENCE MASKING (resident.MaskedCorpus; reference: --mask_inner_sentences / --mask_probability,
 * utils/load_datasets_precomputed.py:174-185, done per batch on the device instead of once at load time): the PLAN of a masked batch.
 * For batch row b, d = doc_index[b], rows r = 0 .. n-1 of document d (n = row_start[d + 1] - row_start[d], below 2^31):
 *   row r is KEPT when targets[row_start[d] + r] != 0, or when (uint64) mts_hash32(doc_seed[b], r) < T,
 *   T = clamp((uint64)(keep_probability * 4294967296.0), 0, 2^32), computed in double; mts_hash32 is the counter hash of the dropout
 *   kernels (splitmix64's finaliser of doc_seed + 0x9E3779B97F4A7C15 * (r + 1), high 32 bits).  keep_probability is the chance that a
 *   NEGATIVE row stays (upstream's code: `rand() > mask_probability and not label` drops): 1.0 keeps every row, 0.0 drops every negative,
 *   a boundary row is never dropped.  If no row of a non-empty document is kept, row 0 is kept (upstream would make an empty document).
 *   kept[b]       = the number of kept rows, NOT clipped to Lmax;
 *   src_row[b, t] = the document-relative index of the t-th kept row for t < min(kept[b], Lmax), -1 behind it.
 * A doc_index outside 0 .. n_docs - 1, or a document without rows, gives kept[b] = 0 and a row of -1; no address is formed from such an
 * index.  Every element of src_row and kept is written exactly once by a plain vector store: no memset in front, no atomics, no
 * workspace; integers, so bitwise reproducible.  One workgroup per batch row walks the document in chunks (any length): keep flags from
 * the hash, the place inside a wave from the popcount of the wave's ballot below the lane, the waves' totals through LDS, the running
 * count in a register.  mts_gather_rows builds the batch from src_row.
 * MTS_ERR_INVALID before any device work: B < 0, Lmax < 1, n_docs < 1, keep_probability outside [0, 1] or NaN, and with B > 0 a null
 * pointer.  B == 0 returns MTS_OK without a launch. */
int mts_mask_plan(void* stream, int B, int Lmax,
                  const float* targets,        /* device [total_rows] */
                  const int64_t* row_start,    /* device [n_docs + 1], ascending, row_start[0] = 0 */
                  int n_docs,
                  const int32_t* doc_index,    /* device [B], repeats allowed */
                  const uint64_t* doc_seed,    /* device [B] */
                  double keep_probability,
                  int32_t* src_row,            /* device [B, Lmax] out */
                  int32_t* kept);              /* device [B] out */
/* ROW-TABLE GATHER: mts_gather_pad with a row table in front of the source row.
 *   dst[b, t, :] = corpus[row_start[d] + src_row[b, t], :]  when 0 <= src_row[b, t] < row_start[d + 1] - row_start[d],  d = doc_index[b];
 *   every other element of dst = pad_value.
 * A negative entry, one at or behind the document's end, and every row of a doc_index outside 0 .. n_docs - 1 is written as pad without
 * forming an address: table CONTENTS are ordinary input, as in mts_gather_segments.  Dtypes, rounding, access widths, alignment, 64-bit
 * offsets, "every element of dst written once by a plain vector store, one launch, no memset, no atomics, no workspace" and the refusals
 * are those of mts_gather_pad -- the three gathers share their copy units, width selection and copy loop in csrc/gather.hip.  Rows of
 * 64 or more access units: one wave owns four consecutive destination rows and reads their table entries as wave-uniform values;
 * thinner rows (the targets, D = 1, which travel with their rows: no label rule): one lane per destination unit.
 * MTS_ERR_INVALID before any device work: what mts_gather_pad refuses, and with B > 0 a null src_row.  B == 0 returns MTS_OK. */
int mts_gather_rows(void* stream, int src_dtype, int dst_dtype, int B, int Lmax, int D,
                    const void* corpus,          /* device [total_rows, D], row-major, contiguous */
                    const int64_t* row_start,    /* device [n_docs + 1], ascending, row_start[0] = 0 */
                    int n_docs,
                    const int32_t* doc_index,    /* device [B], repeats allowed */
                    const int32_t* src_row,      /* device [B, Lmax]: document-relative source row of every destination row */
                    void* dst,                   /* device [B, Lmax, D] in dst_dtype */
                    float pad_value);
/* PCA PROJECTION OF THE RESIDENT CORPUS (pca.PcaReducer, ResidentCorpus.fit_pca / projected; reference: --pca_reduce / --pca_value,
 * EncoderDataset.py:49-70): the moments of the fit and the transform, csrc/pca.hip.  x is the corpus as stored: dtype MTS_F32 | MTS_BF16,
 * row-major [rows, D], contiguous, any alignment its dtype has.  All three run on the caller's stream, use no atomics, no workspace and no
 * dependence between workgroups, write every output element exactly once and give the same bits for the same inputs.
 * MTS_ERR_INVALID before any device work: an unknown dtype, a null pointer, rows < 1, D < 1, k outside 1 .. D;  MTS_ERR_UNSUPPORTED:
 * D > 4096 (the fp64 Gram matrix is D * D * 8 bytes), and for mts_pca_project the pair bf16 -> fp32.
 *   mts_pca_colsum   sum_out[d] = sum_r x[r, d] in fp64 (a thread adds every 16th row of a column, the 16 partial sums are added in order).
 *   mts_pca_gram     gram_out[i, j] = sum_r z[r, i] z[r, j],  z[r, d] = fl32(x[r, d] - center[d]): the element is upcast to fp32 and the centre
 *                    subtracted once, in fp32; products and sums on v_mfma_f32_32x32x2_f32 (exact fp32, a row-ordered fma chain); after
 *                    every PCA_SLICE = 1024 rows the fp32 accumulators are added to fp64 ones and restarted, so
 *                    |G - exact| <= (1024 + 4) 2^-24 sum_r |z_ri| |z_rj| elementwise at any number of rows.  One workgroup owns a 64 x 64
 *                    tile on or above the diagonal for all rows and writes the tile and its mirror: gram_out is exactly symmetric.
 *   mts_pca_project  y[r, j] = sum_d z[r, d] w[j, d] for j < k: the same staging, one fp32 fma chain over D on the same instruction, ONE
 *                    rounding to out_dtype (fp32, or bf16 round-to-nearest-even).  fp32 -> fp32, bf16 -> bf16, fp32 -> bf16. */
int mts_pca_colsum(void* stream, int dtype, int rows, int D,
                   const void* x,               /* device [rows, D] */
                   double* sum_out);            /* device [D] out */
int mts_pca_gram(void* stream, int dtype, int rows, int D,
                 const void* x,                 /* device [rows, D] */
                 const float* center,           /* device [D] */
                 double* gram_out);             /* device [D, D] out */
int mts_pca_project(void* stream, int in_dtype, int out_dtype, int rows, int D, int k,
                    const void* x,              /* device [rows, D] in in_dtype */
                    const float* center,        /* device [D] */
                    const float* w,             /* device [k, D], row-major: the components */
                    void* y);                   /* device [rows, k] in out_dtype, out */
/* SENTENCE POOLING OF FRAME-LEVEL FEATURES (frames.ResidentFrames, ResidentCorpus.with_frames; reference: extract_embeddings.py:644-667,
 * the six pooled variants _mean, _max, _mean_std, _max_std, _last, _delta_gap of a sentence's frame-level encoder output), csrc/frame_pool.hip.
 * frames is [total_frames, D], row-major, contiguous, MTS_F32 | MTS_BF16, any D >= 1 and any alignment its dtype has (16-byte accesses when
 * D is a multiple of 4 / 8 elements and the base is 16-byte aligned, element accesses otherwise).  Sentence s is the rows frame_start[s] ..
 * frame_start[s + 1] (int64 [n_sent + 1]); entries are clamped into 0 .. total_frames before an address is formed and row offsets are
 * 64-bit.  Output row s starts at out + s * ld_out (elements) in out_dtype MTS_F32 | MTS_BF16 (bf16: ONE rounding of the fp32 result, to
 * nearest even); ld_out may exceed the width of the block written and nothing outside the block is touched, so the block can be written
 * into the right-hand columns of a wider matrix.  A sentence without frames writes 0.  Both run on the caller's stream, use no atomics, no
 * workspace and no dependence between workgroups, write every element of the block exactly once and give the same bits for the same inputs.
 * MTS_ERR_INVALID before any device work: a null pointer, an unknown dtype / statistic / mode, n_sent < 1, D < 1, total_frames < 0, ld_out
 * smaller than the block written, nothing to compute (MTS_POOL_NONE without with_std).
 *   mts_frame_pool   the reductions, one launch: the first statistic (MTS_POOL_MEAN | MTS_POOL_MAX | MTS_POOL_NONE: none) into columns
 *                    [0, D) and, with_std = 1, the population standard deviation into the D columns behind it ([D, 2D); [0, D) after
 *                    MTS_POOL_NONE).  Per sentence of n frames and per column, the element upcast to fp32 once, every operation fp32 and
 *                    correctly rounded:  m = fl(fl(sum x) / n);  max exact;  std = fl(sqrt(fl(fl(sum fl(fl(x - m)^2)) / n))) -- the
 *                    deviations about the COMPUTED mean m, as np.std.  Order of a sum: wave w of four adds rows w, w + 4, .. in ascending
 *                    order into one chain, the four chains are added as ((p0 + p1) + p2) + p3.
 *   mts_frame_edges  the gathers: MTS_EDGE_LAST is the sentence's last frame; MTS_EDGE_DELTA_GAP is the frame at row frame_start[s + 1] (the
 *                    next sentence's first frame) minus the last frame, one fp32 subtraction, and the last frame itself where doc_last[s]
 *                    != 0 (the last sentence of its document: upstream's IndexError branch) or s = n_sent - 1.  doc_last may be null for
 *                    MTS_EDGE_LAST. */
typedef enum { MTS_POOL_NONE = 0, MTS_POOL_MEAN = 1, MTS_POOL_MAX = 2 } mts_pool_stat;
typedef enum { MTS_EDGE_LAST = 0, MTS_EDGE_DELTA_GAP = 1 } mts_edge_mode;
int mts_frame_pool(void* stream, int in_dtype, int out_dtype, int n_sent, int D, int first, int with_std,
                   const void* frames,          /* device [total_frames, D] in in_dtype */
                   int64_t total_frames,
                   const int64_t* frame_start,  /* device [n_sent + 1], ascending */
                   void* out,                   /* device: row s at out + s * ld_out, D or 2 D columns written */
                   int64_t ld_out);
int mts_frame_edges(void* stream, int in_dtype, int out_dtype, int n_sent, int D, int mode,
                    const void* frames,         /* device [total_frames, D] in in_dtype */
                    int64_t total_frames,
                    const int64_t* frame_start, /* device [n_sent + 1], ascending */
                    const uint8_t* doc_last,    /* device [n_sent]: 1 on the last sentence of a document */
                    void* out,                  /* device: row s at out + s * ld_out, D columns written */
                    int64_t ld_out);
/* MFCC SENTENCE FEATURES FROM RESIDENT WAVEFORMS (audio.ResidentAudio.mfcc; reference: extract_acoustic_features.py:58-72, the `mfcc`
 * encoder of train_fit.py:245-248: per sentence librosa.feature.mfcc(y, sr, n_mfcc=50) and its librosa.feature.delta, then mean and std over
 * the frames of both -- the last step is mts_frame_pool with MTS_POOL_MEAN and with_std on the [mfcc | delta] frames), csrc/mfcc.hip.
 * The definition is librosa 0.8.1's at the reference's arguments, restated; parity with librosa itself is UNPINNED (the tests' oracle is a
 * NumPy restatement of these lines).  Sentence s is the n = sent_len[s] samples of `wave` from sent_start[s] (both clamped into the
 * buffer before an address is formed; offsets are 64-bit) and owns the T = frame_start[s + 1] - frame_start[s] rows of the outputs from
 * row frame_start[s] (entries clamped into 0 .. total_frames); the caller sets T = 1 + n / hop (librosa's center=True).
 *   frame t   the n_fft samples t * hop - n_fft / 2 .. t * hop + n_fft / 2 - 1 of the sentence; an index outside 0 .. n - 1 is reflected about
 *             the sentence's OWN ends without repeating the end sample (np.pad(y, n_fft / 2, 'reflect'): the fold of period 2 (n - 1), n == 1
 *             constant), so every n >= 1 is defined and the neighbouring audio is never read;
 *   window    x[i] = fl(y[.] * window[i]); the host passes the periodic Hann window 0.5 - 0.5 cos(2 pi i / n_fft);
 *   power     P[k] = |X[k]|^2, k = 0 .. n_fft / 2, X = rfft(x) computed as an N = n_fft / 2 point complex transform of z[i] = x[2 i] + i x[2 i + 1]:
 *             Stockham passes Ns = 1, 4, 16, .. of radix 4 -- v_r = in[j + r N / 4] * tw[r k n_fft / (4 Ns)] (k = j mod Ns; no product in the first
 *             pass), a0 = v0 + v2, a1 = v0 - v2, a2 = v1 + v3, a3 = -i (v1 - v3), out[4 (j - k) + k + {0, Ns, 2 Ns, 3 Ns}] = a0 + a2, a1 + a3,
 *             a0 - a2, a1 - a3 -- and one radix-2 pass (a + w b, a - w b) last when log2 N is odd; then X[k] = E + tw[k] O with
 *             E = (Z[k] + conj Z[N - k]) / 2, O = -i (Z[k] - conj Z[N - k]) / 2, Z[N] = Z[0];  P = fl(fl(Xr^2) + fl(Xi^2)).  A complex product is
 *             four fp32 products and two sums, each rounded (no contraction).  tw[m] = exp(-2 pi i m / n_fft), m < n_fft, as (cos, -sin) pairs:
 *             window, tw, the mel weights and the DCT table are built by the host in fp64 and rounded ONCE to fp32; no sine, cosine or fast
 *             intrinsic is evaluated on the device;
 *   mel       M[m] = sum_j mel_w[mel_ptr[m] + j] * P[mel_first[m] + j], j = 0 .. mel_ptr[m + 1] - mel_ptr[m] - 1: ONE chain from 0 in ascending j,
 *             product and sum each rounded; filter-major, no scatter (table entries are clamped into the tables and the spectrum);
 *   dB        d = fl(10 * log10f(max(1e-10, M))), then max(d, fl(top - 80)), top = the same dB of the LARGEST mel power over all frames and bands
 *             of the sentence (the maximum is exact);
 *   MFCC      c[i] = sum_m d[m] dct[i][m]: eight fma chains (chain u takes m = u, u + 8, ..., ascending) added as ((a0 + a1) + (a2 + a3)) +
 *             ((a4 + a5) + (a6 + a7));
 *   delta     scipy.signal.savgol_filter(c, 9, polyorder=1, deriv=1, mode='interp') over the frames of the sentence: for 4 <= t <= T - 5,
 *             D[t] = fl(S / 60), S = sum_{k=1..4} fl(k * fl(c[t + k] - c[t - k])) from 0 in ascending k; D[0..3] = D[4] and D[T-4..T-1] = D[T-5]
 *             (the same bits); T < 9 (librosa raises there) is defined as D = 0.  The delta reads the fp32 MFCC, never a rounded output.
 * All run on the caller's stream, use no atomics and no dependence between workgroups of one launch, write every output element exactly
 * once and give the same bits for the same inputs.  MTS_ERR_INVALID before any device work: a null pointer, an unknown out_dtype, a size
 * < 1, n_fft no power of two in 64 .. 4096, n_mfcc > n_mels, ld_out < 2 n_mfcc, a workspace smaller than mts_mfcc_frames_workspace.
 * MTS_ERR_UNSUPPORTED: a DCT table beyond a workgroup's 64 KiB of LDS, more frames than one launch covers.
 *   mts_mel_frames   wave -> mel [total_frames, n_mels] fp32, the mel POWER before the log; one workgroup per frame.  A sentence without
 *                    samples writes 0.
 *   mts_mfcc_frames  mel -> out: row f at out + f * ld_out in out_dtype MTS_F32 | MTS_BF16 (bf16: ONE rounding of the fp32 value), columns
 *                    [0, n_mfcc) the MFCC, [n_mfcc, 2 n_mfcc) the delta; ld_out may exceed 2 n_mfcc and nothing outside the block is touched.
 *                    Three launches: the sentences' tops, the DCT into the workspace's fp32 MFCC, the block with the delta. */
int mts_mel_frames(void* stream, int n_sent, int n_fft, int hop, int n_mels,
                   const float* wave,           /* device [total_samples] */
                   int64_t total_samples,
                   const int64_t* sent_start,   /* device [n_sent]: first sample of the sentence */
                   const int64_t* sent_len,     /* device [n_sent]: its samples */
                   const int64_t* frame_start,  /* device [n_sent + 1], ascending */
                   int64_t total_frames,
                   const float* window,         /* device [n_fft] */
                   const float* twiddle,        /* device [n_fft, 2] */
                   const int32_t* mel_first,    /* device [n_mels]: first FFT bin of the filter */
                   const int32_t* mel_ptr,      /* device [n_mels + 1]: its weights are mel_w[mel_ptr[m] .. mel_ptr[m + 1]) */
                   const float* mel_w,          /* device [mel_nnz] */
                   int mel_nnz,
                   float* mel);                 /* device [total_frames, n_mels] out */
size_t mts_mfcc_frames_workspace(int n_sent, int64_t total_frames, int n_mfcc);
int mts_mfcc_frames(void* stream, int out_dtype, int n_sent, int n_mels, int n_mfcc,
                    const float* mel,           /* device [total_frames, n_mels] */
                    int64_t total_frames,
                    const int64_t* frame_start, /* device [n_sent + 1], ascending */
                    const float* dct,           /* device [n_mfcc, n_mels] */
                    void* workspace, size_t workspace_bytes,
                    void* out,                  /* device: row f at out + f * ld_out, 2 n_mfcc columns written */
                    int64_t ld_out);
/* PROSODIC SENTENCE FEATURES FROM RESIDENT WAVEFORMS (audio.ResidentAudio.pitch / yin / prosodic; reference: extract_acoustic_features.py
 * :20-55 and :74-108, the `prosodic` encoder of train_fit.py:245 (167 wide): librosa.pyin(y, fmin=70, fmax=500, sr=16000), the pause and
 * voiced-segment statistics of its voicing probability, mean and std of librosa.feature.melspectrogram(y, n_mels=40) and of its
 * librosa.feature.delta, and the pitch jump against the previous sentence's librosa.yin track), csrc/prosody.hip.  The definition is
 * librosa 0.8.1's, restated; parity with librosa itself is UNPINNED (the tests' oracle is a NumPy restatement of these lines).  RECALLED
 * rather than read, and named as such: the window-edge indexing of the difference function (j = 1 .. W below), the transition width
 * (round(35.92 * 12 * hop / sr) semitones * 10 + 1 = 141) and the Beta(2, 18) / Boltzmann(2) / 0.01 priors.  Sentences, frames and the
 * reflect fold are those of the MFCC block above (frame_length = 2048, hop = 512, T = 1 + n / hop at the defaults).
 *   difference  d(tau) = sum_{j=1..W} fl(fl(x[j] - x[j + tau])^2), tau = 1 .. max_period, x the frame_length samples of the frame, W = win_length:
 *               eight chains (chain u takes j = 1 + u, 9 + u, ..) added as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)).  The DIRECT
 *               form -- a deviation on purpose: librosa takes the products from an FFT autocorrelation and zeroes |.| < 1e-6;
 *   cmnd        c[i] = fl(d(tau) / fl(fl(cs(tau) / tau) + FLT_MIN)), tau = min_period + i, i = 0 .. n_lags - 1 = max_period - min_period,
 *               cs(tau) = d(1) + .. + d(tau): lane l of 64 owns the lags l k + 1 .. (l + 1) k (k = ceil(max_period / 64)), a chain inside,
 *               the lanes' totals scanned (Hillis-Steele), cs = fl(before + chain);
 *   shift       0 at i = 0 and i = n_lags - 1, else a = fl(fl(fl(c[i-1] + c[i+1]) - fl(2 c[i])) / 2), b = fl(fl(c[i+1] - c[i-1]) / 2),
 *               shift = fl(-b / fl(fl(2 a) + FLT_MIN)), and 0 unless |shift| <= 1 (a non-finite quotient is 0 here, NaN upstream);
 *   trough      lag i is one iff c[i] < c[i-1] and c[i] <= c[i+1]; lag 0 iff c[0] < c[1]; the last lag iff c[n_lags-1] < c[n_lags-2];
 *   pYIN prior  thresholds th[k] = (k + 1) / 100 and beta[k] = the Beta(2, 18) mass of ((k) / 100, (k + 1) / 100], k = 0 .. 99 (host tables,
 *               fp64).  With the troughs in lag order, trough t of those with c < th[k] at position p of N gets boltz_fact[N] * boltz_exp[p] =
 *               (1 - e^-2) / (1 - e^-2N) * e^-2p; prob[t] = sum over ascending k of fl(fl(fact * exp) * beta[k]) (one fp64 chain; c is
 *               upcast for the compare).  The lowest trough (the first of equals) also gets fl(no_trough_prob * beta_head[m]), m = the
 *               number of thresholds it is not below, beta_head[m] = sum(beta[:m]);
 *   bins        period = (double)(min_period + lag) + (double)shift, bin = clip(rint(bins_per_octave * log2((sr / period) / fmin)), 0,
 *               n_bins); of two troughs in one bin the LATER in lag order is kept (an assignment, not a sum); bin n_bins is dropped (it is
 *               the first unvoiced state upstream and overwritten there); voiced_prob = clip(sum of the bins, 0, 1) (lane chains over bins
 *               lane, lane + 64, .. and a butterfly, fp64) rounded to fp32; log-observations fp64 [2 n_bins]: log(obs + DBL_MIN) (log_floor
 *               = log(DBL_MIN) where obs is 0), every unvoiced state log((1 - voiced_prob) / n_bins + DBL_MIN) with the UNROUNDED sum;
 *   Viterbi     2 n_bins states, the voiced half first.  value_0[s] = fl(logobs_0[s] + linit[s]);  value_t[s] = fl(logobs_t[s] + max_j
 *               cand(j, s)), the FIRST j among equals, with -- the order of the two additions -- cand(j, s) = fl(fl(value[j] + lsrc[2 v +
 *               v'][bj]) + ltri[bs - bj + width / 2]) for |bs - bj| <= width / 2 (v, v' the halves and bj, bs the bins of j and s: j = v n_bins
 *               + bj), and fl(value[j] + log_floor) outside the band: upstream's matrix is dense, log(T + tiny), and a jump out of the band costs
 *               the floor, not infinity.  Host tables in fp64: ltri = log of the triangle window of `width` points, lsrc[2 v + v'][j] =
 *               log(switch[v][v']) - log(the sum of the window's points that fall inside 0 .. n_bins - 1 around j) (transition_local,
 *               no wrap, a normaliser per source row; switch [[.99, .01], [.01, .99]]), linit = log(p_init + tiny), all mass uniform on the
 *               unvoiced half.  The last state is the first of the best; f0 = freqs[state] (the host's fmin 2^(bin / 120), fp32), NaN and
 *               flag 0 in the unvoiced half.  Every step is one rounded fp64 add and an exact compare: the path is bit for bit that of a
 *               NumPy fp64 Viterbi over the same numbers.  backptr is int16 [total_frames, 2 n_bins] of workspace;
 *   plain YIN   the first trough with c < trough_threshold (fp32 compare), else the first global minimum; f0 = fl(sr / fl((float)(min_period
 *               + lag) + shift));
 *   delta       the `delta` line of the MFCC block over any fp32 [total_frames, D], T < 9 -> 0 (the reference applies it to the mel POWER);
 *   statistics  per sentence, fp64 inside (lane chains over frames lane, lane + 64, .. and a butterfly), ONE rounding to fp32 (bf16: one more
 *               of that fp32): columns 0 .. 5 = mean and population std of f0 over its non-NaN frames (0, 0 without one), of the pause
 *               lengths and of the voiced intensities of get_pause_durations: a pause is a run of voiced_prob < 0.5 (fp32 compare) CLOSED
 *               by a frame that is not; without a closed run the list is [the number of pause frames] and, when that is not 0, a 0 joins
 *               the voiced intensities.  Column jump_col = pitch_jump: 0 where doc_first[s] != 0 or s = 0 (upstream resets the previous
 *               track per document), else nanmean(f0[: T / 5] / nanmean(f0)) - nanmean(q[Tp - ceil(Tp / 5) :] / nanmean(q)), q the
 *               previous sentence's frames of prev_f0 (the plain-YIN track), NaN -> 0 (a sentence without a voiced frame gives 0).
 * All run on the caller's stream, use no atomics and no dependence between workgroups of one launch, write every output element exactly
 * once and give the same bits for the same inputs.  MTS_ERR_INVALID before any device work: a null pointer, an unknown out_dtype, a size
 * < 1, frame_length odd or outside 16 .. 4096, win_length no multiple of 8, periods outside 1 <= min_period, min_period + 2 <= max_period
 * <= frame_length - win_length - 1, n_lags < 3, Boltzmann tables shorter than n_lags / 2 + 2, an even width, a log_floor >= 0, jump_col < 6
 * or >= ld_out, a misaligned pointer.  MTS_ERR_UNSUPPORTED: more than 1024 states, tables beyond a workgroup's 64 KiB of LDS, more frames
 * than one launch covers. */
int mts_yin_frames(void* stream, int n_sent, int frame_length, int win_length, int hop, int min_period, int max_period,
                   const float* wave,           /* device [total_samples] */
                   int64_t total_samples,
                   const int64_t* sent_start,   /* device [n_sent] */
                   const int64_t* sent_len,     /* device [n_sent] */
                   const int64_t* frame_start,  /* device [n_sent + 1], ascending */
                   int64_t total_frames,
                   float* cmnd,                 /* device [total_frames, max_period - min_period + 1] out */
                   float* shift);               /* device, the same shape, out */
int mts_pyin_observe(void* stream, int64_t total_frames, int n_lags, int min_period, int n_bins, double sr, double fmin,
                     double bins_per_octave,
                     const float* cmnd,         /* device [total_frames, n_lags] */
                     const float* shift,        /* device [total_frames, n_lags] */
                     const double* thresholds,  /* device [n_thresholds], ascending */
                     const double* beta,        /* device [n_thresholds] */
                     const double* beta_head,   /* device [n_thresholds + 1] */
                     int n_thresholds,
                     const double* boltz_fact,  /* device [n_boltz] */
                     const double* boltz_exp,   /* device [n_boltz] */
                     int n_boltz, double no_trough_prob, double log_floor,
                     float* voiced_prob,        /* device [total_frames] out */
                     double* logobs);           /* device [total_frames, 2 n_bins] out */
int mts_pyin_viterbi(void* stream, int n_sent, int n_bins, int width,
                     const double* logobs,      /* device [total_frames, 2 n_bins] */
                     int64_t total_frames,
                     const int64_t* frame_start,/* device [n_sent + 1], ascending */
                     const double* ltri,        /* device [width] */
                     const double* lsrc,        /* device [4, n_bins] */
                     const double* linit,       /* device [2 n_bins] */
                     double log_floor,
                     const float* freqs,        /* device [n_bins] */
                     int16_t* backptr,          /* device [total_frames, 2 n_bins] workspace */
                     int32_t* state,            /* device [total_frames] out */
                     float* f0,                 /* device [total_frames] out */
                     uint8_t* voiced);          /* device [total_frames] out */
int mts_yin_pick(void* stream, int64_t total_frames, int n_lags, int min_period, float sr, float trough_threshold,
                 const float* cmnd, const float* shift, /* device [total_frames, n_lags] */
                 float* f0);                    /* device [total_frames] out */
int mts_frame_delta(void* stream, int n_sent, int D,
                    const float* x,             /* device [total_frames, D] */
                    int64_t total_frames,
                    const int64_t* frame_start, /* device [n_sent + 1], ascending */
                    float* out);                /* device [total_frames, D] out */
int mts_prosodic_stats(void* stream, int out_dtype, int n_sent,
                       const float* f0,         /* device [total_frames]: the pYIN track, NaN where unvoiced */
                       const float* voiced_prob,/* device [total_frames] */
                       const float* prev_f0,    /* device [total_frames]: the plain-YIN track */
                       int64_t total_frames,
                       const int64_t* frame_start, /* device [n_sent + 1], ascending */
                       const uint8_t* doc_first,/* device [n_sent]: 1 on the first sentence of a document */
                       void* out,               /* device: row s at out + s * ld_out; columns 0 .. 5 and jump_col written */
                       int64_t ld_out, int jump_col);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm family (biased variance, eps inside sqrt).
 * Replaces: LongformerEmbeddings (modeling_longformer.py:402-426: x + pos_emb[2+i] + type_emb[0] -> LN),
 * LongformerSelfOutput / LongformerOutput LayerNorm (:1068-1072, :1127-1131) and their backward.
 * ------------------------------------------------------------------------------------------- */
/* y[b,i,:] = LN(x[b,i,:] + pos[pos_offset+i,:] + type0[:]); x fp32 [B*L, D] (the batch as the collater made it);
 * pre (act dtype, optional) receives the pre-LN sum for the backward; mean/rstd fp32 [B*L]. */
int mts_embed_layernorm_fwd(void* stream, int dtype, int B, int L, int D, const float* x, const float* pos,
                            int pos_offset, const float* type0, const float* gamma, const float* beta, float eps,
                            void* y, void* pre, float* mean, float* rstd, const int32_t* row_src, int n_rows);
/* ... on a batch that arrived in bf16 (x_bf16: bf16 [B, L, D]; bf16 activations; one source): the same bits as mts_embed_layernorm_fwd on the fp32
 * values of the same numbers, without an fp32 copy of the batch (prefetch.DevicePrefetcher / AudioPortionDataset(wire_dtype='bf16')). */
int mts_embed_layernorm_fwd_x16(void* stream, int B, int L, int D, const void* x_bf16, const float* pos, int pos_offset, const float* type0,
                                const float* gamma, const float* beta, float eps, void* y, void* pre, float* mean, float* rstd,
                                const int32_t* row_src, int n_rows);
/* ... and the same embedding + LayerNorm as mts_embed_layernorm_fwd on x = x1[b,i,0:D1] | x2[b,i,0:D2] (D = D1 + D2). */
int mts_embed_layernorm_fwd2(void* stream, int dtype, int B, int L, int D1, int D2, const float* x1, const float* x2, const float* pos,
                             int pos_offset, const float* type0, const float* gamma, const float* beta, float eps,
                             void* y, void* pre, float* mean, float* rstd, const int32_t* row_src, int n_rows);
/* If head_w != NULL the tagger head is fused in: scores[r,c] = y[r,:].head_w[c,:] + head_b[c] (fp32 [rows,n_out],
 * n_out <= 4), computed on the stored (act dtype) y.  models/CRF.py:579 on top of modeling_longformer.py:1127-1131.
 * With a fused head and mean/rstd given, y may be NULL: the row is normalised, rounded to the act dtype and fed to the head, but
 * not written (training step of the last layer: mts_layernorm_bwd recomputes it, see dhead_w there). */
int mts_layernorm_fwd(void* stream, int dtype, int rows, int D, const void* x, const float* gamma,
                      const float* beta, float eps, void* y, float* mean, float* rstd,
                      const float* head_w, const float* head_b, int n_out, float* scores);
/* dx = LN'(x) dy ; dgamma/dbeta (fp32 [D]) are OVERWRITTEN with the column reductions; dxsum (optional,
 * fp32 [D]) receives colsum(dx) = the bias gradient of the linear layer that produced x.
 * If head_w != NULL the incoming gradient is dy[r,:] (if non-null) + sum_c dlogit[r,c]*head_w[c,:]
 * (the tagger head's data gradient fused in; n_out columns).
 * If additionally dhead_w != NULL (needs beta, dhead_b, n_out <= 2) the head's PARAMETER gradients are produced in the same pass:
 * dhead_w[c,:] = sum_r dlogit[r,c] * y[r,:], dhead_b[c] = sum_r dlogit[r,c] (OVERWRITE; models/CRF.py:579's nn.Linear), with
 * y[r,:] = LN(x[r,:]) recomputed from the saved statistics exactly as the forward rounded it -- the forward of that layer did not
 * have to store y and no separate mts_head_bwd_params pass reads it.  beta / dhead_w / dhead_b may be NULL together.
 * partial: fp32 workspace of mts_layernorm_bwd_workspace(D) bytes. */
size_t mts_layernorm_bwd_workspace(int D);
int mts_layernorm_bwd(void* stream, int dtype, int rows, int D, const void* x, const void* dy,
                      const float* dlogit, const float* head_w, int n_out,
                      const float* gamma, const float* mean, const float* rstd,
                      void* dx, float* dgamma, float* dbeta, float* dxsum, void* partial,
                      const float* beta, float* dhead_w, float* dhead_b);
/* THE LAST LAYER'S TAIL IN ONE PASS (training): LayerNorm forward + tagger head + masked loss + loss gradient + head data gradient + LayerNorm
 * backward of x = the layer's pre-LayerNorm sum s2 [rows, D], row by row -- what mts_layernorm_fwd(head) + mts_tagger_loss (+ mts_scale) +
 * mts_layernorm_bwd(head, dhead_w) do in four launches and two reads of x.  (modeling_longformer.py:1127-1131, models/CRF.py:579-595,
 * focal_loss.py:38-57 and their backward.)  scores fp32 [rows, n_out]; loss_out fp32 [2] = {loss, rows averaged}; dx act dtype [rows, D];
 * dgamma / dbeta / dxsum (may be NULL) fp32 [D]; dhead_w fp32 [n_out, D], dhead_b [n_out] (all OVERWRITTEN).  Batch description as
 * mts_tagger_loss (targets fp32 [B, Lt], lengths, packed rows through row_src / n_rows); grad_scale multiplies d loss / d scores.
 * n_out = 1 (BCE / focal) or 2 (CrossEntropy); D in {256, 512, 1024, 1792, 2048}: mts_layernorm_loss_tail_supported.  Scores and gradients are
 * bitwise those of the four launches; the loss differs by the grouping of its partial sums.  workspace: mts_layernorm_bwd_workspace(D) bytes. */
int mts_layernorm_loss_tail_supported(int dtype, int D, int n_out);
int mts_layernorm_loss_tail(void* stream, int dtype, int rows, int D, const void* x, const float* gamma, const float* beta, float eps,
                            const float* head_w, const float* head_b, int n_out, int loss_kind, int B, int L, int Lt, const float* targets,
                            const int32_t* lengths, float alpha, float gamma_focal, float grad_scale, const int32_t* row_src, int n_rows,
                            float* scores, float* loss_out, void* dx, float* dgamma, float* dbeta, float* dxsum, float* dhead_w,
                            float* dhead_b, void* workspace);
/* Backward of the embedding block in ONE pass (modeling_longformer.py:402-426: LN(x + pos[2+i] + type0)): dh (act dtype [rows, D]) is
 * the gradient at the LayerNorm's output, pre / mean / rstd what mts_embed_layernorm_fwd saved.  OVERWRITES dgamma, dbeta, dtype0
 * (= sum over all rows of the pre-LN gradient: the token-type row 0) and rows pos_offset .. pos_offset+L-1 of dpos (= the sum over the
 * documents of each position; positions no document reaches get 0).  The pre-LN gradient itself is never written to memory.
 * row0 / lengths / n_rows: packed batches (below), else NULL / NULL / 0.  D <= 2048. */
size_t mts_embed_layernorm_bwd_workspace(int B, int L, int D);
int mts_embed_layernorm_bwd(void* stream, int dtype, int B, int L, int D, const void* pre, const void* dh, const float* gamma,
                            const float* mean, const float* rstd, float* dgamma, float* dbeta, float* dtype0, float* dpos,
                            int pos_offset, const int32_t* row0, const int32_t* lengths, int n_rows, void* workspace, size_t workspace_bytes);
/* gradient of the position table from a STORED pre-LN gradient: dpos[pos_offset+i,:] += sum_b dpre[b,i,:].  (The token-type row's
 * gradient is sum_{b,i} dpre = the `dxsum` output of the embedding LayerNorm's mts_layernorm_bwd.)  Kept for D > 2048. */
int mts_embed_bwd(void* stream, int dtype, int B, int L, int D, const void* dpre, float* dpos, int pos_offset,
                  const int32_t* row0, const int32_t* lengths);

/* Inverted dropout: y = keep ? x / (1-p) : 0 (+ residual, if given), keep decided by a counter-based hash of (seed, element index)
 * (F.dropout in RNN.forward, NeuralArchitectures.py:94,119 -- active even in eval mode there; nn.Dropout of the HF layers,
 * modeling_longformer.py:424,1070,1129).  mask (optional, uint8 [n]) records keep = 1; x == y is allowed; n % 4 == 0.
 * mts_dropout_bwd: dx = mask ? dy / (1-p) : 0 (dx == dy allowed).
 * The kernels move 4 elements per access: x, residual, y, dy and dx must be aligned to 4 elements (16 bytes of fp32, 8 of bf16) and
 * mask to 4 bytes.  A pointer off its boundary, n % 4 != 0, p outside [0, 1), a bad dtype or a null operand (the backward needs its
 * mask) is MTS_ERR_INVALID before any launch; there is no scalar fallback. */
int mts_dropout_fwd(void* stream, int dtype, size_t n, const void* x, const void* residual, void* y, uint8_t* mask,
                    float p, uint64_t seed);
int mts_dropout_bwd(void* stream, int dtype, size_t n, const void* dy, void* dx, const uint8_t* mask, float p);

/* dy *= gelu_erf'(u) in place (FFN backward; modeling_longformer.py:1113-1116); n elements, n % 4 == 0 */
int mts_gelu_bwd(void* stream, int dtype, size_t n, const void* u, void* dy);
/* dy *= (u > 0) in place (backward of the legacy layer's ReLU, models/RestrictedTransformerLayer.py:308); n % 4 == 0 */
int mts_relu_bwd(void* stream, int dtype, size_t n, const void* u, void* dy);

/* ---------------------------------------------------------------------------------------------
 * Fused feed-forward block (hidden width F = 256, D a multiple of 256, bf16): LongformerIntermediate + LongformerOutput.dense +
 * residual (modeling_longformer.py:1113-1131) in one launch, and the data gradient of the same block in one launch.
 *   forward : u = a1 W1^T + b1 ; f = gelu_erf(u) (relu != 0: max(u, 0)) ; s2 = f W2^T + b2 + a1
 *   backward: du = (ds2 W2) * act'(u) ; da1 = du W1 + ds2        (weight / bias gradients: mts_gemm TN, mts_colsum on du)
 * a1, ds2 [M, D]; w1 [F, D]; w2 [D, F] (bf16 mirrors); b1 [F], b2 [D] fp32; u, f, du [., F]; s2, da1 [., D].  OUTPUT buffers must
 * have room for ceil(M / 64) * 64 rows (rows past M are written, not masked).  Bitwise the results of the two-GEMM path.
 * mts_ffn_supported: 1 when the fused block covers (dtype, M, D, F), else the caller uses mts_gemm.
 * ------------------------------------------------------------------------------------------- */
int mts_ffn_supported(int dtype, int M, int D, int F);
int mts_ffn_fwd(void* stream, int M, int D, int F, const void* a1, const void* w1, const float* b1, const void* w2, const float* b2,
                int relu, void* u, void* f, void* s2);
int mts_ffn_bwd_data(void* stream, int M, int D, int F, const void* ds2, const void* w1, const void* w2, const void* u, int relu,
                     void* du, void* da1);

/* ---------------------------------------------------------------------------------------------
 * PACKED BATCHES (training path; the reference pads every Transformer batch to 3600 sentences, train_fit.py:104-106,
 * and runs all of them through the encoder).  Activations may hold only the valid sentences, document after document:
 * n_rows = sum of lengths; `row_src[r]` = b*L + i names the sentence of the padded batch that packed row r holds
 * (mts_embed_layernorm_fwd gathers x and the position, mts_tagger_loss finds the target); `row0[b]` = first packed row of
 * document b (band attention, mts_embed_bwd).  All four are NULL for the padded [B, L] layout.  Padded rows never
 * influence valid rows or any gradient (masked as keys, excluded from the loss), so results on valid rows are the same.
 * ------------------------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------------------------
 * Restricted-window (band) self-attention.
 * Replaces: LongformerSelfAttention.forward local path (modeling_longformer.py:482-640:
 * _sliding_chunks_query_key_matmul :759-823, padding mask :524-536, softmax fp32 :574-576, masked
 * query rows zeroed :579, _sliding_chunks_matmul_attn_probs_value :825-867) and, equivalently, the
 * legacy per-position loop models/RestrictedTransformerLayer.py:509-636; plus the backward.
 * qkv: [B*L, 3*D] act dtype, row = [q(D) | k(D) | v(D)], q already scaled; head h owns columns
 * h*hd..(h+1)*hd of each third.  lengths: int32 [B] (NULL = all L).  ctx: [B*L, D].
 * probs: fp32 [B*L, heads, slots] with slots = mts_band_slots(radius), saved for the backward.
 * drop_p > 0: dropout on the attention probabilities (modeling_longformer.py:590; HF attention_probs_dropout_prob = the reference's
 * dropout_out): what multiplies V is keep ? p / (1 - drop_p) : 0 with keep = hash(drop_seed, (row, head, slot)); `probs` stays whole
 * and the backward, given the same drop_p / drop_seed, regenerates the mask.
 * ------------------------------------------------------------------------------------------- */
int mts_band_slots(int radius);
int mts_band_attn_fwd(void* stream, int dtype, int B, int L, int D, int heads, int radius,
                      const void* qkv, const int32_t* lengths, void* ctx, float* probs, const int32_t* row0,
                      float drop_p, uint64_t drop_seed);
/* dqkv [B*L, 3D] (dq already multiplied by q_scale so it is the gradient wrt the unscaled projection);
 * dscores: fp32 scratch of the same size as probs (the one-pass bf16 kernel leaves it untouched: dS stays on the chip).  dbias (optional): fp32 [3D] column sums of dqkv as stored =
 * the gradient of the q/k/v biases (modeling_longformer.py:504-506), produced from the kernels' output tiles instead of
 * re-reading dqkv; needs `workspace` of mts_band_attn_bwd_workspace(B, L, D) bytes.  Bitwise reproducible. */
size_t mts_band_attn_bwd_workspace(int B, int L, int D);
int mts_band_attn_bwd(void* stream, int dtype, int B, int L, int D, int heads, int radius, float q_scale,
                      const void* qkv, const int32_t* lengths, const float* probs, const void* dctx,
                      void* dqkv, float* dscores, float* dbias, void* workspace, const int32_t* row0, int n_rows,
                      float drop_p, uint64_t drop_seed);

/* ---------------------------------------------------------------------------------------------
 * Full self-attention (every valid key of the document).
 * Replaces: BertSelfAttention of the BertModel inside Classic_Transformer (models/RestrictedTransformerLayer.py:16-63, used by
 * Transformer_segmenter(restricted=False), models/CRF.py:543-549); plus the backward.
 * Operands as for the band kernels: qkv [rows, 3D] act dtype with q already scaled, lengths int32 [B] (NULL = all L; every
 * lengths[b] >= 1), row0 (optional) = packed rows, ctx [rows, D].  Query i of document b attends to keys j < len_b: padded keys get
 * probability exactly 0 (their tiles are never visited); padded query rows of the [B, L] layout are NOT zeroed -- they attend to the
 * document's valid keys like any other row (BERT has no masked-row step).
 * lse: fp32 [rows, heads] = log sum_j exp(s_ij), saved by the forward; the backward recomputes P = exp(S - lse) from q, k and lse,
 * and takes delta = rowsum(dCtx o ctx) from the saved ctx.  Nothing [L, L] is ever stored.
 * drop_p > 0: dropout on the attention probabilities (BERT's attention_probs_dropout_prob): what multiplies V is
 * keep ? p / (1 - drop_p) : 0 with
 *     keep = mts_hash32(drop_seed, ((uint64_t)grow * heads + h) * L + j) >= (uint32_t)max(1, min(2^32 - 1, drop_p * 2^32))
 * grow = the activation row of the query (packed or not), L = the batch's padded length, j = the key's position in its document
 * (mts_hash32: csrc/common.h, splitmix64 finaliser, high 32 bits).  The backward, given the same drop_p / drop_seed, regenerates it.
 * Head dims: multiples of 4 (fp32) / 8 (bf16) up to 512 whose staged tiles fit 160 KiB of LDS (fp32: up to 292; bf16: up to 512);
 * anything else is MTS_ERR_UNSUPPORTED before any launch.  bf16 with head dim % 32 == 0 and <= 256 runs on matrix-core kernels
 * (v_mfma_f32_16x16x32_bf16); mts_set_option("full_mfma", 0) sends it to the generic kernels, which serve every other shape.
 * mts_full_attn_bwd: dqkv [rows, 3D] (dq multiplied by q_scale); dbias (optional) fp32 [3D] = column sums of dqkv;
 * workspace (REQUIRED) of mts_full_attn_bwd_workspace(B, L, D, heads) bytes.  Two kernels (dQ per query tile, dK/dV per key tile),
 * no atomics: bitwise reproducible.
 * ------------------------------------------------------------------------------------------- */
int mts_full_attn_fwd(void* stream, int dtype, int B, int L, int D, int heads, const void* qkv, const int32_t* lengths,
                      void* ctx, float* lse, const int32_t* row0, float drop_p, uint64_t drop_seed);
size_t mts_full_attn_bwd_workspace(int B, int L, int D, int heads);
int mts_full_attn_bwd(void* stream, int dtype, int B, int L, int D, int heads, float q_scale, const void* qkv,
                      const int32_t* lengths, const float* lse, const void* ctx, const void* dctx, void* dqkv, float* dbias,
                      void* workspace, const int32_t* row0, int n_rows, float drop_p, uint64_t drop_seed);

/* ---------------------------------------------------------------------------------------------
 * LongT5 local self-attention with a learned, bucketed relative-position bias.
 * Replaces: LongT5LocalAttention of the LongT5EncoderModel inside RecurrentLongT5 (models/CRF.py:613-762,
 * models/RestrictedTransformerLayer.py:135-187; HF modeling_longt5.py); plus the backward.
 * Padded [B, L] layout only.  qkv [B*L, 3*inner] act dtype (columns q | k | v, inner = heads * head_dim, NO 1/sqrt(d) scaling);
 * lengths int32 [B] (NULL = all L; every lengths[b] >= 1); radius r >= 1 (one-sided); table fp32 [buckets, heads] =
 * relative_attention_bias.weight; bucket_of_offset int32 [2r + 1]: entry r + (j - i) is the bucket of offset j - i, each in
 * [0, buckets) (the caller computes it once with the reference's own _relative_position_bucket; kernels never take the log).
 * ctx [B*L, inner] act dtype.  Per head, s_ij = q_i . k_j + table[bucket_of_offset[r + j - i], h].
 *   valid query rows i < len_b: softmax over keys j in [i - r, i + r] with 0 <= j < len_b;
 *   padded query rows len_b <= i < L: every key is masked with -1e10 in the reference, which absorbs the scores in fp32, so the row
 *   is the uniform mean sum_j v_j / (3 (r + 1)) over j in [(floor(i/(r+1)) - 1)(r+1), (floor(i/(r+1)) + 2)(r+1)) and 0 <= j < L
 *   (padded v rows included; the reference departs from this only when a padded row's |score| reaches 512).
 * lse: fp32 [B*L, heads] = log sum_j exp(s_ij) of valid rows (0 on padded rows), saved by the forward; the backward recomputes
 * P = exp(S - lse) and takes delta = rowsum(dCtx o ctx) from the saved ctx.  Nothing [L, L] or [L, 2r+1] is ever stored.
 * drop_p > 0: dropout on the probabilities of valid rows (training mode; padded rows are never dropped): what multiplies V is
 * keep ? p / (1 - drop_p) : 0 with
 *     keep = mts_hash32(drop_seed, ((uint64_t)(b * L + i) * heads + h) * (2r + 1) + (r + j - i)) >= (uint32_t)max(1, min(2^32 - 1, drop_p * 2^32))
 * (mts_hash32: csrc/common.h).  The backward, given the same drop_p / drop_seed, regenerates it.
 * mts_t5_local_attn_bwd: dqkv [B*L, 3*inner] act dtype, every row written: padded query rows carry no gradient (they never reach a
 * valid row or the loss) -- their dq is 0 and their dctx is NOT read; dk = dv = 0 for padded keys.  dtable fp32 [buckets, heads]
 * OVERWRITTEN: per-workgroup sums of dS per (head, offset) go to the workspace, one kernel sums them per (head, offset) in a fixed
 * order, another adds the offsets of each bucket in ascending offset; buckets no offset maps to get exactly 0.  workspace (REQUIRED)
 * of mts_t5_local_attn_bwd_workspace(B, L, heads, radius) bytes.  No atomics: bitwise reproducible.
 * Covered: head_dim 64 (LongT5's d_kv), radius <= 1024, fp32 and bf16; qkv, ctx, dctx and dqkv 16-byte aligned (rows are 16-byte
 * vectors); anything else is MTS_ERR_UNSUPPORTED before any launch.  bf16 runs on matrix-core kernels (v_mfma_f32_16x16x32_bf16);
 * mts_set_option("t5_mfma", 0) sends it to the generic kernels (v_dot2_f32_bf16), which also serve fp32.
 * ------------------------------------------------------------------------------------------- */
int mts_t5_local_attn_fwd(void* stream, int dtype, int B, int L, int heads, int head_dim, int radius, const void* qkv,
                          const int32_t* lengths, const float* table, int buckets, const int32_t* bucket_of_offset, void* ctx,
                          float* lse, float drop_p, uint64_t drop_seed);
size_t mts_t5_local_attn_bwd_workspace(int B, int L, int heads, int radius);
int mts_t5_local_attn_bwd(void* stream, int dtype, int B, int L, int heads, int head_dim, int radius, const void* qkv,
                          const int32_t* lengths, const float* table, int buckets, const int32_t* bucket_of_offset,
                          const float* lse, const void* ctx, const void* dctx, void* dqkv, float* dtable, void* workspace,
                          float drop_p, uint64_t drop_seed);

/* ---------------------------------------------------------------------------------------------
 * RMSNorm (T5LayerNorm: no mean subtraction, no bias).  Replaces the layer_norm / final_layer_norm of LongT5 (HF modeling_longt5.py
 * LongT5LayerNorm) inside RecurrentLongT5, and its backward.
 * x, y [rows, D] act dtype; w fp32 [D]; y = w * (x * rstd), rstd = 1 / sqrt(mean(x^2) + eps) computed in fp32; rstd fp32 [rows]
 * (saved for the backward; may be NULL in the forward).  D a multiple of 4, <= 2048; activations aligned to 4 elements (16 B fp32,
 * 8 B bf16) and w to 16 bytes (else MTS_ERR_UNSUPPORTED).
 * mts_rmsnorm_bwd: dx = rstd (dy w - n mean(dy w . n)) (+ dres), n = x rstd; dres (optional, act dtype [rows, D]) is the residual
 * branch's gradient, and dx may alias it (not x or dy).  dw fp32 [D] = sum_rows dy n, OVERWRITTEN: per-workgroup partial rows in the
 * workspace (mts_rmsnorm_bwd_workspace(rows, D) bytes, REQUIRED), then one fixed-order reduce (as mts_layernorm_bwd): bitwise
 * reproducible.
 * ------------------------------------------------------------------------------------------- */
int mts_rmsnorm_fwd(void* stream, int dtype, int rows, int D, const void* x, const float* w, float eps, void* y, float* rstd);
size_t mts_rmsnorm_bwd_workspace(int rows, int D);
int mts_rmsnorm_bwd(void* stream, int dtype, int rows, int D, const void* x, const void* dy, const void* dres, const float* w,
                    const float* rstd, void* dx, float* dw, void* workspace);

/* ---------------------------------------------------------------------------------------------
 * Adjacent-pair bilinear score.  Replaces the tail of SheikhBiLSTM (models/CRF.py:1009-1014 in loss, :1029-1035 in forward):
 * (x_for[:, :-1] * x_bac[:, 1:]).sum(2) and the appended step of ones.
 * F, G: [B*L, H] act dtype with leading dimensions ldf, ldg in ELEMENTS (they may be the two halves of one [B*L, 2H] buffer);
 * scores, dscores: fp32 [B, L].
 * forward: scores[b, t] = sum_h F[bL + t, h] G[bL + t + 1, h] for t < L - 1 (fp32 accumulation), scores[b, L - 1] = 1.0f exactly; a
 * pair never crosses a document.
 * backward: dF[b, t, :] = dscores[b, t] G[b, t + 1, :] (exactly 0 at t = L - 1), dG[b, t, :] = dscores[b, t - 1] F[b, t - 1, :]
 * (exactly 0 at t = 0); every row of dF and dG is OVERWRITTEN, dscores[b, L - 1] is never read; no atomics, bitwise reproducible.
 * Covered: H a multiple of 8 (bf16) / 4 (fp32); F, G, dF, dG and their leading dimensions 16-byte aligned; anything else is
 * MTS_ERR_UNSUPPORTED before any launch.  B * L == 0 returns MTS_OK without a launch; L == 1 is valid (all scores 1, dF = dG = 0).
 * ------------------------------------------------------------------------------------------- */
int mts_pair_score_fwd(void* stream, int dtype, int B, int L, int H, const void* F, int ldf, const void* G, int ldg, float* scores);
int mts_pair_score_bwd(void* stream, int dtype, int B, int L, int H, const void* F, int ldf, const void* G, int ldg,
                       const float* dscores, void* dF, int lddf, void* dG, int lddg);

/* ---------------------------------------------------------------------------------------------
 * Gated merge of two encoder outputs: BiLSTMLateFusion(merge='gate').  An extension: the reference concatenates (models/CRF.py:425, :469)
 * and has no gate, so DESIGN.md "Gated late-fusion merge" is the specification.
 * a, h1, h2, m, dm, da, dh1, dh2: [rows, W] act dtype with leading dimensions in ELEMENTS; a = the gate's pre-activation.
 * forward:  z = sigmoid(a) = 1 / (1 + expf(-a));  m = z h1 + (1 - z) h2  (= h2 + z (h1 - h2)).
 * backward: dh1 = dm z;  dh2 = dm - dm z;  da = dm (h1 - h2) z (1 - z);  z is recomputed from a.  The caller adds da W_g to dh1 / dh2.
 * fp32 arithmetic, every output rounded once and OVERWRITTEN; outputs may not overlap the inputs or each other.  Saturation is exact:
 * a = +-1e4 gives z = 1 | 0, m = h1 | h2 bit for bit and da = 0; a finite input never gives a NaN or an Inf.
 * Streaming: 16-byte accesses when W, every leading dimension and every base allow (fp32: always; bf16: multiples of 8 elements and
 * 16-byte bases), 4-element accesses otherwise; no atomics, no workspace, no LDS, one launch, 64-bit offsets; bitwise reproducible.
 * MTS_ERR_INVALID before any device work: unknown dtype; W < 1; W or a leading dimension no multiple of 4; a leading dimension below
 * W; a base not aligned to a 4-element vector (16 bytes in fp32, 8 in bf16); with rows > 0 a null operand.  rows == 0: MTS_OK, no launch.
 * ------------------------------------------------------------------------------------------- */
int mts_gate_merge_fwd(void* stream, int dtype, size_t rows, int W, const void* a, int lda, const void* h1, int ldh1, const void* h2,
                       int ldh2, void* m, int ldm);
int mts_gate_merge_bwd(void* stream, int dtype, size_t rows, int W, const void* a, int lda, const void* h1, int ldh1, const void* h2,
                       int ldh2, const void* dm, int lddm, void* da, int ldda, void* dh1, int lddh1, void* dh2, int lddh2);

/* ---------------------------------------------------------------------------------------------
 * Cosine auxiliary segment loss.  Replaces cosine_loss / aggregate_embeddings + nn.CosineEmbeddingLoss() of the `segments=` branch of
 * BiLSTM.loss and BiLSTMLateFusion.loss (models/CRF.py:23-92, :322-337, :427-442).
 * x, dx: [B*L, W] act dtype with leading dimensions in ELEMENTS (late fusion hands in a view).  int32 device tables, built on the host
 * from the batch's segment lists:
 *   seg_table  [n_seg, 8]:  {document, begin row, end row, tail flag, positive pair, negative pair with this segment as FIRST member,
 *                           negative pair with it as SECOND member, 0}; rows are relative to the document, pair entries are -1 for "none".
 *                           A document's listed segments and its tail (end of the last listed segment .. length; may be empty) are adjacent.
 *   pair_table [n_pair, 4]: {segment a, segment b, target +1 | -1, 0}.  target +1: (even rows of a, odd rows of a), a == b;
 *                           target -1: (all rows of a, all rows of b).
 *   row_map    [B*L]:       2 * segment + parity of the row inside its segment, or -1 for a row in no segment.
 * forward:  cos_p = a.b / sqrt((|a|^2 + 1e-12)(|b|^2 + 1e-12)) from fp32 row sums; term_p = 1 - cos_p (target +1) | max(cos_p, 0) (target -1);
 *           loss_out fp32 [2] = {mean of the terms, n_pair}; pair_cos (fp32 [n_pair], may be NULL) receives every cos_p.  x is read once.
 *           n_pair == 0 writes {0, 0} and launches nothing.
 * backward: dx[r, :] (+)= scale * d(sum of the terms)/dx[r, :]  (the caller folds 1 / n_pair into scale; the clamp passes the gradient
 *           where cos >= 0).  accumulate = 1 adds into dx and leaves rows in no segment alone, accumulate = 0 overwrites every row, rows in no
 *           segment with zeros.  Needs the workspace of the forward call untouched.  Gather form, no atomics: bitwise reproducible.
 * workspace: mts_segment_cosine_workspace(n_seg, n_pair, W) bytes, 16-byte aligned: fp32 row sums and gradient vectors per segment
 *           and parity, four statistics per pair.
 * A table entry outside its range contributes nothing and no address is formed from it.
 * Covered: W a multiple of 8 (bf16) / 4 (fp32); x, dx, their leading dimensions and the workspace 16-byte aligned; anything else is
 * MTS_ERR_UNSUPPORTED before any launch.
 * ------------------------------------------------------------------------------------------- */
size_t mts_segment_cosine_workspace(int n_seg, int n_pair, int W);
int mts_segment_cosine_fwd(void* stream, int dtype, int B, int L, int W, const void* x, int ldx, int n_seg, const int32_t* seg_table,
                           int n_pair, const int32_t* pair_table, float* loss_out, float* pair_cos, void* workspace);
int mts_segment_cosine_bwd(void* stream, int dtype, int B, int L, int W, int n_seg, const int32_t* seg_table, int n_pair,
                           const int32_t* pair_table, const int32_t* row_map, float scale, int accumulate, void* dx, int lddx,
                           void* workspace);

/* ---------------------------------------------------------------------------------------------
 * Tagger head tail: loss + its gradient, and greedy decode.
 * Replaces: the un-pad loop + BCE/Focal/CE of models/CRF.py:342-356 (=:447-461, :581-595),
 * models/focal_loss.py:38-57, and decode models/CRF.py:362-369.
 * scores: fp32 [B, L, n_out] (n_out = 1 for BCE / focal, 2..4 = tagset_size for CrossEntropy); targets: fp32 [B, Lt] (pad -1 / 0 as
 * the collater wrote them), Lt >= L; lengths int32 [B].  loss_out: fp32 [2] = {loss, number of rows averaged}.  dscores may be NULL.
 * workspace: mts_tagger_loss_workspace(B, L) bytes of device scratch for the per-workgroup partial sums
 * (NULL = single-workgroup path; same result up to fp32 summation order).
 * ------------------------------------------------------------------------------------------- */
size_t mts_tagger_loss_workspace(int B, int L);
int mts_tagger_loss(void* stream, int loss_kind, int B, int L, int Lt, int n_out, const float* scores,
                    const float* targets, const int32_t* lengths, float alpha, float gamma,
                    float* loss_out, float* dscores, void* workspace, size_t workspace_bytes,
                    const int32_t* row_src, int n_rows);
/* tags_out: uint8 [B, L]; positions >= length are 0.  prob > threshold, strict; prob = sigmoid (n_out 1) or softmax[..., 1] (n_out 2..4). */
int mts_greedy_decode(void* stream, int B, int L, int n_out, const float* scores, const int32_t* lengths,
                      float threshold, uint8_t* tags_out);
/* PREDICTION PASS: SEGMENT TABLES AND A MINIMUM-LENGTH DECODE (predict.py; csrc/segment_decode.hip).  Replaces what a caller of the
 * reference's predict.py does on the host after the forward -- tag lists per document, then a loop per list -- and adds a decode under a
 * minimum segment length (an extension: upstream has none, and no claim about Pk is made for it).  scores fp32 [B, L, n_out], n_out 1..4;
 * lengths int32 [B], NULL = every document has L sentences (clamped to 0..L).  For document b of n sentences, in ONE launch:
 *   p_i = the probability of mts_greedy_decode, same bits;  prob[b, i] = p_i for i < n and 0 behind (prob may be NULL)
 *   min_segment == 1:   tag_i = p_i > threshold, strict: bit for bit what mts_greedy_decode writes, at any threshold
 *   min_segment = m >= 2, exact in integers:  P_i = rint((double) p_i * 2^32),  T = rint((double) threshold * 2^32) as int64, half to
 *     even;  q_i = P_i - T.  The last sentence keeps the greedy rule, tag_{n-1} = p_{n-1} > threshold (it ends the document either
 *     way).  Interior boundaries are eligible at t in [m-1, n-1-m] only, so the first and the last segment hold at least m sentences
 *     too; n < 2m gives none.  With best(u) = 0 for u < m-1 and t ascending:
 *         cand_t = q_t + best(t - m);   take_t = cand_t > best(t - 1), strict;   best(t) = max(best(t - 1), cand_t)
 *     and the walk back from t = n-1-m: down to the largest u <= t with take_u, tag_u = 1, continue at t = u - m.  This maximises
 *     sum_{t in S} (p_t - threshold) over the admissible boundary sets S (any two boundaries at least m apart), the minimum-expected-cost
 *     decode whose m = 1 case is the threshold rule: for thresholds in [2^-8, 1) T is exact and q_t > 0 iff p_t > threshold.  The rule
 *     is these integers, not a mapping onto threads: any parallelisation gives the same bits.  threshold must lie in [-1024, 1024].
 *   tags[b, i] (uint8, may be NULL) = tag_i for i < n, 0 behind
 *   seg_end[b, j] = the position BEHIND the j-th sentence with tag 1 (an exclusive end), ascending; with close_last != 0, n > 0 and
 *     tag_{n-1} == 0 one more entry, n (the tail).  n_seg[b] = their number, NOT clipped to Smax (mts_mask_plan's rule); entries at
 *     j >= min(n_seg[b], Smax) are -1.  n == 0 gives n_seg = 0.
 * One workgroup per document; masks, prefix popcounts and a ring of the last m best() values in LDS.  Every element of every output is
 * written exactly once by a plain vector store: no atomics, no workspace, no memset; the same bits on every call.
 * MTS_ERR_INVALID before any device work: B < 0, L < 1, Smax < 1, n_out outside 1..4, with min_segment >= 2 a threshold outside
 * [-1024, 1024] or NaN, and with B > 0 a null scores / seg_end / n_seg.  MTS_ERR_UNSUPPORTED: L > 65536, min_segment outside 1..1024.
 * B == 0 returns MTS_OK without a launch. */
int mts_segment_decode(void* stream, int B, int L, int n_out,
                       const float* scores,         /* device fp32 [B, L, n_out] */
                       const int32_t* lengths,      /* device [B] or NULL */
                       float threshold, int min_segment, int close_last, int Smax,
                       uint8_t* tags,               /* device [B, L] or NULL */
                       float* prob,                 /* device [B, L] or NULL */
                       int32_t* seg_end,            /* device [B, Smax] */
                       int32_t* n_seg);             /* device [B] */
/* DECISION-THRESHOLD SWEEP.  Replaces the host loop of models/lightning_model.py:435-553 (the disabled validation-epoch hook) over
 * compute_Pk / compute_window_diff / f1_score: for every document b and threshold j the six integers from which Pk, WindowDiff and
 * boundary-F1 follow exactly.  scores fp32 [B, L, n_out], n_out 1..4; targets fp32 [B, Lt], Lt >= L, 0 / 1 inside a document's length
 * (pad values are never read); lengths int32 [B], NULL = every document has L sentences (clamped to 0..L); thresholds DEVICE fp32 [T],
 * 1 <= T <= 64, any order; counts_out int32 [B, T, 6] = {pk_err, wd_err, windows, tp, fp, fn}.  For a document of n sentences:
 *   h_i = p_i > thresholds[j], strict, p_i the probability of mts_greedy_decode, same bits;  t_i = (targets[b, i] == 1)
 *   pos_x(i) = sum_{m < i} x_m  (the segment index of sentence i once the last sentence is forced to a boundary, as compute_Pk does)
 *   nseg = 1 + sum_{i < n-1} t_i;  k = max(round_half_even(n / (2 nseg)), 2);  windows = max(n - k, 0)
 *   pk_err = #{i < windows: (pos_h(i) == pos_h(i+k)) != (pos_t(i) == pos_t(i+k))}
 *   wd_err = #{i < windows: pos_h(i+k) - pos_h(i) != pos_t(i+k) - pos_t(i)}
 *   tp / fp / fn over i < n of h' against t', where t' = t with t'_{n-1} = 0 (compute_Pk leaves it so before f1_score runs) and
 *   h' = h, with h'_{n-1} = 0 when end_boundary.
 * n == 0 gives six zeros.  One launch, no workspace, no atomics: integers, identical from run to run.
 * MTS_ERR_INVALID before any device work for null operands, n_out outside 1..4, T outside 1..64, Lt < L;  MTS_ERR_UNSUPPORTED for L > 65536. */
int mts_threshold_sweep(void* stream, int B, int L, int Lt, int n_out, const float* scores, const float* targets,
                        const int32_t* lengths, int T, const float* thresholds, int end_boundary, int32_t* counts_out);
/* WinPR SWEEP (metric 'scaiano').  Replaces the host loop over WinPR (models/lightning_model.py:57-124) as test_step calls it (:622),
 * WinPR(reference = tags, hypothesis = target): operands, ranges and status codes as mts_threshold_sweep, plus the window k, 1..64
 * (upstream: 10); counts_out int32 [B, T, 3] = {TP, FP, FN}.  For a document of n sentences, h and t as above, except that the masks
 * are left as the scaiano branch of test_step leaves them: under end_boundary bit n-1 is 0 in BOTH, otherwise nothing is cleared (the
 * target's last sentence counts, unlike the F1 counts above).  For every i = 1-k .. n (n + k windows) and a in {h, t}:
 *   cnt(a, i)  = #{x in [max(i,0), min(i+k,n)) : a_x} + prev(a, i)
 *   prev(a, i) = 0 for i == 1-k;  a[i-1] for i >= 1;  for 2-k <= i <= 0: a[lo] if lo < hi else 0, lo = max(n+i-1, 0), hi = min(i-1+k, n)
 *                (python's wrap-around of reference[i-1:i-1+k] for a negative start; non-zero only for n < k)
 *   R = cnt(h, i), C = cnt(t, i);  TP += min(R, C);  FP += max(0, C - R);  FN += max(0, R - C)
 * n == 0 gives three zeros.  One launch, no workspace, no atomics: integers, identical from run to run.
 * MTS_ERR_INVALID additionally for k outside 1..64. */
int mts_winpr_sweep(void* stream, int B, int L, int Lt, int n_out, const float* scores, const float* targets,
                    const int32_t* lengths, int T, const float* thresholds, int end_boundary, int k, int32_t* counts_out);
/* BOOTSTRAP RESAMPLING SUMS.  Replaces the host loop of train_fit.py:540-562 / compute_accuracy_metrics_sentence.py:63-260 (10 000 x
 * DataFrame.sample(frac=1, replace=True) and a mean per metric).  values: DEVICE float64 [M, n], M metric rows over n documents;
 * sums: DEVICE float64 [M, S], every element written.  Resample s (0 .. S-1) draws n indices with replacement by the counter hash of
 * the dropout kernels (splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (idx + 1), upper 32 bits), no RNG state:
 *   i_j        = (uint32)(((uint64)hash32(seed, (uint64)s * n + j) * (uint64)n) >> 32),   j = 0 .. n-1
 *   sums[m, s] = ((0 + values[m, i_0]) + values[m, i_1]) + ... + values[m, i_{n-1}]       float64, added in that order
 * All M rows share the draw (a resampled document keeps its metrics paired).  The multiply-shift draw gives every index floor(2^32 / n)
 * or one more of the 2^32 hash values: a relative bias below n / 2^32.  The division by n is the caller's.  Bitwise reproducible: a host
 * loop with the same hash gives the same bits.  One launch, no workspace, no atomics.
 * MTS_ERR_INVALID before any device work for n outside 1..2^20, M outside 1..16, S outside 1..2^22, null operands. */
int mts_bootstrap_sums(void* stream, int n, int M, int S, const double* values, uint64_t seed, double* sums);
/* scores[r, c] = x[r,:] . w[c,:] + b[c]  (x act dtype [rows, D]; w fp32 [n_out, D]); n_out in 1..4 */
int mts_head_fwd(void* stream, int dtype, int rows, int D, int n_out, const void* x, int ldx, const float* w,
                 const float* b, float* scores);
/* dw[c,:] = sum_r dscores[r,c] x[r,:], db[c] = sum_r dscores[r,c] (OVERWRITE); workspace as layernorm_bwd */
int mts_head_bwd_params(void* stream, int dtype, int rows, int D, int n_out, const void* x, int ldx,
                        const float* dscores, float* dw, float* db, void* partial);
/* dx[r,:] (+)= sum_c dscores[r,c] w[c,:] */
int mts_head_bwd_data(void* stream, int dtype, int rows, int D, int n_out, const float* dscores, const float* w,
                      void* dx, int lddx, int accumulate);

/* ---------------------------------------------------------------------------------------------
 * Domain-switched heads.  Replaces the `switch == 'dense'` tail of SwitchBiLSTM (models/CRF.py:1195-1205 in loss, :1248-1258 in
 * forward) with its regroup (:1132-1139): classification_1 / classification_2 over the whole batch and the per-document pick.
 * x, dx: [B*L, D] act dtype with leading dimensions in ELEMENTS; w: fp32 [2, n_out, D] (the two heads stacked), bias: fp32 [2, n_out];
 * n_out in 1..4; scores, dscores: fp32 [B, L, n_out].  int32 device maps, built on the host from the batch's `domains`:
 *   doc_head [B]: the head (0 = classification_1, 1 = classification_2) that scores document b;
 *   doc_src  [B]: the document whose rows of x document b is scored from (upstream: its rank inside its own domain group);
 *   doc_tgt  [2, B]: doc_tgt[k][r] = the one document of head k with doc_src == r, or -1 (the inverse of the two maps above).
 * forward:    scores[b, t, c] = x[doc_src[b], t, :] . w[doc_head[b], c, :] + bias[doc_head[b], c]   (fp32 accumulation)
 * bwd_params: dw[k, c, :] = sum_{b: doc_head[b] = k} sum_t dscores[b, t, c] x[doc_src[b], t, :], db[k, c] likewise; OVERWRITE: a head that
 *             no document uses comes out as exact zeros; no atomics, bitwise reproducible.  workspace: mts_switch_head_bwd_workspace(D)
 *             bytes, 16-byte aligned.
 * bwd_data:   dx[r, t, :] = sum_k sum_c dscores[doc_tgt[k][r], t, c] w[k, c, :]  (gather form, no atomics); every row is OVERWRITTEN, rows
 *             that no document reads with zeros.
 * A map entry outside its range (doc_src not in [0, B), doc_head not in {0, 1}, doc_tgt not in [-1, B)) contributes nothing: the
 * kernels write 0 there and form no address from it.
 * MTS_ERR_INVALID before any launch: D or a leading dimension no multiple of 4; x / dx not aligned to a 4-element vector (16 bytes in
 * fp32, 8 in bf16); w, dw or the workspace not 16-byte aligned; n_out outside 1..4.  MTS_ERR_UNSUPPORTED: bwd_params with D > 4096.
 * ------------------------------------------------------------------------------------------- */
int mts_switch_head_fwd(void* stream, int dtype, int B, int L, int D, int n_out, const void* x, int ldx, const float* w,
                        const float* bias, const int32_t* doc_src, const int32_t* doc_head, float* scores);
size_t mts_switch_head_bwd_workspace(int D);
int mts_switch_head_bwd_params(void* stream, int dtype, int B, int L, int D, int n_out, const void* x, int ldx, const float* dscores,
                               const int32_t* doc_src, const int32_t* doc_head, float* dw, float* db, void* workspace);
int mts_switch_head_bwd_data(void* stream, int dtype, int B, int L, int D, int n_out, const float* dscores, const float* w,
                             const int32_t* doc_tgt, void* dx, int lddx);

/* ---------------------------------------------------------------------------------------------
 * LSTM recurrence with packed-sequence semantics.
 * Replaces: aten::lstm under pack_padded_sequence / pad_packed_sequence
 * (models/NeuralArchitectures.py:98-115): gate order i,f,g,o, zero initial state, rows >= len are 0,
 * the reverse direction starts at each document's own last sentence.
 * xproj: [B*L, ndir*4H] act dtype = x W_ih^T + b_ih for both directions (direction d owns columns
 *   d*4H..(d+1)*4H), produced by mts_gemm.  w_hh: fp32 [ndir, 4H, H]; b_hh: fp32 [ndir, 4H] (may be NULL),
 *   added to the gate pre-activations in fp32 inside the recurrence.
 * out: [B*L, ndir*H] act dtype.  gates (saved for backward): act dtype, B*L*ndir*4H elements, post-activation
 *   i,f,g,o; cells: fp32, B*L*ndir*H elements.  Both are OPAQUE saved state handed unchanged to mts_lstm_bwd under the same options
 *   (the generic and the persistent-MFMA kernels keep them as [B*L, ndir*4H] / [B*L, ndir*H]; the bf16 CU-quad recurrences keep
 *   step-major blocks).
 * lengths int32 [B], NULL = every document has L sentences (clamped to 0..L): a document of length 0 gets rows of exact zeros in out
 *   and dxproj and contributes nothing to dw_hh; ndir is 1 (forward direction only) or 2 in every form.
 * bf16 with H % 8 != 0, fp32 with H % 4 != 0: the forward and mts_lstm_bwd_recurrence run, mts_lstm_bwd / mts_lstm_bwd_whh return
 *   MTS_ERR_UNSUPPORTED before any launch (the dW_hh GEMM needs such rows; the taggers pad the hidden size to a multiple of 8).
 * ------------------------------------------------------------------------------------------- */
/* workspace (both calls): mts_lstm_workspace(dtype, B, L, H, ndir) bytes */
size_t mts_lstm_workspace(int dtype, int B, int L, int H, int ndir);
int mts_lstm_fwd(void* stream, int dtype, int B, int L, int H, int ndir, const void* xproj, const float* w_hh,
                 const float* b_hh, const int32_t* lengths, void* out, void* gates, float* cells, void* workspace);
/* dxproj: [B*L, ndir*4H] act dtype (gradient wrt pre-activation gates); dw_hh fp32 [ndir,4H,H] OVERWRITTEN. */
int mts_lstm_bwd(void* stream, int dtype, int B, int L, int H, int ndir, const float* w_hh, const int32_t* lengths,
                 const void* out, const void* gates, const float* cells, const void* dout, void* dxproj,
                 float* dw_hh, void* workspace);
/* mts_lstm_bwd in two calls (recurrence | h_{t-1} + dW_hh), so that the weight-gradient half can run on another stream while the caller's next
 * dependent launch follows the recurrence directly.  `workspace`: the same buffer for both calls of a layer, untouched in between. */
int mts_lstm_bwd_recurrence(void* stream, int dtype, int B, int L, int H, int ndir, const float* w_hh, const int32_t* lengths,
                            const void* out, const void* gates, const float* cells, const void* dout, void* dxproj, void* workspace);
int mts_lstm_bwd_whh(void* stream, int dtype, int B, int L, int H, int ndir, const int32_t* lengths, const void* out, const void* dxproj,
                     float* dw_hh, void* workspace);

/* ---------------------------------------------------------------------------------------------
 * CRF head.  Replaces models/CRF.py:98-240 (fc output = `feats` is produced by mts_gemm/mts_head_fwd).
 * feats: fp32 [B, L, C]; C = num_tags + 2 (START = C-2, STOP = C-1); trans fp32 [C, C], T[i,j] = j -> i.
 * ------------------------------------------------------------------------------------------- */
/* loss_out[0] = mean_b(logZ_b - gold_b); dfeats [B,L,C] and dtrans [C,C] are OVERWRITTEN (may be NULL; dtrans needs dfeats).
 * C in 3..8; lengths may be NULL (every document L long) and are clamped to 0..L; tags fp32 [B, Lt], Lt >= L; rows of dfeats past a
 * document's length are written 0.
 * Numeric domain of C == 4: that path carries softmax(alpha) in fp32 (the scaled recursion), so a step's worst filtered-probability
 * ratio exp(-(2 Se + 2 St)) -- Se, St: the largest |emission| and |finite transition| -- must stay a normal fp32: emission spread
 * plus transition spread below about 87 nats per step.  Beyond that a tag's probability underflows to 0 and dfeats / dtrans can be
 * wrong WITHOUT a NaN or an error code (the loss degrades later than the gradients).  The generic path (C != 4) works in the log
 * domain and has no such limit.  Evidence so far: an fp32 CPU emulation of the recursion (exact at +-30 / +-10 and +-40 / +-20,
 * dfeats off by 1.0 at +-60 / +-20) and tests/test_gpu_crf.py at +-30 / +-10; the kernel neither detects nor survives that regime. */
size_t mts_crf_workspace(int B, int L, int C);
int mts_crf_nll(void* stream, int B, int L, int C, const float* feats, const float* tags, int Lt,
                const int32_t* lengths, const float* trans, float* loss_out, float* dfeats, float* dtrans,
                float* workspace /* mts_crf_workspace(B, L, C) bytes */);
/* best_score fp32 [B]; paths int32 [B, L] (entries >= length are written -1); bp_ws int32 [B, L, C].  Ties go to the lowest tag
 * index (torch.max).  C == 4 keeps its back-pointers in LDS up to L = 10 240 and uses bp_ws (the generic kernel) beyond. */
int mts_crf_viterbi(void* stream, int B, int L, int C, const float* feats, const int32_t* lengths,
                    const float* trans, float* best_score, int32_t* paths, int32_t* bp_ws);
/* Posterior (max-marginal) decode, an extension (the reference decodes by Viterbi only; DESIGN.md "CRF posterior-marginal decode"):
 * the forward-backward recursion of models/CRF.py:218-240 without tags.  With alpha_0 the START one-hot (-1e4 convention),
 * alpha_{t+1}(i) = lse_j(alpha_t(j) + T[i][j]) + f_t(i), beta_n(i) = T[stop][i], beta_t(j) = lse_i(T[i][j] + f_t(i) + beta_{t+1}(i)),
 * lm_t(i) = alpha_{t+1}(i) + beta_{t+1}(i) - log Z:
 *   scores[b, t] = clamp(lm_t(cls) - lse_{i != cls} lm_t(i), -80, +80) for t < n_b, exactly 0 for t >= n_b  (fp32 [B, L], every element
 *   written); logz[b] = lse_i(alpha_n(i) + T[stop][i]) (fp32 [B], may be NULL; n_b = 0 included).
 * A logit for the 1-wide decode rule sigmoid(score) > th (mts_greedy_decode, the threshold sweeps): sigmoid(+80) is exactly 1 in fp32 and
 * sigmoid(-80) a normal positive number, so no threshold in (0, 1) decodes the clamped score differently.  C in 3..8, cls in 0..C-1;
 * lengths may be NULL and are clamped to 0..L.  No atomics; bitwise reproducible from launch to launch.
 * Numeric domain of C == 4: as mts_crf_nll -- that path carries softmax(alpha) in fp32 (the scaled recursion), so a step's worst
 * filtered-probability ratio exp(-(2 Se + 2 St)) -- Se, St: the largest |emission| and |finite transition| -- must stay a normal fp32:
 * emission spread plus transition spread below about 87 nats per step.  Inside it the scores are finite and within tolerance
 * (tests/test_gpu_crf_marginal.py at +-30 / +-10); beyond it a tag's probability underflows to 0 and a score can be wrong (still finite:
 * the clamp drops a NaN) WITHOUT an error code.  The generic path (C != 4) works in the log domain and has no such limit. */
int mts_crf_marginals(void* stream, int B, int L, int C, int cls, const float* feats, const int32_t* lengths,
                      const float* trans, float* scores, float* logz, float* workspace /* mts_crf_workspace(B, L, C) bytes */);
/* The three entry points above on PACKED rows (the layout the transformer taggers train on: only the valid sentences, document after
 * document).  Arguments of the sibling, then row0 int32 [B] (device) and n_rows:
 *   feats / dfeats fp32 [n_rows, C]; document b owns rows row0[b] .. row0[b] + len_b - 1 (len_b: lengths[b] clamped to 0..L; lengths
 *   must be given with row0); tags stays [B, Lt] and the workspace mts_crf_workspace(B, L, C) bytes (alphas are kept per document);
 *   mts_crf_marginals_packed: scores fp32 [n_rows] (one logit per packed row, nothing behind them); logz [B];
 *   mts_crf_viterbi_packed: paths stays int32 [B, L] with -1 past the length; bp_ws int32 [n_rows, C].
 * The same kernels and the same arithmetic at other addresses: for rows that hold the same emissions the results are bitwise those of
 * the padded entry points, and row0 == NULL IS the padded layout (n_rows is then only checked for its sign).  mts_crf_nll_packed scales
 * the n_rows * C elements of dfeats by 1 / B and writes nothing behind them; rows of dfeats / scores that no document owns keep what
 * they held (dfeats: times 1 / B).  A document whose rows would leave [0, n_rows) forms no address and contributes nothing: loss and
 * gradients 0 (B still divides), best_score 0 and a path of -1, logz 0, no score written.  MTS_ERR_INVALID before any launch: a null
 * operand, n_rows < 0, C outside 3..8, row0 without lengths.  No atomics; bitwise reproducible from launch to launch. */
int mts_crf_nll_packed(void* stream, int B, int L, int C, const float* feats, const float* tags, int Lt,
                       const int32_t* lengths, const float* trans, float* loss_out, float* dfeats, float* dtrans,
                       float* workspace, const int32_t* row0, int n_rows);
int mts_crf_viterbi_packed(void* stream, int B, int L, int C, const float* feats, const int32_t* lengths,
                           const float* trans, float* best_score, int32_t* paths, int32_t* bp_ws, const int32_t* row0, int n_rows);
int mts_crf_marginals_packed(void* stream, int B, int L, int C, int cls, const float* feats, const int32_t* lengths,
                             const float* trans, float* scores, float* logz, float* workspace, const int32_t* row0, int n_rows);

/* ---------------------------------------------------------------------------------------------
 * Optimizer step over a flat fp32 parameter buffer.
 * Replaces torch.optim.Adam(eps=1e-7) / SGD(momentum .9, wd 1e-4) of models/lightning_model.py:759-765.
 * grad_scale multiplies the gradient first (1/world_size after an RCCL sum all-reduce).
 * If bf16_copy != NULL the updated parameters are also written as bf16 (next step's GEMM weights).
 * mts_adam_step uses 16-byte accesses: param, grad and both moments must be 16-byte aligned and bf16_copy 8-byte aligned (a slice
 * of the flat buffer has to begin on a multiple of 4 elements); any n.  mts_sgd_step works element by element: fp32 operands
 * 4-byte, bf16_copy 2-byte aligned.  A pointer off its boundary is MTS_ERR_INVALID before any launch; there is no scalar fallback.
 * ------------------------------------------------------------------------------------------- */
int mts_adam_step(void* stream, size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* bf16_copy);
int mts_sgd_step(void* stream, size_t n, float* param, const float* grad, float* momentum_buf, float lr,
                 float momentum, float weight_decay, int first_step, float grad_scale, void* bf16_copy);
/* GRADIENT CLIPPING inside the optimizer pass.  Replaces what Lightning's Trainer(gradient_clip_val, gradient_clip_algorithm)
 * (train_fit.py:288,295,779) does between backward and optimizer.step(): torch.nn.utils.clip_grad_norm_ / clip_grad_value_.
 *
 * mts_grad_norm: norm_out[0] = || grad_scale * grad ||_2 over n_spans (1..4) spans [span_begin_host[s], span_end_host[s]) (in ELEMENTS
 * of `grad`, host arrays read before the call returns) of the flat fp32 gradient -- the same grad_scale the optimizer applies, so
 * the norm is that of the averaged gradient.  norm_out is a DEVICE fp32 scalar the clipped steps below read on the same stream;
 * the host never sees it.  Two launches: per-workgroup partial sums of squares STORED to `workspace` (mts_grad_norm_workspace()
 * bytes, REQUIRED), then one workgroup adds them in a fixed order and takes the square root.  No atomics: bitwise reproducible.
 * A NaN / Inf element gives a NaN / Inf norm.  Every span must begin on a 16-byte boundary (MTS_ERR_INVALID before any launch
 * otherwise); any length.  All spans empty: MTS_OK without a launch, norm_out is not written (a zeroed scalar stays 0).
 *
 * mts_adam_step_clipped / mts_sgd_step_clipped: mts_adam_step / mts_sgd_step with gr = clip(grad * grad_scale) in place of
 * grad * grad_scale (SGD adds the weight decay AFTER clipping, as torch does when .grad is clipped before step()).
 *   norm mode  (total_norm != NULL, clip_value == 0): gr = (grad * grad_scale) * coef, coef = min(1, max_norm / (*total_norm + 1e-6))
 *              read from device memory; a NaN norm gives a NaN coef.  coef == 1 gives the bits of the unclipped entry points.
 *              clip_coef_out (optional, device fp32 scalar) receives coef.
 *   value mode (total_norm == NULL, clip_value > 0): gr = clamp(grad * grad_scale, -clip_value, +clip_value); a NaN stays NaN.
 * Before any device work: null operands, max_norm < 0 (or NaN), clip_value < 0, neither or both modes selected, and operands that
 * are not aligned (Adam: param, grad and moments to 16 bytes, bf16_copy to 8 -- the vector accesses of the kernel) are
 * MTS_ERR_INVALID.  n == 0: MTS_OK without a launch. */
size_t mts_grad_norm_workspace(void);
int mts_grad_norm(void* stream, const float* grad, int n_spans, const size_t* span_begin_host, const size_t* span_end_host,
                  float grad_scale, float* workspace, float* norm_out);
int mts_adam_step_clipped(void* stream, size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                          float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* bf16_copy,
                          const float* total_norm, float max_norm, float clip_value, float* clip_coef_out);
int mts_sgd_step_clipped(void* stream, size_t n, float* param, const float* grad, float* momentum_buf, float lr,
                         float momentum, float weight_decay, int first_step, float grad_scale, void* bf16_copy,
                         const float* total_norm, float max_norm, float clip_value, float* clip_coef_out);
/* x[0..n) *= scale (fp32).  Token-weighted data parallelism: the reference's loss is a mean over the LOCAL batch's valid
 * sentences (models/CRF.py:352); multiplying d loss / d scores by world * n_local / n_global before the SUM all-reduce (and
 * grad_scale = 1/world in the optimizer) gives the single-process gradient of the global batch. */
int mts_scale(void* stream, size_t n, float* x, float scale);

/* ---------------------------------------------------------------------------------------------
 * wav2vec 2.0 sentence features (csrc/wav2vec2.hip): the pieces of the reference's learned audio encoder (extract_embeddings.py:173-183,
 * Wav2Vec2Model(...).last_hidden_state per sentence) that are not a GEMM, a LayerNorm or full attention.  The encoder is composed of
 * these and of mts_gemm / mts_layernorm_fwd / mts_full_attn_fwd in multimodaltopicsegmentation_amd/wav2vec2.py; inference only.
 * Sentence s is the sent_len[s] samples from sent_start[s] of `wave`, as for mts_mel_frames (clamped into the waveform before any address
 * is formed); it gives T = (n - kernel) / stride + 1 frames of layer 0, none for n < kernel.
 *   wave_stats   stats[s] = (mean, 1 / sqrt(var + 1e-7)) of the sentence's samples, var biased as np.var (two passes); fp64 inside: lane
 *                chains over samples tid, tid + 256, .. and a fixed tree; ONE rounding to fp32.  Wav2Vec2FeatureExtractor(do_normalize).
 *   conv0_stats  v[t, c] = sum_k w[c, k] * fl((x[t * stride + k] - mean) * rstd), an fmaf chain over k = 0 .. kernel - 1 from 0 (conv
 *                layer 0, C_in = 1, no bias).  gmean / grstd [n_sent, C]: the mean of v over the sentence's T frames and 1 / sqrt(var + eps),
 *                var = E[v^2] - mean^2 >= 0 in fp64 (sums per wave over frames q, q + 4, .. , added in wave order), rounded once.  v is
 *                never stored.
 *   conv0        out[block_start[s] + t, c] = gelu_erf(((v[t, c] - gmean) * grstd) * gamma[c] + beta[c]) (GroupNorm(C, C) and exact GELU)
 *                in out_dtype, v recomputed by the same chain; the rows t >= T of the sentence's block [block_start[s], block_start[s + 1])
 *                are written as 0.  block_start: int64 [n_sent + 1] from 0 to total_rows in multiples of 64, block s at least T rows.
 *   regroup      x [*, H] -> out [G][rows_p, H / G]: the padded row pad_start[s] + K_p / 2 + t of group g holds x[src_row0[s] + t,
 *                g * H / G ..], t < pad_start[s + 1] - pad_start[s] - K_p / 2; every other row of out is written as 0 (the K_p / 2 rows in
 *                front of every sentence, which close the sentence before it as well, and the rows from pad_start[n_sent] to rows_p).
 *                With it the grouped convolution Conv1d(H, H, K_p, padding = K_p / 2, groups = G) without its last frame is, per group,
 *                the NT product of the overlapping rows A = out_g + m * H / G (lda = H / G, K = K_p * H / G) with the weights laid
 *                [H / G out, K_p, H / G in]: its row pad_start[s] + t is frame t of sentence s.
 *   pos_conv     the same convolution on the matrix cores (bf16, v_mfma_f32_16x16x32_bf16, fp32 accumulation in four K quarters added
 *                in order), with bias, exact GELU and the residual: y[dst_start[s] + t] = x[src_row0[s] + t] + gelu_erf(conv + bias),
 *                rounded once.  w: bf16 [G][H / G][K_p * H / G] as above; tile_start: int32 [n_sent + 1], the running sum of
 *                ceil(T_s / 64), n_tiles its last entry; T_s = dst_start[s + 1] - dst_start[s].  Zero padding is per sentence.
 *   rows         dst[dst_start[s] + t] = src[src_row0[s] + t] (+ res[res_row0[s] + t], added in fp32) for t < dst_start[s + 1] -
 *                dst_start[s], rounded once to dst_dtype; src and res share src_dtype; all matrices [*, D] with row stride D.
 * All run on the caller's stream, use no atomics, write every output element exactly once and give the same bits for the same inputs; row
 * offsets are 64-bit.  MTS_ERR_INVALID before any device work: a null pointer (res may be NULL), an unknown dtype, a size < 1, H not
 * divisible by G, a negative eps, total_rows no multiple of 64, a matrix off its 16-byte boundary, D no multiple of 4.
 * MTS_ERR_UNSUPPORTED before any launch: C no multiple of 8, kernel > 32, a stride whose tile of samples exceeds 64 KiB of LDS, H / G no
 * multiple of 8, K_p odd or above 128, more rows than one launch covers; pos_conv also H / G > 64 or K_p * H / G no multiple of 128
 * (the GEMM form serves those).
 * ------------------------------------------------------------------------------------------- */
int mts_w2v_wave_stats(void* stream, int n_sent,
                       const float* wave,           /* device [total_samples] */
                       int64_t total_samples,
                       const int64_t* sent_start,   /* device [n_sent] */
                       const int64_t* sent_len,     /* device [n_sent] */
                       float* stats);               /* device [n_sent, 2] out */
int mts_w2v_conv0_stats(void* stream, int n_sent, int C, int kernel, int stride, const float* wave, int64_t total_samples,
                        const int64_t* sent_start, const int64_t* sent_len,
                        const float* wave_stats,    /* device [n_sent, 2] */
                        const float* w,             /* device [C, kernel] */
                        float eps,
                        float* gmean,               /* device [n_sent, C] out */
                        float* grstd);              /* device [n_sent, C] out */
int mts_w2v_conv0(void* stream, int out_dtype, int n_sent, int C, int kernel, int stride, const float* wave, int64_t total_samples,
                  const int64_t* sent_start, const int64_t* sent_len, const float* wave_stats, const float* w, const float* gmean,
                  const float* grstd,
                  const float* gamma,               /* device [C] */
                  const float* beta,                /* device [C] */
                  const int64_t* block_start,       /* device [n_sent + 1] */
                  int64_t total_rows,
                  void* out);                       /* device [total_rows, C] out */
int mts_w2v_regroup(void* stream, int dtype, int n_sent, int H, int G, int Kp,
                    const void* x,                  /* device [*, H] */
                    const int64_t* src_row0,        /* device [n_sent] */
                    const int64_t* pad_start,       /* device [n_sent + 1] */
                    int64_t rows_p,
                    void* out);                     /* device [G, rows_p, H / G] out */
int mts_w2v_rows(void* stream, int src_dtype, int dst_dtype, int n_sent, int D, const void* src, const int64_t* src_row0, const void* res,
                 const int64_t* res_row0,
                 const int64_t* dst_start,          /* device [n_sent + 1] */
                 int64_t total_rows,
                 void* dst);                        /* device [total_rows, D] out */
int mts_w2v_pos_conv(void* stream, int n_sent, int H, int G, int Kp, const void* x, const int64_t* src_row0, const int64_t* dst_start,
                     const int32_t* tile_start, int n_tiles, const void* w, const float* bias, void* y);

/* ---------------------------------------------------------------------------------------------
 * Text sentence features (csrc/text_encoder.hip): the pieces of a BERT-family sentence encoder (BertModel / RobertaModel /
 * XLMRobertaModel behind sentence-transformers' mean pooling: the reference's --encoder / --online_encoding path,
 * EncoderDataset.py:238-250, and the RoBERTa folders of its run scripts) that are not a GEMM, a LayerNorm or mts_full_attn_fwd.  The
 * encoder is composed of these and of mts_gemm / mts_layernorm_fwd / mts_full_attn_fwd in multimodaltopicsegmentation_amd/text.py;
 * inference only.
 *   text_embed   out[i, 0:H] = LayerNorm((word[ids[i]] + position[pos[i]]) + type_row) * gamma + beta, i < n_tokens: BertEmbeddings /
 *                RobertaEmbeddings for token type 0.  The tables word [vocab, H], position [n_pos, H] and type_row [H] are in `dtype`
 *                (MTS_F32 | MTS_BF16), gamma / beta fp32 [H] as for mts_layernorm_fwd, out in `dtype` with row stride ldo (elements;
 *                columns H .. ldo - 1 are not touched).  pos[i] is the row of the position table: the caller has added RoBERTa's offset
 *                (pad_token_id + 1).  One pass: the three rows are read with 16-byte accesses and summed in fp32 in the order written,
 *                the mean and then the biased variance about it are reduced from registers, eps is inside the root
 *                (torch.nn.functional.layer_norm), every element is stored once.  One wave per row; no workspace.
 *                ids and pos are NOT validated on the device: 0 <= ids[i] < vocab and 0 <= pos[i] < n_pos are the caller's to guarantee
 *                before the launch (text.py checks the corpus' largest id and longest sentence on the host); vocab and n_pos are taken
 *                for the argument check only.
 *                MTS_ERR_INVALID: a null pointer, an unknown dtype, a size < 1, a negative eps, ldo < H or no multiple of 4 (fp32) / 8
 *                (bf16), a table, gamma, beta or out off its 16-byte boundary.  MTS_ERR_UNSUPPORTED: H no multiple of 4 (fp32) / 8
 *                (bf16) or above 2048 (fp32) / 4096 (bf16).
 *   sent_attn    full self-attention over packed SHORT sequences, bf16: operands as for mts_full_attn_fwd -- qkv [rows, 3D] with q already
 *                scaled, ctx [rows, D]; sentence s owns the rows row0[s] .. row0[s] + lengths[s] - 1 (both int32 [n_sent], REQUIRED),
 *                1 <= lengths[s] <= max_len.  Query i attends to every key of its sentence.  One wave owns one (sentence, head) pair and
 *                four pairs share a workgroup; the rows of q and k are read once, straight into v_mfma_f32_16x16x32_bf16 fragments; the
 *                softmax is exact over the whole row on the accumulators (max, exp, sum; no online rescaling), P is rounded to bf16
 *                unnormalised and the row's 1 / sum multiplies the fp32 product P V, rounded once to bf16.  No lse (inference only), no
 *                dropout.  Rows outside the listed ones are neither read nor written; a lengths[s] above max_len breaks the contract and is
 *                cut to the instantiation's cover, which max_len selects: 32 tokens for max_len <= 32, else 64.
 *                Covers head dims that are multiples of 32 up to 128 and max_len <= 64; anything else, and fp32, is
 *                MTS_ERR_UNSUPPORTED before any launch (mts_full_attn_fwd serves it).  MTS_ERR_INVALID: a null pointer, an unknown
 *                dtype, a size < 1, D not divisible by heads, qkv off its 16-byte boundary.
 * Both run on the caller's stream, use no atomics, write every output element exactly once and give the same bits for the same inputs.
 * ------------------------------------------------------------------------------------------- */
int mts_text_embed(void* stream, int dtype, int n_tokens, int H,
                   const int32_t* ids,              /* device [n_tokens] */
                   const int32_t* pos,              /* device [n_tokens] */
                   const void* word, int vocab,     /* device [vocab, H] */
                   const void* position, int n_pos, /* device [n_pos, H] */
                   const void* type_row,            /* device [H] */
                   const float* gamma, const float* beta, float eps,
                   void* out, int ldo);             /* device [n_tokens, ldo] out */
int mts_sent_attn_fwd(void* stream, int dtype, int n_sent, int D, int heads, const void* qkv, const int32_t* row0, const int32_t* lengths,
                      int max_len, void* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MTS_H */
