// Device-side collation: the padded batch [B, Lmax, D] is GATHERED from a corpus that lives in HBM (all documents concatenated into one
// [total_rows, D] matrix, uploaded once) by a list of document indices.  Same semantics as mts_collate_pad (collate.hip; the reference's
// `merge`, EncoderDataset.py:20-27, :103-109) with the host pass and the per-step host-to-device copy gone: RadioNews is 119 MB in bf16
// against 288 GB of HBM.
//
// A pure stream of 2 x bytes(batch).  One wave owns a destination row at a time, ROWS_PER_WAVE consecutive rows in flight: the row's
// document, its first corpus row and its length are wave-uniform (scalar loads of doc_index / row_start, once per row, not per lane),
// a row past the document's end (or of an index outside the corpus) is written as pad without forming a source address, and every
// element of dst is written by exactly one plain vector store -- no memset in front, no atomics, no workspace, no LDS.  The access width
// is the widest one the row's byte length and both base addresses allow (16 / 8 / 4 / 2 bytes for a copy; 8 / 2 / 1 elements for
// fp32 -> bf16); rows shorter than one wave-wide access (the targets: D = 1) go through a kernel with one lane per destination unit,
// so that a wave still writes whole cache lines.  All element offsets are 64-bit.
#include <algorithm>
#include "common.h"

namespace {

constexpr int WAVES_PER_BLOCK = 4;
constexpr int ROWS_PER_WAVE = 4;

// fp32 -> bf16, round to nearest even, NaN kept quiet: collate.hip's f32_to_bf16_rne, bit for bit
__host__ __device__ __forceinline__ uint32_t bf16_bits_rne(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

struct alignas(16) F32x8 { uint4 a, b; };

// One "unit" = what a lane moves per access: S read from the corpus, T written to the batch.  `pad` holds the pad value's bit pattern
// replicated over 16 bytes in the DESTINATION dtype.
template <typename V> struct CopyOp {
  typedef V S;
  typedef V T;
  static __device__ __forceinline__ T cvt(const S& s) { return s; }
};
template <int E> struct CastOp;
template <> struct CastOp<8> {
  typedef F32x8 S;
  typedef uint4 T;
  static __device__ __forceinline__ T cvt(const S& s) {
    return make_uint4(bf16_bits_rne(s.a.x) | (bf16_bits_rne(s.a.y) << 16), bf16_bits_rne(s.a.z) | (bf16_bits_rne(s.a.w) << 16),
                      bf16_bits_rne(s.b.x) | (bf16_bits_rne(s.b.y) << 16), bf16_bits_rne(s.b.z) | (bf16_bits_rne(s.b.w) << 16));
  }
};
template <> struct CastOp<2> {
  typedef uint2 S;
  typedef uint32_t T;
  static __device__ __forceinline__ T cvt(const S& s) { return bf16_bits_rne(s.x) | (bf16_bits_rne(s.y) << 16); }
};
template <> struct CastOp<1> {
  typedef uint32_t S;
  typedef uint16_t T;
  static __device__ __forceinline__ T cvt(const S& s) { return (uint16_t)bf16_bits_rne(s); }
};

__device__ __forceinline__ uint4 pad_as(const uint4& p, uint4*) { return p; }
__device__ __forceinline__ uint2 pad_as(const uint4& p, uint2*) { return make_uint2(p.x, p.y); }
__device__ __forceinline__ uint32_t pad_as(const uint4& p, uint32_t*) { return p.x; }
__device__ __forceinline__ uint16_t pad_as(const uint4& p, uint16_t*) { return (uint16_t)p.x; }

// corpus row that destination row (b, i) copies, or -1 for a pad row.  Reads doc_index[b] (b < B) and, for an index inside the corpus
// only, row_start[d] and row_start[d + 1].
__device__ __forceinline__ int64_t source_row(int b, int i, const int64_t* __restrict__ row_start, int n_docs,
                                              const int32_t* __restrict__ doc_index) {
  const int d = doc_index[b];
  if ((unsigned)d >= (unsigned)n_docs) return -1;
  const int64_t s = row_start[d];
  return (int64_t)i < row_start[d + 1] - s ? s + i : -1;
}

// U units per row, U >= 64.  Wave w of the launch owns destination rows [w * ROWS_PER_WAVE, (w + 1) * ROWS_PER_WAVE).
template <typename Op>
__global__ __launch_bounds__(WAVES_PER_BLOCK* MTS_WAVE) void gather_rows_kernel(const typename Op::S* __restrict__ corpus,
                                                                                const int64_t* __restrict__ row_start, int n_docs,
                                                                                const int32_t* __restrict__ doc_index,
                                                                                typename Op::T* __restrict__ dst, int64_t rows, int Lmax, int U,
                                                                                uint4 pad16) {
  typedef typename Op::S S;
  typedef typename Op::T T;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & (MTS_WAVE - 1);
  const int64_t r0 = ((int64_t)blockIdx.x * WAVES_PER_BLOCK + wave) * ROWS_PER_WAVE;
  if (r0 >= rows) return;
  const T padv = pad_as(pad16, (T*)nullptr);
  int b = (int)(r0 / Lmax), i = (int)(r0 - (int64_t)b * Lmax);
  const S* src[ROWS_PER_WAVE];
  bool live[ROWS_PER_WAVE];
#pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    live[k] = r0 + k < rows;
    src[k] = nullptr;
    if (live[k]) {
      const int64_t s = source_row(b, i, row_start, n_docs, doc_index);
      if (s >= 0) src[k] = corpus + s * U;
    }
    if (++i == Lmax) { i = 0; ++b; }
  }
  T* d0 = dst + r0 * U;
  // two wave-wide accesses of every row per trip: 2 x ROWS_PER_WAVE loads in flight per lane before the first store
  for (int c = lane; c < U; c += 2 * MTS_WAVE) {
    const int c1 = c + MTS_WAVE;
    const bool two = c1 < U;
    T v0[ROWS_PER_WAVE], v1[ROWS_PER_WAVE];
#pragma unroll
    for (int k = 0; k < ROWS_PER_WAVE; ++k) {
      v0[k] = padv;
      v1[k] = padv;
      if (src[k]) {
        v0[k] = Op::cvt(src[k][c]);
        if (two) v1[k] = Op::cvt(src[k][c1]);
      }
    }
#pragma unroll
    for (int k = 0; k < ROWS_PER_WAVE; ++k) {
      if (live[k]) {
        d0[(int64_t)k * U + c] = v0[k];
        if (two) d0[(int64_t)k * U + c1] = v1[k];
      }
    }
  }
}

// U units per row, U < 64 (the targets, narrow test shapes): one lane per destination unit, consecutive lanes write consecutive units
template <typename Op>
__global__ __launch_bounds__(256) void gather_thin_kernel(const typename Op::S* __restrict__ corpus, const int64_t* __restrict__ row_start,
                                                          int n_docs, const int32_t* __restrict__ doc_index,
                                                          typename Op::T* __restrict__ dst, int64_t units, int Lmax, int U, uint4 pad16) {
  typedef typename Op::T T;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= units) return;
  const int64_t r = idx / U;
  const int c = (int)(idx - r * U);
  const int b = (int)(r / Lmax), i = (int)(r - (int64_t)b * Lmax);
  const int64_t s = source_row(b, i, row_start, n_docs, doc_index);
  dst[idx] = s >= 0 ? Op::cvt(corpus[s * U + c]) : pad_as(pad16, (T*)nullptr);
}

template <typename Op>
int launch(hipStream_t st, const void* corpus, const int64_t* row_start, int n_docs, const int32_t* doc_index, void* dst, int64_t rows,
           int Lmax, int U, uint4 pad16) {
  typedef typename Op::S S;
  typedef typename Op::T T;
  if (U >= MTS_WAVE) {
    const int64_t per_block = WAVES_PER_BLOCK * ROWS_PER_WAVE;
    const int64_t blocks = (rows + per_block - 1) / per_block;
    MTS_UNSUPPORTED(blocks <= 0x7fffffffLL, "mts_gather_pad: %lld destination rows are more than one launch covers", (long long)rows);
    hipLaunchKernelGGL(gather_rows_kernel<Op>, dim3((unsigned)blocks), dim3(WAVES_PER_BLOCK * MTS_WAVE), 0, st, (const S*)corpus, row_start,
                       n_docs, doc_index, (T*)dst, rows, Lmax, U, pad16);
  } else {
    const int64_t units = rows * U;
    const int64_t blocks = (units + 255) / 256;
    MTS_UNSUPPORTED(blocks <= 0x7fffffffLL, "mts_gather_pad: %lld destination rows are more than one launch covers", (long long)rows);
    hipLaunchKernelGGL(gather_thin_kernel<Op>, dim3((unsigned)blocks), dim3(256), 0, st, (const S*)corpus, row_start, n_docs, doc_index,
                       (T*)dst, units, Lmax, U, pad16);
  }
  MTS_LAUNCH_CHECK("mts_gather_pad");
  return MTS_OK;
}

}  // namespace

extern "C" int mts_gather_pad(void* stream, int src_dtype, int dst_dtype, int B, int Lmax, int D, const void* corpus, const int64_t* row_start,
                              int n_docs, const int32_t* doc_index, void* dst, float pad_value) {
  MTS_CHECK_ARG((src_dtype == MTS_F32 || src_dtype == MTS_BF16) && (dst_dtype == MTS_F32 || dst_dtype == MTS_BF16),
                "mts_gather_pad: dtypes must be fp32 or bf16 (got %d -> %d)", src_dtype, dst_dtype);
  MTS_CHECK_ARG(B >= 0 && Lmax >= 1 && D >= 1 && n_docs >= 1, "mts_gather_pad: bad shape (B %d, Lmax %d, D %d, n_docs %d)", B, Lmax, D, n_docs);
  if (B == 0) return MTS_OK;
  MTS_CHECK_ARG(corpus && row_start && doc_index && dst, "mts_gather_pad: null pointer");
  MTS_UNSUPPORTED(!(src_dtype == MTS_BF16 && dst_dtype == MTS_F32), "mts_gather_pad: bf16 -> fp32 is not covered (hold the corpus in fp32)");
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * Lmax;
  uint32_t pbits;
  memcpy(&pbits, &pad_value, 4);
  if (dst_dtype == MTS_BF16) {
    const uint32_t h = bf16_bits_rne(pbits) & 0xffffu;
    pbits = h | (h << 16);
  }
  const uint4 pad16 = make_uint4(pbits, pbits, pbits, pbits);
  const uintptr_t sa = (uintptr_t)corpus, da = (uintptr_t)dst;
  MTS_CHECK_ARG((sa & (src_dtype == MTS_F32 ? 3 : 1)) == 0 && (da & (dst_dtype == MTS_F32 ? 3 : 1)) == 0,
                "mts_gather_pad: corpus / dst not aligned to their element size");
  if (src_dtype == dst_dtype) {
    const int64_t row_bytes = (int64_t)D * (dst_dtype == MTS_F32 ? 4 : 2);
    const uintptr_t all = sa | da | (uintptr_t)row_bytes;
    MTS_CHECK_ARG(row_bytes / 2 <= 0x7fffffffLL, "mts_gather_pad: D %d too large", D);
    if ((all & 15) == 0) return launch<CopyOp<uint4>>(st, corpus, row_start, n_docs, doc_index, dst, rows, Lmax, (int)(row_bytes / 16), pad16);
    if ((all & 7) == 0) return launch<CopyOp<uint2>>(st, corpus, row_start, n_docs, doc_index, dst, rows, Lmax, (int)(row_bytes / 8), pad16);
    if ((all & 3) == 0) return launch<CopyOp<uint32_t>>(st, corpus, row_start, n_docs, doc_index, dst, rows, Lmax, (int)(row_bytes / 4), pad16);
    return launch<CopyOp<uint16_t>>(st, corpus, row_start, n_docs, doc_index, dst, rows, Lmax, (int)(row_bytes / 2), pad16);
  }
  // fp32 -> bf16
  if (D % 8 == 0 && (sa & 15) == 0 && (da & 15) == 0) return launch<CastOp<8>>(st, corpus, row_start, n_docs, doc_index, dst, rows, Lmax, D / 8, pad16);
  if (D % 2 == 0 && (sa & 7) == 0 && (da & 3) == 0) return launch<CastOp<2>>(st, corpus, row_start, n_docs, doc_index, dst, rows, Lmax, D / 2, pad16);
  return launch<CastOp<1>>(st, corpus, row_start, n_docs, doc_index, dst, rows, Lmax, D, pad16);
}
