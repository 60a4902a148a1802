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
//
// mts_gather_segments is the same stream with one more table in front of the source row: a document is gathered as a list of its own
// row ranges ("listed segments": a destination offset and a source offset each), which reorders its topic segments on the way into the
// batch (resident.AugmentedCorpus).  mts_gather_rows names every destination row's source row in a table of its own (resident.MaskedCorpus:
// the table is the plan mts_mask_plan made).  The three entry points share the units (CopyOp / CastOp), the width selection (gather) and
// the copy loop (copy_rows) below, so that they cannot drift apart; only the rule that names a destination row's source row differs.
#include <algorithm>
#include <type_traits>
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

// The copy itself, shared by both gathers: ROWS_PER_WAVE consecutive destination rows at d0; src[k] == nullptr writes row k as pad, a row
// that is not live is not written.  Two wave-wide accesses of every row per trip: 2 x ROWS_PER_WAVE loads in flight per lane before
// the first store.
template <typename Op>
__device__ __forceinline__ void copy_rows(const typename Op::S* const (&src)[ROWS_PER_WAVE], const bool (&live)[ROWS_PER_WAVE],
                                          typename Op::T* __restrict__ d0, int U, int lane, typename Op::T padv) {
  typedef typename Op::T T;
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
  copy_rows<Op>(src, live, dst + r0 * U, U, lane, padv);
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


// ---- mts_gather_segments --------------------------------------------------------------------------------------------------------
// The listed-segment tables of a batch (include/mts.h).  Document b lists segments [ptr[b], ptr[b + 1]): segment j holds destination
// rows dst_off[j] .. dst_off[j + 1] (the last one: .. dst_len[b]) and copies them from the document's rows src_off[j] onwards.
struct SegTables {
  const int32_t* ptr;         // [B + 1]
  const int32_t* dst_off;     // [n_listed], ascending per document
  const int32_t* src_off;     // [n_listed], relative to the document's first row
  const int32_t* dst_len;     // [B]
  const int32_t* close_last;  // [B], or null: no label rule
  int n_listed;
};

// Where one destination document stands: its stored rows, its listed segments and the one that holds the current row.  In the
// wave-per-row kernel every field is wave-uniform (b is), so open() and advance() are scalar loads and scalar arithmetic.
struct SegCursor {
  int64_t first, rows;  // first corpus row and number of rows of the stored document; rows == 0: every row is pad
  int hi, len;          // end of the document's listed segments in the tables; its destination length
  int j, lo;            // listed segment that holds the current row (lo - 1: none does)
  int cur_dst, cur_src, next;  // dst_off[j], src_off[j]; dst_off[j + 1], INT_MAX behind the last listed segment

  __device__ __forceinline__ void load(const SegTables& t) {
    cur_dst = j >= lo ? t.dst_off[j] : 0;
    cur_src = j >= lo ? t.src_off[j] : 0;
    next = j + 1 < hi ? t.dst_off[j + 1] : 0x7fffffff;
  }
  // document b, standing on its row i: the segment is found by a binary search over the document's destination offsets
  __device__ __forceinline__ void open(int b, int i, const int64_t* __restrict__ row_start, int n_docs, const int32_t* __restrict__ doc_index,
                                       const SegTables& t) {
    const int d = doc_index[b];
    first = 0;
    rows = 0;
    if ((unsigned)d < (unsigned)n_docs) {
      first = row_start[d];
      rows = row_start[d + 1] - first;
    }
    lo = min(max(t.ptr[b], 0), t.n_listed);
    hi = min(max(t.ptr[b + 1], lo), t.n_listed);
    len = t.dst_len[b];
    int a = lo, z = hi;  // first listed segment that starts behind row i
    while (a < z) {
      const int m = (a + z) >> 1;
      if (t.dst_off[m] <= i) a = m + 1; else z = m;
    }
    j = a - 1;
    load(t);
  }
  // the next row of the same document: a forward walk, which loads only when the row leaves the segment
  __device__ __forceinline__ void advance(int i, const SegTables& t) {
    while (i >= next) {
      ++j;
      load(t);
    }
  }
  // corpus row that destination row i copies, or -1 for a pad row: past the destination length, held by no listed segment, or a
  // source row outside the stored document (no address is formed from it)
  __device__ __forceinline__ int64_t source(int i) const {
    if (i >= len || j < lo) return -1;
    const int64_t off = (int64_t)cur_src + ((int64_t)i - cur_dst);
    return off >= 0 && off < rows ? first + off : -1;
  }
};

template <typename Op>
__global__ __launch_bounds__(WAVES_PER_BLOCK* MTS_WAVE) void gather_seg_rows_kernel(const typename Op::S* __restrict__ corpus,
                                                                                    const int64_t* __restrict__ row_start, int n_docs,
                                                                                    const int32_t* __restrict__ doc_index, SegTables seg,
                                                                                    typename Op::T* __restrict__ dst, int64_t rows, int Lmax,
                                                                                    int U, uint4 pad16) {
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
  SegCursor cur;
#pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    live[k] = r0 + k < rows;
    src[k] = nullptr;
    if (live[k]) {
      if (k == 0 || i == 0)
        cur.open(b, i, row_start, n_docs, doc_index, seg);
      else
        cur.advance(i, seg);
      const int64_t s = cur.source(i);
      if (s >= 0) src[k] = corpus + s * U;
    }
    if (++i == Lmax) { i = 0; ++b; }
  }
  copy_rows<Op>(src, live, dst + r0 * U, U, lane, padv);
}

// U < 64: one lane per destination unit, and a lane finds its own segment (a wave spans many rows here).  LABELS (the targets, one fp32
// per row): the last row of a listed segment is written as 1, the document's last row as close_last[b] ? 1 : 0.
template <typename Op, bool LABELS>
__global__ __launch_bounds__(256) void gather_seg_thin_kernel(const typename Op::S* __restrict__ corpus, const int64_t* __restrict__ row_start,
                                                              int n_docs, const int32_t* __restrict__ doc_index, SegTables seg,
                                                              typename Op::T* __restrict__ dst, int64_t units, int Lmax, int U, uint4 pad16) {
  typedef typename Op::T T;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= units) return;
  const int64_t r = idx / U;
  const int c = (int)(idx - r * U);
  const int b = (int)(r / Lmax), i = (int)(r - (int64_t)b * Lmax);
  SegCursor cur;
  cur.open(b, i, row_start, n_docs, doc_index, seg);
  const int64_t s = cur.source(i);
  T v = s >= 0 ? Op::cvt(corpus[s * U + c]) : pad_as(pad16, (T*)nullptr);
  if constexpr (LABELS) {
    if (s >= 0) {
      if (i == cur.len - 1)
        v = seg.close_last[b] ? 0x3f800000u : 0u;
      else if (i + 1 == cur.next)
        v = 0x3f800000u;
    }
  }
  dst[idx] = v;
}

// ---- mts_gather_rows ------------------------------------------------------------------------------------------------------------
// The third rule: a row table in front of the source row (negative-sentence masking: mts_mask_plan writes the table, mask_plan.hip).
// Destination row (b, i) copies the document's row src_row[b, i]; a negative entry, one at or behind the document's end, or an index
// outside the corpus is a pad row, and no address is formed from it.  In the wave-per-row kernel b and i are wave-uniform, so the entry
// is one scalar load.
__device__ __forceinline__ int64_t table_row(int b, int i, int Lmax, const int64_t* __restrict__ row_start, int n_docs,
                                             const int32_t* __restrict__ doc_index, const int32_t* __restrict__ src_row) {
  const int d = doc_index[b];
  if ((unsigned)d >= (unsigned)n_docs) return -1;
  const int64_t s = row_start[d];
  const int64_t e = src_row[(int64_t)b * Lmax + i];
  return e >= 0 && e < row_start[d + 1] - s ? s + e : -1;
}

template <typename Op>
__global__ __launch_bounds__(WAVES_PER_BLOCK* MTS_WAVE) void gather_tab_rows_kernel(const typename Op::S* __restrict__ corpus,
                                                                                    const int64_t* __restrict__ row_start, int n_docs,
                                                                                    const int32_t* __restrict__ doc_index,
                                                                                    const int32_t* __restrict__ src_row,
                                                                                    typename Op::T* __restrict__ dst, int64_t rows, int Lmax,
                                                                                    int U, uint4 pad16) {
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
      const int64_t s = table_row(b, i, Lmax, row_start, n_docs, doc_index, src_row);
      if (s >= 0) src[k] = corpus + s * U;
    }
    if (++i == Lmax) { i = 0; ++b; }
  }
  copy_rows<Op>(src, live, dst + r0 * U, U, lane, padv);
}

template <typename Op>
__global__ __launch_bounds__(256) void gather_tab_thin_kernel(const typename Op::S* __restrict__ corpus, const int64_t* __restrict__ row_start,
                                                              int n_docs, const int32_t* __restrict__ doc_index,
                                                              const int32_t* __restrict__ src_row, typename Op::T* __restrict__ dst,
                                                              int64_t units, int Lmax, int U, uint4 pad16) {
  typedef typename Op::T T;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= units) return;
  const int64_t r = idx / U;
  const int c = (int)(idx - r * U);
  const int b = (int)(r / Lmax), i = (int)(r - (int64_t)b * Lmax);
  const int64_t s = table_row(b, i, Lmax, row_start, n_docs, doc_index, src_row);
  dst[idx] = s >= 0 ? Op::cvt(corpus[s * U + c]) : pad_as(pad16, (T*)nullptr);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct RowTable {
  const int32_t* src_row;  // [B, Lmax]
};

struct Args {
  const char* name;
  hipStream_t st;
  const void* corpus;
  const int64_t* row_start;
  int n_docs;
  const int32_t* doc_index;
  const SegTables* seg;  // mts_gather_segments
  const RowTable* tab;   // mts_gather_rows; neither: mts_gather_pad
  void* dst;
  int64_t rows;
  int Lmax;
  uint4 pad16;
};

template <typename Op>
int launch(const Args& a, int U) {
  typedef typename Op::S S;
  typedef typename Op::T T;
  const bool wide = U >= MTS_WAVE;
  const int64_t units = a.rows * U;
  const int64_t per_block = WAVES_PER_BLOCK * ROWS_PER_WAVE;
  const int64_t blocks = wide ? (a.rows + per_block - 1) / per_block : (units + 255) / 256;
  MTS_UNSUPPORTED(blocks <= 0x7fffffffLL, "%s: %lld destination rows are more than one launch covers", a.name, (long long)a.rows);
  const dim3 grid((unsigned)blocks), block(wide ? WAVES_PER_BLOCK * MTS_WAVE : 256);
  if (a.tab) {
    if (wide)
      hipLaunchKernelGGL(gather_tab_rows_kernel<Op>, grid, block, 0, a.st, (const S*)a.corpus, a.row_start, a.n_docs, a.doc_index,
                         a.tab->src_row, (T*)a.dst, a.rows, a.Lmax, U, a.pad16);
    else
      hipLaunchKernelGGL(gather_tab_thin_kernel<Op>, grid, block, 0, a.st, (const S*)a.corpus, a.row_start, a.n_docs, a.doc_index,
                         a.tab->src_row, (T*)a.dst, units, a.Lmax, U, a.pad16);
  } else if (!a.seg) {
    if (wide)
      hipLaunchKernelGGL(gather_rows_kernel<Op>, grid, block, 0, a.st, (const S*)a.corpus, a.row_start, a.n_docs, a.doc_index, (T*)a.dst, a.rows,
                         a.Lmax, U, a.pad16);
    else
      hipLaunchKernelGGL(gather_thin_kernel<Op>, grid, block, 0, a.st, (const S*)a.corpus, a.row_start, a.n_docs, a.doc_index, (T*)a.dst, units,
                         a.Lmax, U, a.pad16);
  } else if (wide) {
    hipLaunchKernelGGL(gather_seg_rows_kernel<Op>, grid, block, 0, a.st, (const S*)a.corpus, a.row_start, a.n_docs, a.doc_index, *a.seg,
                       (T*)a.dst, a.rows, a.Lmax, U, a.pad16);
  } else {
    if constexpr (std::is_same<Op, CopyOp<uint32_t>>::value) {
      if (a.seg->close_last) {
        hipLaunchKernelGGL((gather_seg_thin_kernel<Op, true>), grid, block, 0, a.st, (const S*)a.corpus, a.row_start, a.n_docs, a.doc_index,
                           *a.seg, (T*)a.dst, units, a.Lmax, U, a.pad16);
        MTS_LAUNCH_CHECK(a.name);
        return MTS_OK;
      }
    }
    hipLaunchKernelGGL((gather_seg_thin_kernel<Op, false>), grid, block, 0, a.st, (const S*)a.corpus, a.row_start, a.n_docs, a.doc_index, *a.seg,
                       (T*)a.dst, units, a.Lmax, U, a.pad16);
  }
  MTS_LAUNCH_CHECK(a.name);
  return MTS_OK;
}

// Argument checks, the pad pattern and the access width: one body for the three entry points.
int gather(const char* name, void* stream, int src_dtype, int dst_dtype, int B, int Lmax, int D, const void* corpus, const int64_t* row_start,
           int n_docs, const int32_t* doc_index, const SegTables* seg, const RowTable* tab, void* dst, float pad_value) {
  MTS_CHECK_ARG((src_dtype == MTS_F32 || src_dtype == MTS_BF16) && (dst_dtype == MTS_F32 || dst_dtype == MTS_BF16),
                "%s: dtypes must be fp32 or bf16 (got %d -> %d)", name, src_dtype, dst_dtype);
  MTS_CHECK_ARG(B >= 0 && Lmax >= 1 && D >= 1 && n_docs >= 1, "%s: bad shape (B %d, Lmax %d, D %d, n_docs %d)", name, B, Lmax, D, n_docs);
  MTS_CHECK_ARG(!seg || seg->n_listed >= 0, "%s: bad shape (n_listed %d)", name, seg ? seg->n_listed : 0);
  if (B == 0) return MTS_OK;
  MTS_CHECK_ARG(corpus && row_start && doc_index && dst, "%s: null pointer", name);
  MTS_CHECK_ARG(!tab || tab->src_row, "%s: null row table", name);
  MTS_CHECK_ARG(!seg || (seg->ptr && seg->dst_len && (seg->n_listed == 0 || (seg->dst_off && seg->src_off))), "%s: null segment table", name);
  MTS_CHECK_ARG(!seg || !seg->close_last || (D == 1 && src_dtype == MTS_F32 && dst_dtype == MTS_F32),
                "%s: close_last (the label rule) takes D = 1 in fp32 only (got D %d, %d -> %d)", name, D, src_dtype, dst_dtype);
  MTS_UNSUPPORTED(!(src_dtype == MTS_BF16 && dst_dtype == MTS_F32), "%s: bf16 -> fp32 is not covered (hold the corpus in fp32)", name);
  uint32_t pbits;
  memcpy(&pbits, &pad_value, 4);
  if (dst_dtype == MTS_BF16) {
    const uint32_t h = bf16_bits_rne(pbits) & 0xffffu;
    pbits = h | (h << 16);
  }
  const Args a = {name, (hipStream_t)stream, corpus, row_start, n_docs, doc_index, seg, tab, dst, (int64_t)B * Lmax, Lmax,
                  make_uint4(pbits, pbits, pbits, pbits)};
  const uintptr_t sa = (uintptr_t)corpus, da = (uintptr_t)dst;
  MTS_CHECK_ARG((sa & (src_dtype == MTS_F32 ? 3 : 1)) == 0 && (da & (dst_dtype == MTS_F32 ? 3 : 1)) == 0,
                "%s: corpus / dst not aligned to their element size", name);
  if (src_dtype == dst_dtype) {
    const int64_t row_bytes = (int64_t)D * (dst_dtype == MTS_F32 ? 4 : 2);
    const uintptr_t all = sa | da | (uintptr_t)row_bytes;
    MTS_CHECK_ARG(row_bytes / 2 <= 0x7fffffffLL, "%s: D %d too large", name, D);
    if ((all & 15) == 0) return launch<CopyOp<uint4>>(a, (int)(row_bytes / 16));
    if ((all & 7) == 0) return launch<CopyOp<uint2>>(a, (int)(row_bytes / 8));
    if ((all & 3) == 0) return launch<CopyOp<uint32_t>>(a, (int)(row_bytes / 4));
    return launch<CopyOp<uint16_t>>(a, (int)(row_bytes / 2));
  }
  // fp32 -> bf16
  if (D % 8 == 0 && (sa & 15) == 0 && (da & 15) == 0) return launch<CastOp<8>>(a, D / 8);
  if (D % 2 == 0 && (sa & 7) == 0 && (da & 3) == 0) return launch<CastOp<2>>(a, D / 2);
  return launch<CastOp<1>>(a, D);
}

}  // namespace

extern "C" int mts_gather_pad(void* stream, int src_dtype, int dst_dtype, int B, int Lmax, int D, const void* corpus, const int64_t* row_start,
                              int n_docs, const int32_t* doc_index, void* dst, float pad_value) {
  return gather("mts_gather_pad", stream, src_dtype, dst_dtype, B, Lmax, D, corpus, row_start, n_docs, doc_index, nullptr, nullptr, dst, pad_value);
}

extern "C" int mts_gather_rows(void* stream, int src_dtype, int dst_dtype, int B, int Lmax, int D, const void* corpus, const int64_t* row_start,
                               int n_docs, const int32_t* doc_index, const int32_t* src_row, void* dst, float pad_value) {
  const RowTable tab = {src_row};
  return gather("mts_gather_rows", stream, src_dtype, dst_dtype, B, Lmax, D, corpus, row_start, n_docs, doc_index, nullptr, &tab, dst, pad_value);
}

extern "C" int mts_gather_segments(void* stream, int src_dtype, int dst_dtype, int B, int Lmax, int D, const void* corpus,
                                   const int64_t* row_start, int n_docs, const int32_t* doc_index, const int32_t* seg_ptr,
                                   const int32_t* seg_dst, const int32_t* seg_src, int n_listed, const int32_t* dst_len,
                                   const int32_t* close_last, void* dst, float pad_value) {
  const SegTables seg = {seg_ptr, seg_dst, seg_src, dst_len, close_last, n_listed};
  return gather("mts_gather_segments", stream, src_dtype, dst_dtype, B, Lmax, D, corpus, row_start, n_docs, doc_index, &seg, nullptr, dst,
                pad_value);
}
