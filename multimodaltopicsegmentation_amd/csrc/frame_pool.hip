// Sentence pooling of frame-level audio features (frames.ResidentFrames; reference: extract_embeddings.py:644-667, which keeps every
// sentence's frame-level encoder output and writes six pooled variants of it: _mean, _max, _mean_std, _max_std, _last, _delta_gap).  The
// frames of a whole corpus lie in HBM as one row-major [total_frames, D] matrix in fp32 or bf16; sentence s is the rows
// frame_start[s] .. frame_start[s + 1].  A ragged segmented reduction: every frame is needed once, every output row once.
//
// Arithmetic of mts_frame_pool, per sentence of n frames and per column (the tests' bounds are derived from these lines alone).  An element
// is upcast to fp32 ONCE; everything below is fp32, every operation correctly rounded (no contraction; `/` and sqrtf are the compiler's
// correctly rounded forms -- the __fdiv_rn / __fsqrt_rn spellings are NOT: they lower to the native approximations):
//   m   = fl(fl(sum_r x_r) / n)                                           the mean
//   max = max_r x_r                                                       exact
//   std = fl(sqrt(fl(fl(sum_r fl(fl(x_r - m)^2)) / n)))                   the population deviation ABOUT THE COMPUTED MEAN m: two passes in
//                                                                         meaning, as np.std
// Order of a sum (fixed, so the same inputs give the same bits): wave w of the workgroup's four adds the sentence's rows w, w + 4, w + 8,
// .. in ascending order into ONE chain per column; the four chains are added as ((p0 + p1) + p2) + p3.  A wave without a row adds 0.
//
// Mapping.  One workgroup of FP_WAVES = 4 waves owns one (sentence, column tile); the grid is sentences x column tiles, consecutive
// workgroups hold the tiles of one sentence.  A lane owns VEC consecutive columns and moves them with one 16-byte access (VEC = 4 fp32 /
// 8 bf16) when D is a multiple of VEC and the matrix is 16-byte aligned; any other width or alignment takes VEC = 1 (a wave then reads
// 256 / 128 contiguous bytes per row): every D >= 1 works.  The sentence's first row is a wave-uniform value, so the table is read by
// scalar loads and a row's address is formed in 64 bits ((first + r) * D exceeds 2^31 on real data).
// A wave has FP_ROWS = 8 rows in flight before it accumulates them: the loads are issued at an address clamped into the sentence with no
// branch round them and masked by a wave-uniform test when they are added.
// The second pass (the squared deviations need m, which needs every row) gets its data
//   * from REGISTERS for the first FP_ROWS rows of every wave -- a sentence of up to FP_WAVES * FP_ROWS = 32 frames is read once;
//   * by a RE-READ for the rows behind them: the same wave reads the same addresses again a few microseconds later (60 frames x 512 x 4 B
//     = 120 KB per sentence, in reach of the 4 MiB L2 of the XCD and of the 256 MiB Infinity Cache behind it).
// The waves' partial results meet in LDS ([wave][element][lane]: consecutive lanes on consecutive banks), every thread adds them in the
// fixed order, wave 0 puts the tile's results into LDS and all 256 threads store them: consecutive lanes write consecutive elements of
// the output row, whatever ld_out and the output's alignment are.  No atomics, no workspace, no workgroup depends on another, every
// element of the block written exactly once by a plain vector store, nothing outside the block touched.  A sentence without frames
// (or a table that runs backwards there) writes 0; table entries are clamped into 0 .. total_frames before an address is formed.
//
// mts_frame_edges is the two gathers: one workgroup per sentence, a thread per column, the rows wave-uniform.
#include "common.h"

namespace {

constexpr int FP_WAVES = 4;
constexpr int FP_THREADS = FP_WAVES * MTS_WAVE;
constexpr int FP_ROWS = 8;  // rows a wave has in flight; the first FP_ROWS of a wave stay in registers for the second pass

// what a lane holds of one row: VEC elements as they are stored
template <typename T, int VEC> struct FrameVec;
template <> struct FrameVec<float, 4> {
  uint4 v;
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ float get(int i) const { return __uint_as_float((&v.x)[i]); }
};
template <> struct FrameVec<bf16_t, 8> {
  uint4 v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ float get(int i) const {
    const uint32_t u = (&v.x)[i >> 1];
    return (i & 1) ? bf16_hi(u) : bf16_lo(u);
  }
};
template <typename T> struct FrameVec<T, 1> {
  T v;
  __device__ __forceinline__ void load(const T* p) { v = *p; }
  __device__ __forceinline__ float get(int) const { return to_f32(v); }
};

__device__ __forceinline__ int64_t fp_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int64_t fp_min64(int64_t a, int64_t b) { return a < b ? a : b; }

__device__ __forceinline__ void fp_store(void* out, int out_dtype, int64_t at, float v) {
  if (out_dtype == MTS_F32)
    reinterpret_cast<float*>(out)[at] = v;
  else
    reinterpret_cast<bf16_t*>(out)[at] = from_f32<bf16_t>(v);
}

template <typename T, int VEC>
__global__ __launch_bounds__(FP_THREADS) void frame_pool_kernel(const T* __restrict__ frames, int64_t total_frames,
                                                                const int64_t* __restrict__ frame_start, int D, int tiles, int first,
                                                                int with_std, void* __restrict__ out, int out_dtype, int64_t ld_out) {
  constexpr int TILE = MTS_WAVE * VEC;
  __shared__ float p_sum[FP_WAVES][VEC][MTS_WAVE];
  __shared__ float p_max[FP_WAVES][VEC][MTS_WAVE];
  __shared__ float p_sq[FP_WAVES][VEC][MTS_WAVE];
  __shared__ float res[2][TILE];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & (MTS_WAVE - 1);
  const int s = (int)(blockIdx.x / (unsigned)tiles);
  const int c0 = (int)(blockIdx.x - (unsigned)s * (unsigned)tiles) * TILE;
  const int width = min(TILE, D - c0);  // columns of this tile: 1 .. TILE, a multiple of VEC
  const int64_t f0 = fp_clamp(frame_start[s], total_frames);
  const int64_t n = fp_clamp(frame_start[s + 1], total_frames) - f0;
  const int64_t o0 = (int64_t)s * ld_out + c0;
  const int blocks_out = (first != MTS_POOL_NONE ? 1 : 0) + (with_std ? 1 : 0);
  if (n <= 0) {  // uniform over the workgroup
    for (int k = 0; k < blocks_out; ++k)
      for (int j = tid; j < width; j += FP_THREADS) fp_store(out, out_dtype, o0 + (int64_t)k * D + j, 0.0f);
    return;
  }
  const bool col_ok = lane * VEC < width;
  // a lane beyond the tile's width reads the tile's first columns (a valid address) and is never stored
  const T* __restrict__ base = frames + f0 * D + c0 + (col_ok ? lane * VEC : 0);
  const int64_t last = n - 1;
  const float fn = (float)n;

  float sum[VEC], mx[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    sum[j] = 0.0f;
    mx[j] = -INFINITY;
  }
  // ---- pass 1: the wave's rows wave, wave + 4, ..; the first FP_ROWS of them stay in `head`
  FrameVec<T, VEC> head[FP_ROWS];
#pragma unroll
  for (int k = 0; k < FP_ROWS; ++k) head[k].load(base + fp_min64((int64_t)wave + k * FP_WAVES, last) * D);
#pragma unroll
  for (int k = 0; k < FP_ROWS; ++k) {
    if ((int64_t)wave + k * FP_WAVES < n) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float x = head[k].get(j);
        sum[j] = __fadd_rn(sum[j], x);
        mx[j] = fmaxf(mx[j], x);
      }
    }
  }
  for (int64_t r0 = (int64_t)wave + FP_ROWS * FP_WAVES; r0 < n; r0 += FP_ROWS * FP_WAVES) {
    FrameVec<T, VEC> t[FP_ROWS];
#pragma unroll
    for (int k = 0; k < FP_ROWS; ++k) t[k].load(base + fp_min64(r0 + k * FP_WAVES, last) * D);
#pragma unroll
    for (int k = 0; k < FP_ROWS; ++k) {
      if (r0 + k * FP_WAVES < n) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float x = t[k].get(j);
          sum[j] = __fadd_rn(sum[j], x);
          mx[j] = fmaxf(mx[j], x);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    p_sum[wave][j][lane] = sum[j];
    p_max[wave][j][lane] = mx[j];
  }
  __syncthreads();
  float mean[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    float t = p_sum[0][j][lane], m = p_max[0][j][lane];
#pragma unroll
    for (int w = 1; w < FP_WAVES; ++w) {
      t = __fadd_rn(t, p_sum[w][j][lane]);
      m = fmaxf(m, p_max[w][j][lane]);
    }
    mean[j] = t / fn;
    mx[j] = m;
  }
  // ---- pass 2: squared deviations about the computed mean, the same rows in the same order
  float dev[VEC];
  if (with_std) {
    float sq[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) sq[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < FP_ROWS; ++k) {
      if ((int64_t)wave + k * FP_WAVES < n) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float d = __fsub_rn(head[k].get(j), mean[j]);
          sq[j] = __fadd_rn(sq[j], __fmul_rn(d, d));
        }
      }
    }
    for (int64_t r0 = (int64_t)wave + FP_ROWS * FP_WAVES; r0 < n; r0 += FP_ROWS * FP_WAVES) {
      FrameVec<T, VEC> t[FP_ROWS];
#pragma unroll
      for (int k = 0; k < FP_ROWS; ++k) t[k].load(base + fp_min64(r0 + k * FP_WAVES, last) * D);
#pragma unroll
      for (int k = 0; k < FP_ROWS; ++k) {
        if (r0 + k * FP_WAVES < n) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            const float d = __fsub_rn(t[k].get(j), mean[j]);
            sq[j] = __fadd_rn(sq[j], __fmul_rn(d, d));
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) p_sq[wave][j][lane] = sq[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float t = p_sq[0][j][lane];
#pragma unroll
      for (int w = 1; w < FP_WAVES; ++w) t = __fadd_rn(t, p_sq[w][j][lane]);
      dev[j] = sqrtf(t / fn);
    }
  }
  // ---- the tile's results through LDS, so that consecutive lanes store consecutive elements
  if (wave == 0 && col_ok) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      res[0][lane * VEC + j] = first == MTS_POOL_MAX ? mx[j] : mean[j];
      if (with_std) res[1][lane * VEC + j] = dev[j];
    }
  }
  __syncthreads();
  int k = 0;
  if (first != MTS_POOL_NONE) {
    for (int j = tid; j < width; j += FP_THREADS) fp_store(out, out_dtype, o0 + j, res[0][j]);
    k = 1;
  }
  if (with_std)
    for (int j = tid; j < width; j += FP_THREADS) fp_store(out, out_dtype, o0 + (int64_t)k * D + j, res[1][j]);
}

template <typename T>
__global__ __launch_bounds__(FP_THREADS) void frame_edges_kernel(const T* __restrict__ frames, int64_t total_frames,
                                                                 const int64_t* __restrict__ frame_start, const uint8_t* __restrict__ doc_last,
                                                                 int n_sent, int D, int mode, void* __restrict__ out, int out_dtype,
                                                                 int64_t ld_out) {
  const int s = (int)blockIdx.x;
  const int64_t f0 = fp_clamp(frame_start[s], total_frames);
  const int64_t f1 = fp_clamp(frame_start[s + 1], total_frames);
  const int64_t o0 = (int64_t)s * ld_out;
  if (f1 <= f0) {
    for (int j = threadIdx.x; j < D; j += FP_THREADS) fp_store(out, out_dtype, o0 + j, 0.0f);
    return;
  }
  const T* __restrict__ lastp = frames + (f1 - 1) * D;
  // the next sentence's first frame is row f1 of the matrix; the corpus' last sentence has none whatever its flag says
  const bool gap = mode == MTS_EDGE_DELTA_GAP && s + 1 < n_sent && f1 < total_frames && !doc_last[s];
  const T* __restrict__ nextp = frames + (gap ? f1 : f1 - 1) * D;
  for (int j = threadIdx.x; j < D; j += FP_THREADS) {
    const float e = to_f32(lastp[j]);
    fp_store(out, out_dtype, o0 + j, gap ? __fsub_rn(to_f32(nextp[j]), e) : e);
  }
}

int frame_check(const char* who, int in_dtype, int out_dtype, int n_sent, int D, const void* frames, int64_t total_frames,
                const int64_t* frame_start, const void* out, int64_t ld_out, int64_t block) {
  MTS_CHECK_ARG((in_dtype == MTS_F32 || in_dtype == MTS_BF16) && (out_dtype == MTS_F32 || out_dtype == MTS_BF16),
                "%s: dtypes must be fp32 or bf16 (got %d -> %d)", who, in_dtype, out_dtype);
  MTS_CHECK_ARG(n_sent >= 1 && D >= 1 && total_frames >= 0, "%s: bad shape (n_sent %d, D %d, total_frames %lld)", who, n_sent, D,
                (long long)total_frames);
  MTS_CHECK_ARG(frames && frame_start && out, "%s: null pointer", who);
  MTS_CHECK_ARG(ld_out >= block, "%s: ld_out %lld is smaller than the %lld columns written", who, (long long)ld_out, (long long)block);
  MTS_CHECK_ARG(((uintptr_t)frames & (in_dtype == MTS_F32 ? 3 : 1)) == 0 && ((uintptr_t)out & (out_dtype == MTS_F32 ? 3 : 1)) == 0,
                "%s: frames / out not aligned to their element size", who);
  return MTS_OK;
}

template <typename T, int VEC>
int launch_pool(hipStream_t st, const void* frames, int64_t total_frames, const int64_t* frame_start, int n_sent, int D, int first,
                int with_std, void* out, int out_dtype, int64_t ld_out) {
  const int tiles = ceil_div(D, MTS_WAVE * VEC);
  const int64_t blocks = (int64_t)n_sent * tiles;
  MTS_UNSUPPORTED(blocks <= 0x7fffffffLL, "mts_frame_pool: %d sentences x %d column tiles are more than one launch covers", n_sent, tiles);
  hipLaunchKernelGGL((frame_pool_kernel<T, VEC>), dim3((unsigned)blocks), dim3(FP_THREADS), 0, st, (const T*)frames, total_frames,
                     frame_start, D, tiles, first, with_std, out, out_dtype, ld_out);
  MTS_LAUNCH_CHECK("mts_frame_pool");
  return MTS_OK;
}

}  // namespace

extern "C" int mts_frame_pool(void* stream, int in_dtype, int out_dtype, int n_sent, int D, int first, int with_std, const void* frames,
                              int64_t total_frames, const int64_t* frame_start, void* out, int64_t ld_out) {
  MTS_CHECK_ARG(first == MTS_POOL_NONE || first == MTS_POOL_MEAN || first == MTS_POOL_MAX, "mts_frame_pool: unknown first statistic %d", first);
  MTS_CHECK_ARG(with_std == 0 || with_std == 1, "mts_frame_pool: with_std is 0 or 1, not %d", with_std);
  MTS_CHECK_ARG(first != MTS_POOL_NONE || with_std, "mts_frame_pool: nothing to compute (no first statistic and no deviation)");
  const int64_t block = (int64_t)D * ((first != MTS_POOL_NONE ? 1 : 0) + with_std);
  if (int rc = frame_check("mts_frame_pool", in_dtype, out_dtype, n_sent, D, frames, total_frames, frame_start, out, ld_out, block)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool wide = ((uintptr_t)frames & 15) == 0;
  if (in_dtype == MTS_F32) {
    if (wide && D % 4 == 0) return launch_pool<float, 4>(st, frames, total_frames, frame_start, n_sent, D, first, with_std, out, out_dtype, ld_out);
    return launch_pool<float, 1>(st, frames, total_frames, frame_start, n_sent, D, first, with_std, out, out_dtype, ld_out);
  }
  if (wide && D % 8 == 0) return launch_pool<bf16_t, 8>(st, frames, total_frames, frame_start, n_sent, D, first, with_std, out, out_dtype, ld_out);
  return launch_pool<bf16_t, 1>(st, frames, total_frames, frame_start, n_sent, D, first, with_std, out, out_dtype, ld_out);
}

extern "C" int mts_frame_edges(void* stream, int in_dtype, int out_dtype, int n_sent, int D, int mode, const void* frames,
                               int64_t total_frames, const int64_t* frame_start, const uint8_t* doc_last, void* out, int64_t ld_out) {
  MTS_CHECK_ARG(mode == MTS_EDGE_LAST || mode == MTS_EDGE_DELTA_GAP, "mts_frame_edges: unknown mode %d", mode);
  if (int rc = frame_check("mts_frame_edges", in_dtype, out_dtype, n_sent, D, frames, total_frames, frame_start, out, ld_out, D)) return rc;
  MTS_CHECK_ARG(mode == MTS_EDGE_LAST || doc_last, "mts_frame_edges: delta_gap needs the last-of-document flags");
  const dim3 grid((unsigned)n_sent), block(FP_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == MTS_F32)
    hipLaunchKernelGGL(frame_edges_kernel<float>, grid, block, 0, st, (const float*)frames, total_frames, frame_start, doc_last, n_sent, D, mode,
                       out, out_dtype, ld_out);
  else
    hipLaunchKernelGGL(frame_edges_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)frames, total_frames, frame_start, doc_last, n_sent, D, mode,
                       out, out_dtype, ld_out);
  MTS_LAUNCH_CHECK("mts_frame_edges");
  return MTS_OK;
}
