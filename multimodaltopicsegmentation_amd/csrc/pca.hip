// PCA projection of the resident corpus (reference: --pca_reduce / --pca_value, EncoderDataset.py:49-70, sklearn's PCA fitted on the
// training split and applied to all three): the device half.  The corpus is one row-major [rows, D] matrix in fp32 or bf16; the fit
// needs its column sums and the centred Gram matrix G = sum_r (x_r - c)(x_r - c)^T, the transform the centred projection
// y = (x - c) W^T.  Neither maps onto the GEMMs of gemm.hip: X^T X - N mu mu^T cancels in fp32 when a column's mean is many times its
// spread, and a centred bf16 value is no bf16 value.  So here a staged element is upcast to fp32 and the centre subtracted ONCE, in fp32,
// on its way into LDS; products and sums run on the fp32-input matrix instruction (v_mfma_f32_32x32x2_f32: exact fp32, bit for bit a
// k-ordered fmaf chain); the Gram kernel folds its fp32 accumulators into fp64 after every PCA_SLICE rows, so the fp32 chain never grows
// past PCA_SLICE terms whatever the corpus' length.
//
// Mapping, all three kernels 256 threads, no atomics, no workspace, no dependence between workgroups, every output element written
// exactly once by a plain vector store -- the same inputs give the same bits:
//   colsum   a workgroup owns PCA_SUM_COLS columns for all rows: 16 x 16 threads, a thread adds every 16th row of its column in fp64, the
//            16 partial sums of a column are added in a fixed order through LDS.
//   gram     a workgroup owns a PCA_TILE x PCA_TILE tile of G on or above the diagonal for ALL rows (tiles below it return at once) and
//            writes the tile and its mirror: G is exactly symmetric.  PCA_GRAM_KC rows of the tile's two column panels are staged per trip
//            as zs[row][column] (lanes 0..31 of an operand read one staged row, lanes 32..63 the next: no bank conflict); the next
//            trip's elements are already in registers while the matrix cores work.  Four waves, a 32 x 32 quarter each.  A diagonal
//            tile stages one panel and only writes i <= j and its mirror.
//   project  a workgroup owns PCA_TILE rows x PCA_TILE components; the D columns are walked PCA_KC at a time, x (centred) and W staged
//            as [row][PCA_KC + 1] (the odd stride keeps the operand reads, 32 rows of one column, on 32 banks).  One fp32 chain over D
//            (D <= 4096), one rounding to the output dtype.
// Rows, columns and components beyond the edge are staged as 0 (AFTER the centring: a pad is 0, not -c) and never stored.
// A staging load is issued at an address clamped into the matrix, with no branch round it, and is masked and centred when it is stored to
// LDS: with a branch round every load a trip's loads waited for one another (Gram at 33 179 x 1792: 5.6 ms, now 2.5 ms, same bits).
#include "common.h"

namespace {

constexpr int PCA_SLICE = 1024;      // rows after which the Gram kernel's fp32 accumulators are folded into fp64 and restarted
constexpr int PCA_TILE = 64;         // edge of a workgroup's output tile (gram: columns x columns, project: rows x components)
constexpr int PCA_KC = 32;           // columns of x and W the projection stages per trip
constexpr int PCA_GRAM_KC = 64;      // rows the Gram kernel stages per trip: 32 matrix instructions per wave between two barriers
constexpr int PCA_THREADS = 256;
constexpr int PCA_SUM_COLS = 16;     // columns of a colsum workgroup; PCA_THREADS / PCA_SUM_COLS row lanes
constexpr int PCA_SUM_LANES = PCA_THREADS / PCA_SUM_COLS;
constexpr int PCA_MAX_D = 4096;      // the fp64 Gram matrix is D * D * 8 bytes
static_assert(PCA_SLICE % PCA_GRAM_KC == 0, "a fold falls between two staged trips");
static_assert(PCA_THREADS == 4 * MTS_WAVE && PCA_TILE == 64, "four waves, a 32 x 32 quarter of the tile each");

template <typename T>
__global__ __launch_bounds__(PCA_THREADS) void pca_colsum_kernel(const T* __restrict__ x, int rows, int D, double* __restrict__ out) {
  __shared__ double part[PCA_SUM_LANES][PCA_SUM_COLS];
  const int c = threadIdx.x % PCA_SUM_COLS, q = threadIdx.x / PCA_SUM_COLS;
  const int col = blockIdx.x * PCA_SUM_COLS + c;
  double s = 0.0;
  if (col < D) {
    const T* __restrict__ p = x + col;
#pragma unroll 4
    for (int64_t r = q; r < rows; r += PCA_SUM_LANES) s += (double)to_f32(p[r * D]);
  }
  part[q][c] = s;
  __syncthreads();
  if (q == 0 && col < D) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < PCA_SUM_LANES; ++k) t += part[k][c];
    out[col] = t;
  }
}

__device__ __forceinline__ int64_t pca_min64(int64_t a, int64_t b) { return a < b ? a : b; }

// C/D map of the 32x32 matrix instruction: register g of lane l holds row (g & 3) + 8 * (g >> 2) + 4 * (l >> 5), column l & 31
__device__ __forceinline__ int pca_acc_row(int g, int lane) { return (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5); }

template <typename T>
__global__ __launch_bounds__(PCA_THREADS) void pca_gram_kernel(const T* __restrict__ x, int rows, int D, const float* __restrict__ center,
                                                               double* __restrict__ G) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (ti > tj) return;  // the mirror is the upper tile's work
  __shared__ float zs[2][PCA_GRAM_KC][PCA_TILE];  // the row panel's columns, the column panel's columns (unused by a diagonal tile)
  const bool diag = ti == tj;
  const int tid = threadIdx.x, lane = tid & (MTS_WAVE - 1), wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;
  const bool computes = !(diag && wi > wj);  // the quarter below the diagonal of a diagonal tile is never stored
  const int i0 = ti * PCA_TILE, j0 = tj * PCA_TILE;
  // staging: a thread owns one column of each panel and every fourth row of the trip
  constexpr int SR = PCA_THREADS / PCA_TILE, SP = PCA_GRAM_KC / SR;
  const int sc = tid % PCA_TILE, sr = tid / PCA_TILE;
  const int ca = i0 + sc, cb = j0 + sc;
  const bool a_ok = ca < D, b_ok = !diag && cb < D;
  // every load is issued at a clamped (valid) address, with no branch round it, and masked and centred only when it is stored to LDS a
  // trip later: a trip's loads are in flight together, behind the matrix instructions of the trip before
  const int cca = min(ca, D - 1), ccb = min(cb, D - 1);
  const float cen_a = center[cca], cen_b = center[ccb];
  const T* __restrict__ xa = x + cca;
  const T* __restrict__ xb = x + ccb;
  const int64_t last = (int64_t)rows - 1;
  float ra[SP], rb[SP];
#pragma unroll
  for (int p = 0; p < SP; ++p) rb[p] = 0.0f;
  auto fetch = [&](int64_t r0) {
#pragma unroll
    for (int p = 0; p < SP; ++p) ra[p] = to_f32(xa[pca_min64(r0 + sr + p * SR, last) * D]);
    if (!diag) {
#pragma unroll
      for (int p = 0; p < SP; ++p) rb[p] = to_f32(xb[pca_min64(r0 + sr + p * SR, last) * D]);
    }
  };
  f32x16 acc;
  double acc64[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    acc[g] = 0.0f;
    acc64[g] = 0.0;
  }
  const int pb = diag ? 0 : 1;
  const int arow = lane >> 5, acol = wi * 32 + (lane & 31), bcol = wj * 32 + (lane & 31);
  int in_slice = 0;
  fetch(0);
  for (int64_t r0 = 0; r0 < rows; r0 += PCA_GRAM_KC) {  // the trip count is uniform over the workgroup: every barrier is reached by all
    __syncthreads();                               // the last trip's operands have been read
#pragma unroll
    for (int p = 0; p < SP; ++p) {
      const bool in = r0 + sr + p * SR < rows;
      zs[0][sr + p * SR][sc] = (a_ok && in) ? ra[p] - cen_a : 0.0f;
      if (!diag) zs[1][sr + p * SR][sc] = (b_ok && in) ? rb[p] - cen_b : 0.0f;
    }
    __syncthreads();
    if (r0 + PCA_GRAM_KC < rows) fetch(r0 + PCA_GRAM_KC);
    if (computes) {
#pragma unroll
      for (int kk = 0; kk < PCA_GRAM_KC; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(zs[0][kk + arow][acol], zs[pb][kk + arow][bcol], acc, 0, 0, 0);
    }
    in_slice += PCA_GRAM_KC;
    if (in_slice == PCA_SLICE) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        acc64[g] += (double)acc[g];
        acc[g] = 0.0f;
      }
      in_slice = 0;
    }
  }
  if (!computes) return;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const double v = acc64[g] + (double)acc[g];  // the last, partial slice (0 when the rows are a multiple of PCA_SLICE)
    const int gi = i0 + wi * 32 + pca_acc_row(g, lane), gj = j0 + bcol;
    if (gi >= D || gj >= D) continue;
    if (!diag) {
      G[(int64_t)gi * D + gj] = v;
      G[(int64_t)gj * D + gi] = v;
    } else if (gi <= gj) {
      G[(int64_t)gi * D + gj] = v;
      if (gi < gj) G[(int64_t)gj * D + gi] = v;
    }
  }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(PCA_THREADS) void pca_project_kernel(const TI* __restrict__ x, int rows, int D, int k,
                                                                  const float* __restrict__ center, const float* __restrict__ w,
                                                                  TO* __restrict__ y) {
  __shared__ float zs[PCA_TILE][PCA_KC + 1];
  __shared__ float ws[PCA_TILE][PCA_KC + 1];
  const int tid = threadIdx.x, lane = tid & (MTS_WAVE - 1), wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;
  const int64_t r0 = (int64_t)blockIdx.x * PCA_TILE;
  const int j0 = blockIdx.y * PCA_TILE;
  const bool computes = r0 + wi * 32 < rows && j0 + wj * 32 < k;
  // staging: a thread owns one of the trip's columns and every eighth row of both operands
  constexpr int SR = PCA_THREADS / PCA_KC, SP = PCA_TILE / SR;
  const int sd = tid % PCA_KC, sr = tid / PCA_KC;
  // loads at clamped (valid) addresses with no branch round them; masked and centred when they are stored to LDS a trip later
  const int64_t last = (int64_t)rows - 1;
  float rz[SP], rw[SP], cen = 0.0f;
  auto fetch = [&](int d0) {
    const int dc = min(d0 + sd, D - 1);
    cen = center[dc];
#pragma unroll
    for (int p = 0; p < SP; ++p) {
      rz[p] = to_f32(x[pca_min64(r0 + sr + p * SR, last) * D + dc]);
      rw[p] = w[(int64_t)min(j0 + sr + p * SR, k - 1) * D + dc];
    }
  };
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
  const int arow = wi * 32 + (lane & 31), brow = wj * 32 + (lane & 31), kcol = lane >> 5;
  fetch(0);
  for (int d0 = 0; d0 < D; d0 += PCA_KC) {
    __syncthreads();
#pragma unroll
    for (int p = 0; p < SP; ++p) {
      const bool d_ok = d0 + sd < D;
      zs[sr + p * SR][sd] = (d_ok && r0 + sr + p * SR < rows) ? rz[p] - cen : 0.0f;
      ws[sr + p * SR][sd] = (d_ok && j0 + sr + p * SR < k) ? rw[p] : 0.0f;
    }
    __syncthreads();
    if (d0 + PCA_KC < D) fetch(d0 + PCA_KC);
    if (computes) {
#pragma unroll
      for (int kk = 0; kk < PCA_KC; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(zs[arow][kk + kcol], ws[brow][kk + kcol], acc, 0, 0, 0);
    }
  }
  if (!computes) return;
  const int gj = j0 + brow;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int64_t gr = r0 + wi * 32 + pca_acc_row(g, lane);
    if (gr < rows && gj < k) y[gr * k + gj] = from_f32<TO>(acc[g]);
  }
}

int pca_check_shape(const char* who, int dtype, int rows, int D) {
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "%s: unknown dtype %d", who, dtype);
  MTS_CHECK_ARG(rows >= 1 && D >= 1, "%s: bad shape (rows %d, D %d)", who, rows, D);
  return MTS_OK;
}

}  // namespace

extern "C" int mts_pca_colsum(void* stream, int dtype, int rows, int D, const void* x, double* sum_out) {
  if (int rc = pca_check_shape("mts_pca_colsum", dtype, rows, D)) return rc;
  MTS_CHECK_ARG(x && sum_out, "mts_pca_colsum: null pointer");
  MTS_UNSUPPORTED(D <= PCA_MAX_D, "mts_pca_colsum: D %d is above %d", D, PCA_MAX_D);
  const dim3 grid((unsigned)ceil_div(D, PCA_SUM_COLS));
  if (dtype == MTS_F32)
    hipLaunchKernelGGL(pca_colsum_kernel<float>, grid, dim3(PCA_THREADS), 0, (hipStream_t)stream, (const float*)x, rows, D, sum_out);
  else
    hipLaunchKernelGGL(pca_colsum_kernel<bf16_t>, grid, dim3(PCA_THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, rows, D, sum_out);
  MTS_LAUNCH_CHECK("mts_pca_colsum");
  return MTS_OK;
}

extern "C" int mts_pca_gram(void* stream, int dtype, int rows, int D, const void* x, const float* center, double* gram_out) {
  if (int rc = pca_check_shape("mts_pca_gram", dtype, rows, D)) return rc;
  MTS_CHECK_ARG(x && center && gram_out, "mts_pca_gram: null pointer");
  MTS_UNSUPPORTED(D <= PCA_MAX_D, "mts_pca_gram: D %d is above %d (the fp64 Gram matrix is D * D * 8 bytes)", D, PCA_MAX_D);
  const unsigned nt = (unsigned)ceil_div(D, PCA_TILE);
  const dim3 grid(nt, nt);
  if (dtype == MTS_F32)
    hipLaunchKernelGGL(pca_gram_kernel<float>, grid, dim3(PCA_THREADS), 0, (hipStream_t)stream, (const float*)x, rows, D, center, gram_out);
  else
    hipLaunchKernelGGL(pca_gram_kernel<bf16_t>, grid, dim3(PCA_THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, rows, D, center, gram_out);
  MTS_LAUNCH_CHECK("mts_pca_gram");
  return MTS_OK;
}

extern "C" int mts_pca_project(void* stream, int in_dtype, int out_dtype, int rows, int D, int k, const void* x, const float* center,
                               const float* w, void* y) {
  if (int rc = pca_check_shape("mts_pca_project", in_dtype, rows, D)) return rc;
  MTS_CHECK_ARG(out_dtype == MTS_F32 || out_dtype == MTS_BF16, "mts_pca_project: unknown output dtype %d", out_dtype);
  MTS_CHECK_ARG(k >= 1 && k <= D, "mts_pca_project: k %d is outside 1 .. D = %d", k, D);
  MTS_CHECK_ARG(x && center && w && y, "mts_pca_project: null pointer");
  MTS_UNSUPPORTED(D <= PCA_MAX_D, "mts_pca_project: D %d is above %d", D, PCA_MAX_D);
  MTS_UNSUPPORTED(!(in_dtype == MTS_BF16 && out_dtype == MTS_F32), "mts_pca_project: bf16 -> fp32 is not offered (fp32 -> fp32, bf16 -> bf16, fp32 -> bf16)");
  const dim3 grid((unsigned)ceil_div(rows, PCA_TILE), (unsigned)ceil_div(k, PCA_TILE));
  const dim3 block(PCA_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (in_dtype == MTS_F32 && out_dtype == MTS_F32)
    hipLaunchKernelGGL((pca_project_kernel<float, float>), grid, block, 0, s, (const float*)x, rows, D, k, center, w, (float*)y);
  else if (in_dtype == MTS_F32)
    hipLaunchKernelGGL((pca_project_kernel<float, bf16_t>), grid, block, 0, s, (const float*)x, rows, D, k, center, w, (bf16_t*)y);
  else
    hipLaunchKernelGGL((pca_project_kernel<bf16_t, bf16_t>), grid, block, 0, s, (const bf16_t*)x, rows, D, k, center, w, (bf16_t*)y);
  MTS_LAUNCH_CHECK("mts_pca_project");
  return MTS_OK;
}
