// Gated merge of the two late-fusion encoders (BiLSTMLateFusion(merge='gate'); an extension, the reference only concatenates) for gfx950.
//
//   z = sigmoid(a)         a = [h1 ; h2] W_g^T + b_g: the gate's pre-activation, produced by two mts_gemm calls
//   m = z h1 + (1 - z) h2  (= h2 + z (h1 - h2); this form is exact at saturation: z = 1 gives h1, z = 0 gives h2, bit for bit)
//
//   backward, given dm (z recomputed from a, never stored):
//   dh1 = dm z       dh2 = dm - dm z       da = dm (h1 - h2) z (1 - z)
//   (the parts of dh1 / dh2 that come through a, da W_g, are added by the data-gradient GEMMs that follow)
//
// Pure streaming, no reuse: 4 (forward) / 7 (backward) passes of rows x W elements, fp32 arithmetic, every output rounded once.  A
// thread owns one vector of a row and strides over the rows: the block is a power-of-two number of lanes along the columns (up to 64:
// 1 KiB per wave-row) by 256 / that many rows, so there is no division in the index arithmetic and every offset is 64-bit.  16 bytes per
// lane when W, the leading dimensions and the bases allow (always in fp32; bf16: multiples of 8 elements), else 4 elements per lane.
// No atomics, no workspace, no LDS, one launch each.  sigmoid = 1 / (1 + expf(-a)): expf overflows to +Inf (z = 0) and underflows to 0
// (z = 1), so |a| = 1e4 saturates exactly, da is then an exact 0, and no NaN / Inf comes from a finite input.
#include <algorithm>
#include "common.h"

#define GATE_THREADS 256
#define GATE_MAX_BLOCKS 2048     // 8 workgroups of 4 waves per CU: every wave slot of the 256 CUs (the kernels need < 64 VGPRs)

template <typename T, int VEC> __device__ __forceinline__ void gate_load(const T* p, float (&o)[VEC]);
template <> __device__ __forceinline__ void gate_load<float, 4>(const float* p, float (&o)[4]) { load4<float>(p, o); }
template <> __device__ __forceinline__ void gate_load<bf16_t, 4>(const bf16_t* p, float (&o)[4]) { load4<bf16_t>(p, o); }
template <> __device__ __forceinline__ void gate_load<bf16_t, 8>(const bf16_t* p, float (&o)[8]) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  o[0] = bf16_lo(v.x); o[1] = bf16_hi(v.x); o[2] = bf16_lo(v.y); o[3] = bf16_hi(v.y);
  o[4] = bf16_lo(v.z); o[5] = bf16_hi(v.z); o[6] = bf16_lo(v.w); o[7] = bf16_hi(v.w);
}
template <typename T, int VEC> __device__ __forceinline__ void gate_store(T* p, const float (&o)[VEC]);
template <> __device__ __forceinline__ void gate_store<float, 4>(float* p, const float (&o)[4]) { store4<float>(p, o); }
template <> __device__ __forceinline__ void gate_store<bf16_t, 4>(bf16_t* p, const float (&o)[4]) { store4<bf16_t>(p, o); }
template <> __device__ __forceinline__ void gate_store<bf16_t, 8>(bf16_t* p, const float (&o)[8]) {
  uint4 v;
  v.x = pack_bf16x2(o[0], o[1]); v.y = pack_bf16x2(o[2], o[3]); v.z = pack_bf16x2(o[4], o[5]); v.w = pack_bf16x2(o[6], o[7]);
  *reinterpret_cast<uint4*>(p) = v;
}

// lanes_log2: log2 of the block's extent along the columns; thread (x, y) owns columns [VEC (blockIdx.x * lanes + x), + VEC) of rows
// blockIdx.y * rpb + y, + gridDim.y * rpb, ..
template <typename T, int VEC>
__global__ __launch_bounds__(GATE_THREADS) void gate_merge_fwd_kernel(size_t rows, int W, int lanes_log2, const T* __restrict__ a, size_t lda,
                                                                      const T* __restrict__ h1, size_t ldh1, const T* __restrict__ h2,
                                                                      size_t ldh2, T* __restrict__ m, size_t ldm) {
  const int x = threadIdx.x & ((1 << lanes_log2) - 1), y = threadIdx.x >> lanes_log2, rpb = GATE_THREADS >> lanes_log2;
  const size_t c = ((size_t)blockIdx.x << lanes_log2) + x;
  if (c * VEC >= (size_t)W) return;                                  // W % VEC == 0: a vector is inside the row or outside it
  const size_t col = c * VEC, step = (size_t)gridDim.y * rpb;
  for (size_t r = (size_t)blockIdx.y * rpb + y; r < rows; r += step) {
    float av[VEC], p[VEC], q[VEC], o[VEC];
    gate_load<T, VEC>(a + r * lda + col, av);
    gate_load<T, VEC>(h1 + r * ldh1 + col, p);
    gate_load<T, VEC>(h2 + r * ldh2 + col, q);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float z = sigmoid_f(av[j]);
      o[j] = z * p[j] + (1.0f - z) * q[j];
    }
    gate_store<T, VEC>(m + r * ldm + col, o);
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(GATE_THREADS) void gate_merge_bwd_kernel(size_t rows, int W, int lanes_log2, const T* __restrict__ a, size_t lda,
                                                                      const T* __restrict__ h1, size_t ldh1, const T* __restrict__ h2,
                                                                      size_t ldh2, const T* __restrict__ dm, size_t lddm, T* __restrict__ da,
                                                                      size_t ldda, T* __restrict__ dh1, size_t lddh1, T* __restrict__ dh2,
                                                                      size_t lddh2) {
  const int x = threadIdx.x & ((1 << lanes_log2) - 1), y = threadIdx.x >> lanes_log2, rpb = GATE_THREADS >> lanes_log2;
  const size_t c = ((size_t)blockIdx.x << lanes_log2) + x;
  if (c * VEC >= (size_t)W) return;
  const size_t col = c * VEC, step = (size_t)gridDim.y * rpb;
  for (size_t r = (size_t)blockIdx.y * rpb + y; r < rows; r += step) {
    float av[VEC], p[VEC], q[VEC], g[VEC], oa[VEC], o1[VEC], o2[VEC];
    gate_load<T, VEC>(a + r * lda + col, av);
    gate_load<T, VEC>(h1 + r * ldh1 + col, p);
    gate_load<T, VEC>(h2 + r * ldh2 + col, q);
    gate_load<T, VEC>(dm + r * lddm + col, g);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float z = sigmoid_f(av[j]);
      const float gz = g[j] * z;
      o1[j] = gz;
      o2[j] = g[j] - gz;
      oa[j] = ((g[j] * (p[j] - q[j])) * z) * (1.0f - z);
    }
    gate_store<T, VEC>(da + r * ldda + col, oa);
    gate_store<T, VEC>(dh1 + r * lddh1 + col, o1);
    gate_store<T, VEC>(dh2 + r * lddh2 + col, o2);
  }
}

namespace {
struct GateOperand {
  const void* p;
  int ld;
};

// the checks both entry points share -> MTS_OK, or the error; *vec16 = every operand allows 16-byte accesses
int gate_check(const char* who, int dtype, size_t rows, int W, const GateOperand* ops, int n, bool* vec16) {
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "%s: bad dtype %d", who, dtype);
  MTS_CHECK_ARG(W >= 1 && W % 4 == 0, "%s: W=%d must be a positive multiple of 4", who, W);
  const size_t es = dtype == MTS_F32 ? 4 : 2;
  bool v16 = (W * es) % 16 == 0;
  for (int i = 0; i < n; ++i) {
    MTS_CHECK_ARG(ops[i].ld >= W && ops[i].ld % 4 == 0, "%s: leading dimension %d (operand %d) must be a multiple of 4 and >= W=%d", who, ops[i].ld, i, W);
    MTS_CHECK_ARG(((uintptr_t)ops[i].p) % (4 * es) == 0, "%s: operand %d is not aligned to a 4-element vector (%d bytes)", who, i, (int)(4 * es));
    MTS_CHECK_ARG(rows == 0 || ops[i].p != nullptr, "%s: operand %d is NULL", who, i);
    v16 = v16 && ((uintptr_t)ops[i].p) % 16 == 0 && ((size_t)ops[i].ld * es) % 16 == 0;
  }
  *vec16 = v16;
  return MTS_OK;
}

// block / grid shape for `vecs` vectors per row
void gate_shape(size_t rows, int vecs, int* lanes_log2, dim3* grid) {
  int lg = 0;
  while ((1 << lg) < vecs && lg < 6) ++lg;
  const int rpb = GATE_THREADS >> lg;
  const unsigned gx = (unsigned)ceil_div(vecs, 1 << lg);
  const size_t want = (rows + rpb - 1) / rpb;
  const unsigned gy = (unsigned)std::max<size_t>(1, std::min<size_t>(want, std::max<unsigned>(1u, GATE_MAX_BLOCKS / gx)));
  *lanes_log2 = lg;
  *grid = dim3(gx, gy);
}
}  // namespace

extern "C" int mts_gate_merge_fwd(void* stream, int dtype, size_t rows, int W, const void* a, int lda, const void* h1, int ldh1, const void* h2,
                                  int ldh2, void* m, int ldm) {
  const GateOperand ops[4] = {{a, lda}, {h1, ldh1}, {h2, ldh2}, {m, ldm}};
  bool v16 = false;
  int rc = gate_check("mts_gate_merge_fwd", dtype, rows, W, ops, 4, &v16);
  if (rc) return rc;
  if (rows == 0) return MTS_OK;
  hipStream_t st = (hipStream_t)stream;
  int lg;
  dim3 grid;
  if (dtype == MTS_F32) {
    gate_shape(rows, W / 4, &lg, &grid);
    hipLaunchKernelGGL((gate_merge_fwd_kernel<float, 4>), grid, dim3(GATE_THREADS), 0, st, rows, W, lg, (const float*)a, (size_t)lda, (const float*)h1,
                       (size_t)ldh1, (const float*)h2, (size_t)ldh2, (float*)m, (size_t)ldm);
  } else if (v16) {
    gate_shape(rows, W / 8, &lg, &grid);
    hipLaunchKernelGGL((gate_merge_fwd_kernel<bf16_t, 8>), grid, dim3(GATE_THREADS), 0, st, rows, W, lg, (const bf16_t*)a, (size_t)lda,
                       (const bf16_t*)h1, (size_t)ldh1, (const bf16_t*)h2, (size_t)ldh2, (bf16_t*)m, (size_t)ldm);
  } else {
    gate_shape(rows, W / 4, &lg, &grid);
    hipLaunchKernelGGL((gate_merge_fwd_kernel<bf16_t, 4>), grid, dim3(GATE_THREADS), 0, st, rows, W, lg, (const bf16_t*)a, (size_t)lda,
                       (const bf16_t*)h1, (size_t)ldh1, (const bf16_t*)h2, (size_t)ldh2, (bf16_t*)m, (size_t)ldm);
  }
  MTS_LAUNCH_CHECK("mts_gate_merge_fwd");
  return MTS_OK;
}

extern "C" int mts_gate_merge_bwd(void* stream, int dtype, size_t rows, int W, const void* a, int lda, const void* h1, int ldh1, const void* h2,
                                  int ldh2, const void* dm, int lddm, void* da, int ldda, void* dh1, int lddh1, void* dh2, int lddh2) {
  const GateOperand ops[7] = {{a, lda}, {h1, ldh1}, {h2, ldh2}, {dm, lddm}, {da, ldda}, {dh1, lddh1}, {dh2, lddh2}};
  bool v16 = false;
  int rc = gate_check("mts_gate_merge_bwd", dtype, rows, W, ops, 7, &v16);
  if (rc) return rc;
  if (rows == 0) return MTS_OK;
  hipStream_t st = (hipStream_t)stream;
  int lg;
  dim3 grid;
  if (dtype == MTS_F32) {
    gate_shape(rows, W / 4, &lg, &grid);
    hipLaunchKernelGGL((gate_merge_bwd_kernel<float, 4>), grid, dim3(GATE_THREADS), 0, st, rows, W, lg, (const float*)a, (size_t)lda, (const float*)h1,
                       (size_t)ldh1, (const float*)h2, (size_t)ldh2, (const float*)dm, (size_t)lddm, (float*)da, (size_t)ldda, (float*)dh1,
                       (size_t)lddh1, (float*)dh2, (size_t)lddh2);
  } else if (v16) {
    gate_shape(rows, W / 8, &lg, &grid);
    hipLaunchKernelGGL((gate_merge_bwd_kernel<bf16_t, 8>), grid, dim3(GATE_THREADS), 0, st, rows, W, lg, (const bf16_t*)a, (size_t)lda,
                       (const bf16_t*)h1, (size_t)ldh1, (const bf16_t*)h2, (size_t)ldh2, (const bf16_t*)dm, (size_t)lddm, (bf16_t*)da, (size_t)ldda,
                       (bf16_t*)dh1, (size_t)lddh1, (bf16_t*)dh2, (size_t)lddh2);
  } else {
    gate_shape(rows, W / 4, &lg, &grid);
    hipLaunchKernelGGL((gate_merge_bwd_kernel<bf16_t, 4>), grid, dim3(GATE_THREADS), 0, st, rows, W, lg, (const bf16_t*)a, (size_t)lda,
                       (const bf16_t*)h1, (size_t)ldh1, (const bf16_t*)h2, (size_t)ldh2, (const bf16_t*)dm, (size_t)lddm, (bf16_t*)da, (size_t)ldda,
                       (bf16_t*)dh1, (size_t)lddh1, (bf16_t*)dh2, (size_t)lddh2);
  }
  MTS_LAUNCH_CHECK("mts_gate_merge_bwd");
  return MTS_OK;
}
