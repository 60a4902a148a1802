// T5's RMSNorm (T5LayerNorm: no mean subtraction, no bias) for gfx950, forward and backward.
//
//   y = w * (x * rstd),  rstd = rsqrt(mean(x^2) + eps)     (the variance in fp32, as HF computes it)
//   dx = rstd * (dn - n * mean(dn . n)) (+ dres),  n = x * rstd, dn = dy * w
//   dw = sum_rows dy * n   -- per-workgroup partial rows in the workspace, then one fixed-order reduce: no atomics, bitwise reproducible.
//
// One wave per row; lane l holds columns 4 l + 256 k, k < NV (D <= 256 NV).  256-thread workgroups = 4 rows at a time.
#include <algorithm>
#include "common.h"

#define RMS_WAVES 4
#define RMS_BWD_BLOCKS 256   // workgroups of the backward (grid-stride over rows): the partial-dw slab has this many rows at most

template <typename T, int NV>
__global__ __launch_bounds__(256) void rms_fwd_kernel(int rows, int D, const T* __restrict__ x, const float* __restrict__ w, float eps,
                                                      T* __restrict__ y, float* __restrict__ rstd_out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * RMS_WAVES + wv;
  if (r >= rows) return;
  const T* xr = x + (size_t)r * D;
  float v[NV][4];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * lane + 256 * k;
    if (c < D) {
      load4<T>(xr + c, v[k]);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss = fmaf(v[k][e], v[k][e], ss);
    }
  }
  ss = wave_sum(ss);
  const float rs = 1.0f / sqrtf(ss / (float)D + eps);
  T* yr = y + (size_t)r * D;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * lane + 256 * k;
    if (c < D) {
      const float4 wv4 = *reinterpret_cast<const float4*>(w + c);
      float o[4] = {wv4.x * (v[k][0] * rs), wv4.y * (v[k][1] * rs), wv4.z * (v[k][2] * rs), wv4.w * (v[k][3] * rs)};
      store4<T>(yr + c, o);
    }
  }
  if (lane == 0 && rstd_out) rstd_out[r] = rs;
}

// grid-stride over rows: workgroup b takes rows 4 b + wave, 4 (b + nblocks) + wave, ... (fixed for a given (rows, nblocks))
template <typename T, int NV>
__global__ __launch_bounds__(256) void rms_bwd_kernel(int rows, int D, const T* __restrict__ x, const T* __restrict__ dy,
                                                      const T* dres, const float* __restrict__ w, const float* __restrict__ rstd,
                                                      T* dx, float* __restrict__ partial) {
  __shared__ float red[RMS_WAVES][256 * NV];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float dw[NV][4];
#pragma unroll
  for (int k = 0; k < NV; ++k) dw[k][0] = dw[k][1] = dw[k][2] = dw[k][3] = 0.f;
  for (int r = blockIdx.x * RMS_WAVES + wv; r < rows; r += gridDim.x * RMS_WAVES) {
    const float rs = rstd[r];
    float n[NV][4], dn[NV][4];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = 4 * lane + 256 * k;
      if (c < D) {
        float xv[4], g[4];
        load4<T>(x + (size_t)r * D + c, xv);
        load4<T>(dy + (size_t)r * D + c, g);
        const float4 wv4 = *reinterpret_cast<const float4*>(w + c);
        const float ww[4] = {wv4.x, wv4.y, wv4.z, wv4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          n[k][e] = xv[e] * rs;
          dn[k][e] = g[e] * ww[e];
          s = fmaf(dn[k][e], n[k][e], s);
          dw[k][e] = fmaf(g[e], n[k][e], dw[k][e]);
        }
      }
    }
    s = wave_sum(s) / (float)D;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = 4 * lane + 256 * k;
      if (c < D) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rs * (dn[k][e] - n[k][e] * s);
        if (dres) {                                    // may alias dx: each element is read, then written, by this lane
          float q[4];
          load4<T>(dres + (size_t)r * D + c, q);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] += q[e];
        }
        store4<T>(dx + (size_t)r * D + c, o);
      }
    }
  }
  // the four waves' dw, combined in a fixed order
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = 4 * lane + 256 * k;
    if (c < D)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wv][c + e] = dw[k][e];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 256)
    partial[(size_t)blockIdx.x * D + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// grid ceil(D / 16); thread = (part p = tid / 16, column = 16 blockIdx.x + tid % 16): part p sums partial rows p, p + 16, ... in order,
// then parts 0 .. 15 in order
__global__ __launch_bounds__(256) void rms_dw_reduce_kernel(int nblocks, int D, const float* __restrict__ partial, float* __restrict__ dw) {
  __shared__ float part[16][16];
  const int q = threadIdx.x & 15, p = threadIdx.x >> 4, c = blockIdx.x * 16 + q;
  float s = 0.f;
  if (c < D)
    for (int b = p; b < nblocks; b += 16) s += partial[(size_t)b * D + c];
  part[p][q] = s;
  __syncthreads();
  if (p == 0 && c < D) {
    float t = part[0][q];
    for (int k = 1; k < 16; ++k) t += part[k][q];
    dw[c] = t;
  }
}

static int rms_nv(int D) {
  const int nv = (D + 255) / 256;
  return nv <= 1 ? 1 : nv <= 2 ? 2 : nv <= 4 ? 4 : nv <= 8 ? 8 : 0;
}

static int rms_check(int dtype, int rows, int D, const char* who) {
  MTS_CHECK_ARG(rows > 0 && D > 0, "%s: bad shape rows=%d D=%d", who, rows, D);
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "%s: bad dtype %d", who, dtype);
  MTS_UNSUPPORTED(D % 4 == 0 && D <= 2048, "%s: D=%d must be a multiple of 4 and <= 2048", who, D);
  return MTS_OK;
}

// 4-element vector access: activations aligned to 4 elements (16 B fp32, 8 B bf16), w to 16 B; NULL passes
static bool rms_aligned(int dtype, const void* p) { return ((uintptr_t)p & (dtype == MTS_F32 ? 15 : 7)) == 0; }

extern "C" int mts_rmsnorm_fwd(void* stream, int dtype, int rows, int D, const void* x, const float* w, float eps, void* y, float* rstd) {
  int rc = rms_check(dtype, rows, D, "mts_rmsnorm_fwd");
  if (rc) return rc;
  MTS_CHECK_ARG(x && w && y, "mts_rmsnorm_fwd: null pointer");
  MTS_UNSUPPORTED(rms_aligned(dtype, x) && rms_aligned(dtype, y) && ((uintptr_t)w & 15) == 0,
                  "mts_rmsnorm_fwd: x, y must be aligned to 4 elements and w to 16 bytes");
  const dim3 grid(ceil_div(rows, RMS_WAVES));
  hipStream_t st = (hipStream_t)stream;
#define RMS_FWD(T, NV) hipLaunchKernelGGL((rms_fwd_kernel<T, NV>), grid, dim3(256), 0, st, rows, D, (const T*)x, w, eps, (T*)y, rstd)
#define RMS_FWD_T(T)                                                                                         \
  switch (rms_nv(D)) { case 1: RMS_FWD(T, 1); break; case 2: RMS_FWD(T, 2); break; case 4: RMS_FWD(T, 4); break; default: RMS_FWD(T, 8); }
  if (dtype == MTS_F32) { RMS_FWD_T(float) } else { RMS_FWD_T(bf16_t) }
#undef RMS_FWD_T
#undef RMS_FWD
  MTS_LAUNCH_CHECK("mts_rmsnorm_fwd");
  return MTS_OK;
}

extern "C" size_t mts_rmsnorm_bwd_workspace(int rows, int D) {
  const int nb = std::min(RMS_BWD_BLOCKS, std::max(1, ceil_div(rows, RMS_WAVES)));
  return (size_t)nb * (size_t)std::max(D, 1) * sizeof(float);
}

extern "C" int mts_rmsnorm_bwd(void* stream, int dtype, int rows, int D, const void* x, const void* dy, const void* dres, const float* w,
                               const float* rstd, void* dx, float* dw, void* workspace) {
  int rc = rms_check(dtype, rows, D, "mts_rmsnorm_bwd");
  if (rc) return rc;
  MTS_CHECK_ARG(x && dy && w && rstd && dx && dw && workspace, "mts_rmsnorm_bwd: null pointer (workspace is required)");
  MTS_CHECK_ARG(dx != x && dx != dy, "mts_rmsnorm_bwd: dx may alias dres only");
  MTS_UNSUPPORTED(rms_aligned(dtype, x) && rms_aligned(dtype, dy) && rms_aligned(dtype, dres) && rms_aligned(dtype, dx) && ((uintptr_t)w & 15) == 0,
                  "mts_rmsnorm_bwd: x, dy, dres, dx must be aligned to 4 elements and w to 16 bytes");
  const int nb = std::min(RMS_BWD_BLOCKS, std::max(1, ceil_div(rows, RMS_WAVES)));
  float* partial = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
#define RMS_BWD(T, NV)                                                                                                   \
  hipLaunchKernelGGL((rms_bwd_kernel<T, NV>), dim3(nb), dim3(256), 0, st, rows, D, (const T*)x, (const T*)dy, (const T*)dres, w, rstd, \
                     (T*)dx, partial)
#define RMS_BWD_T(T)                                                                                         \
  switch (rms_nv(D)) { case 1: RMS_BWD(T, 1); break; case 2: RMS_BWD(T, 2); break; case 4: RMS_BWD(T, 4); break; default: RMS_BWD(T, 8); }
  if (dtype == MTS_F32) { RMS_BWD_T(float) } else { RMS_BWD_T(bf16_t) }
#undef RMS_BWD_T
#undef RMS_BWD
  hipLaunchKernelGGL(rms_dw_reduce_kernel, dim3(ceil_div(D, 16)), dim3(256), 0, st, nb, D, partial, dw);
  MTS_LAUNCH_CHECK("mts_rmsnorm_bwd");
  return MTS_OK;
}
