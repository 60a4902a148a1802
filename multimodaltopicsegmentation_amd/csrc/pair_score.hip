// Adjacent-pair bilinear score of SheikhBiLSTM (models/CRF.py:1009-1014, :1029-1035) for gfx950, forward and backward.
//
//   scores[b, t] = sum_h F[bL + t, h] * G[bL + t + 1, h]   (t < L - 1; fp32 accumulation),   scores[b, L - 1] = 1   (the appended step)
//   dF[b, t, :] = dscores[b, t] * G[b, t + 1, :]  (0 at t = L - 1),    dG[b, t, :] = dscores[b, t - 1] * F[b, t - 1, :]  (0 at t = 0)
//
// Pure streaming, no reuse: one wave per row, 16-byte loads per lane (8 bf16 / 4 fp32), lanes stride over H, one wave_sum per score.
// A pair never crosses a document.  The backward writes every element of dF and dG exactly once from one product: bitwise reproducible.
#include "common.h"

#define PAIR_WAVES 4      // rows per 256-thread workgroup

template <typename T> struct PairVec;
template <> struct PairVec<float> {
  static constexpr int N = 4;
  float4 v;
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
  __device__ __forceinline__ float get(int i) const { return (&v.x)[i]; }
  __device__ __forceinline__ void set_scaled(const PairVec& s, float a) { v = make_float4(a * s.v.x, a * s.v.y, a * s.v.z, a * s.v.w); }
  __device__ __forceinline__ void zero() { v = make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <> struct PairVec<bf16_t> {
  static constexpr int N = 8;
  uint4 v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ void store(bf16_t* p) const { *reinterpret_cast<uint4*>(p) = v; }
  __device__ __forceinline__ float get(int i) const {
    const uint32_t u = (&v.x)[i >> 1];
    return (i & 1) ? bf16_hi(u) : bf16_lo(u);
  }
  __device__ __forceinline__ void set_scaled(const PairVec& s, float a) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t u = (&s.v.x)[w];
      (&v.x)[w] = pack_bf16x2(a * bf16_lo(u), a * bf16_hi(u));
    }
  }
  __device__ __forceinline__ void zero() { v = make_uint4(0u, 0u, 0u, 0u); }
};

template <typename T>
__global__ __launch_bounds__(256) void pair_score_fwd_kernel(int N, int L, int H, const T* __restrict__ F, int ldf, const T* __restrict__ G,
                                                             int ldg, float* __restrict__ scores) {
  constexpr int V = PairVec<T>::N;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * PAIR_WAVES + wv;
  if (r >= N) return;
  if (r % L == L - 1) {                                // the reference's appended step; row r + 1 is another document's (or past the end)
    if (lane == 0) scores[r] = 1.0f;
    return;
  }
  const T* f = F + (size_t)r * ldf;
  const T* g = G + (size_t)(r + 1) * ldg;
  float acc = 0.f;
  for (int c = lane * V; c < H; c += 64 * V) {
    PairVec<T> a, b;
    a.load(f + c);
    b.load(g + c);
#pragma unroll
    for (int e = 0; e < V; ++e) acc = fmaf(a.get(e), b.get(e), acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) scores[r] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void pair_score_bwd_kernel(int N, int L, int H, const T* __restrict__ F, int ldf, const T* __restrict__ G,
                                                             int ldg, const float* __restrict__ dscores, T* __restrict__ dF, int lddf,
                                                             T* __restrict__ dG, int lddg) {
  constexpr int V = PairVec<T>::N;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * PAIR_WAVES + wv;
  if (r >= N) return;
  const int t = r % L;
  const bool has_next = t < L - 1, has_prev = t > 0;   // dscores[b, L - 1] is never read
  const float ds_f = has_next ? dscores[r] : 0.f;
  const float ds_g = has_prev ? dscores[r - 1] : 0.f;
  const T* g = G + (size_t)(has_next ? r + 1 : r) * ldg;   // row r + 1 < N, same document
  const T* f = F + (size_t)(has_prev ? r - 1 : r) * ldf;   // row r - 1 >= 0, same document
  T* df = dF + (size_t)r * lddf;
  T* dg = dG + (size_t)r * lddg;
  for (int c = lane * V; c < H; c += 64 * V) {
    PairVec<T> in, out;
    if (has_next) { in.load(g + c); out.set_scaled(in, ds_f); } else out.zero();
    out.store(df + c);
    if (has_prev) { in.load(f + c); out.set_scaled(in, ds_g); } else out.zero();
    out.store(dg + c);
  }
}

static bool pair_aligned(const void* p, int ld, int esize) { return ((uintptr_t)p & 15) == 0 && ((size_t)ld * esize) % 16 == 0; }

static int pair_check(const char* who, int dtype, int B, int L, int H) {
  MTS_CHECK_ARG(B >= 0 && L >= 0 && H > 0, "%s: bad shape B=%d L=%d H=%d", who, B, L, H);
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "%s: bad dtype %d", who, dtype);
  MTS_CHECK_ARG((long long)B * L <= 0x7fffffffLL - PAIR_WAVES, "%s: B*L too large", who);
  MTS_UNSUPPORTED(H % (dtype == MTS_F32 ? 4 : 8) == 0, "%s: H=%d must be a multiple of %d (16-byte vectors)", who, H, dtype == MTS_F32 ? 4 : 8);
  return MTS_OK;
}

extern "C" int mts_pair_score_fwd(void* stream, int dtype, int B, int L, int H, const void* F, int ldf, const void* G, int ldg, float* scores) {
  int rc = pair_check("mts_pair_score_fwd", dtype, B, L, H);
  if (rc) return rc;
  if (B == 0 || L == 0) return MTS_OK;
  MTS_CHECK_ARG(F && G && scores && ldf >= H && ldg >= H, "mts_pair_score_fwd: null pointer or leading dimension < H");
  const int es = dtype == MTS_F32 ? 4 : 2;
  MTS_UNSUPPORTED(pair_aligned(F, ldf, es) && pair_aligned(G, ldg, es), "mts_pair_score_fwd: F, G and their leading dimensions must be 16-byte aligned");
  const int N = B * L;
  const dim3 grid(ceil_div(N, PAIR_WAVES));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MTS_F32)
    hipLaunchKernelGGL(pair_score_fwd_kernel<float>, grid, dim3(256), 0, st, N, L, H, (const float*)F, ldf, (const float*)G, ldg, scores);
  else
    hipLaunchKernelGGL(pair_score_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, N, L, H, (const bf16_t*)F, ldf, (const bf16_t*)G, ldg, scores);
  MTS_LAUNCH_CHECK("mts_pair_score_fwd");
  return MTS_OK;
}

extern "C" int mts_pair_score_bwd(void* stream, int dtype, int B, int L, int H, const void* F, int ldf, const void* G, int ldg,
                                  const float* dscores, void* dF, int lddf, void* dG, int lddg) {
  int rc = pair_check("mts_pair_score_bwd", dtype, B, L, H);
  if (rc) return rc;
  if (B == 0 || L == 0) return MTS_OK;
  MTS_CHECK_ARG(F && G && dscores && dF && dG && ldf >= H && ldg >= H && lddf >= H && lddg >= H,
                "mts_pair_score_bwd: null pointer or leading dimension < H");
  MTS_CHECK_ARG(dF != F && dF != G && dG != F && dG != G && dF != dG, "mts_pair_score_bwd: dF and dG may not alias the inputs or each other");
  const int es = dtype == MTS_F32 ? 4 : 2;
  MTS_UNSUPPORTED(pair_aligned(F, ldf, es) && pair_aligned(G, ldg, es) && pair_aligned(dF, lddf, es) && pair_aligned(dG, lddg, es),
                  "mts_pair_score_bwd: F, G, dF, dG and their leading dimensions must be 16-byte aligned");
  const int N = B * L;
  const dim3 grid(ceil_div(N, PAIR_WAVES));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MTS_F32)
    hipLaunchKernelGGL(pair_score_bwd_kernel<float>, grid, dim3(256), 0, st, N, L, H, (const float*)F, ldf, (const float*)G, ldg, dscores,
                       (float*)dF, lddf, (float*)dG, lddg);
  else
    hipLaunchKernelGGL(pair_score_bwd_kernel<bf16_t>, grid, dim3(256), 0, st, N, L, H, (const bf16_t*)F, ldf, (const bf16_t*)G, ldg, dscores,
                       (bf16_t*)dF, lddf, (bf16_t*)dG, lddg);
  MTS_LAUNCH_CHECK("mts_pair_score_bwd");
  return MTS_OK;
}
