// Cosine auxiliary segment loss of BiLSTM / BiLSTMLateFusion (models/CRF.py:23-92, :322-337, :427-442) for gfx950, forward and backward.
//
//   segment s = rows [begin, end) of document doc of x [B*L, W];  even_s = sum of its rows begin, begin + 2, ..,  odd_s = the others
//   positive pair (target +1) of a segment with more than one row: (even_s, odd_s);   negative pair (target -1) of a listed segment:
//   (even_s + odd_s, even_n + odd_n) with n the next segment of the document (its tail after the last listed end; maybe empty -> zero vector)
//   cos = a.b / sqrt((|a|^2 + 1e-12)(|b|^2 + 1e-12));   term = 1 - cos (target +1) | max(cos, 0) (target -1);   loss = mean of the terms
//
// Streaming with short ragged reductions, no reuse: one wave per (segment, 64-lane column slab) reads its rows once, 16 bytes per lane, four
// rows (two of each parity) in flight, fp32 sums in registers.  Per-pair statistics by one wave per pair from the fp32 sums; the mean by one
// wave in a fixed order.  Backward in gather form: one fp32 gradient vector per (segment, parity) from the statistics, then every row of
// dx takes scale x its segment's vector through the row map.  No atomics anywhere: bitwise reproducible.
#include "common.h"

#define SEGCOS_WAVES 4    // work items (forward: segment x slab, backward: rows) per 256-thread workgroup
#define SEG_COLS 8        // int32 per row of the segment table
#define PAIR_COLS 4       // int32 per row of the pair table
#define SEGCOS_EPS 1e-12f // torch's CosineEmbeddingLoss

enum { SEG_DOC = 0, SEG_BEGIN, SEG_END, SEG_TAIL, SEG_POS, SEG_NEG_FIRST, SEG_NEG_SECOND };
enum { PAIR_A = 0, PAIR_B, PAIR_TARGET };
enum { ST_COS = 0, ST_RS, ST_INV_A, ST_INV_B };

template <typename T> struct SegVec;
template <> struct SegVec<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float (&o)[4]) { load4<float>(p, o); }
  static __device__ __forceinline__ void store(float* p, const float (&o)[4]) { store4<float>(p, o); }
};
template <> struct SegVec<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float (&o)[8]) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      o[2 * w] = bf16_lo((&v.x)[w]);
      o[2 * w + 1] = bf16_hi((&v.x)[w]);
    }
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&o)[8]) {
    uint4 v;
#pragma unroll
    for (int w = 0; w < 4; ++w) (&v.x)[w] = pack_bf16x2(o[2 * w], o[2 * w + 1]);
    *reinterpret_cast<uint4*>(p) = v;
  }
};

// V consecutive fp32 of the workspace (16-byte aligned), V = 4 | 8
template <int V> __device__ __forceinline__ void ws_load(const float* p, float (&o)[V]) {
#pragma unroll
  for (int q = 0; q < V; q += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + q);
    o[q] = v.x; o[q + 1] = v.y; o[q + 2] = v.z; o[q + 3] = v.w;
  }
}
template <int V> __device__ __forceinline__ void ws_store(float* p, const float (&o)[V]) {
#pragma unroll
  for (int q = 0; q < V; q += 4) *reinterpret_cast<float4*>(p + q) = make_float4(o[q], o[q + 1], o[q + 2], o[q + 3]);
}

// sums[s][0 | 1][W] = even-row | odd-row sums of segment s.  A table row outside the batch is an empty segment: no address is formed from it.
template <typename T>
__global__ __launch_bounds__(256) void segcos_sums_kernel(int B, int L, int W, const T* __restrict__ x, int ldx, int S, int nslab,
                                                          const int32_t* __restrict__ seg, float* __restrict__ sums) {
  constexpr int V = SegVec<T>::N;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int item = blockIdx.x * SEGCOS_WAVES + wv;
  if (item >= S * nslab) return;
  const int s = item / nslab, c = (item % nslab) * 64 * V + lane * V;
  if (c >= W) return;
  const int32_t* e = seg + (size_t)s * SEG_COLS;
  int doc = e[SEG_DOC], begin = e[SEG_BEGIN], end = e[SEG_END];
  if (doc < 0 || doc >= B || begin < 0 || end > L) { doc = 0; begin = end = 0; }
  float ev[V], od[V];
#pragma unroll
  for (int q = 0; q < V; ++q) ev[q] = od[q] = 0.f;
  const T* base = x + (size_t)doc * L * ldx + c;
  for (int r = begin; r < end; r += 4) {            // four rows in flight (two of each parity); added in row order
    float a[4][V];
    const int left = end - r;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < left) SegVec<T>::load(base + (size_t)(r + u) * ldx, a[u]);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      ev[q] += a[0][q];
      if (left > 1) od[q] += a[1][q];
      if (left > 2) ev[q] += a[2][q];
      if (left > 3) od[q] += a[3][q];
    }
  }
  ws_store<V>(sums + ((size_t)s * 2) * W + c, ev);
  ws_store<V>(sums + ((size_t)s * 2 + 1) * W + c, od);
}

// one wave per pair: stats[p] = {cos, 1 / sqrt((|a|^2 + eps)(|b|^2 + eps)), 1 / (|a|^2 + eps), 1 / (|b|^2 + eps)}
__global__ __launch_bounds__(256) void segcos_pairs_kernel(int W, int S, int P, const int32_t* __restrict__ pair, const float* __restrict__ sums,
                                                           float* __restrict__ stats, float* __restrict__ pair_cos) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p = blockIdx.x * SEGCOS_WAVES + wv;
  if (p >= P) return;
  const int ia = pair[(size_t)p * PAIR_COLS + PAIR_A], ib = pair[(size_t)p * PAIR_COLS + PAIR_B];
  const bool pos = pair[(size_t)p * PAIR_COLS + PAIR_TARGET] > 0;
  const bool ok = ia >= 0 && ia < S && ib >= 0 && ib < S;
  float dot = 0.f, na = 0.f, nb = 0.f;
  if (ok) {
    const float* ae = sums + ((size_t)ia * 2) * W;
    const float* ao = ae + W;
    const float* be = sums + ((size_t)ib * 2) * W;
    const float* bo = be + W;
    for (int c = lane * 4; c < W; c += 256) {
      float a[4], b[4], t[4];
      if (pos) {                                   // (even, odd) of one segment
        ws_load<4>(ae + c, a);
        ws_load<4>(ao + c, b);
      } else {                                     // (whole segment, whole next segment)
        ws_load<4>(ae + c, a);
        ws_load<4>(ao + c, t);
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] += t[q];
        ws_load<4>(be + c, b);
        ws_load<4>(bo + c, t);
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] += t[q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        dot += a[q] * b[q];
        na += a[q] * a[q];
        nb += b[q] * b[q];
      }
    }
  }
  dot = wave_sum(dot);
  na = wave_sum(na);
  nb = wave_sum(nb);
  if (lane == 0) {
    const float rs = 1.0f / sqrtf((na + SEGCOS_EPS) * (nb + SEGCOS_EPS));
    const float cs = dot * rs;
    float* st = stats + (size_t)p * 4;
    st[ST_COS] = cs;
    st[ST_RS] = rs;
    st[ST_INV_A] = 1.0f / (na + SEGCOS_EPS);
    st[ST_INV_B] = 1.0f / (nb + SEGCOS_EPS);
    if (pair_cos) pair_cos[p] = cs;
  }
}

// one wave: loss_out = {mean of the pair terms, P}, lane-strided partial sums added in a fixed order
__global__ __launch_bounds__(64) void segcos_mean_kernel(int P, const int32_t* __restrict__ pair, const float* __restrict__ stats,
                                                         float* __restrict__ loss_out) {
  float acc = 0.f;
  for (int p = threadIdx.x; p < P; p += 64) {
    const float cs = stats[(size_t)p * 4 + ST_COS];
    acc += pair[(size_t)p * PAIR_COLS + PAIR_TARGET] > 0 ? 1.0f - cs : fmaxf(cs, 0.f);
  }
  acc = wave_sum(acc);
  if (threadIdx.x == 0) {
    loss_out[0] = acc / (float)P;
    loss_out[1] = (float)P;
  }
}

// gvec[s][parity][W] = d (sum of the pair terms) / d (a row of that parity of segment s): the positive pair's term for that parity, the
// negative pair with s as first member, the previous segment's negative pair with s as second member
__global__ __launch_bounds__(256) void segcos_seggrad_kernel(int W, int S, int P, int nslab, const int32_t* __restrict__ seg,
                                                             const int32_t* __restrict__ pair, const float* __restrict__ sums,
                                                             const float* __restrict__ stats, float* __restrict__ gvec) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int item = blockIdx.x * SEGCOS_WAVES + wv;
  if (item >= S * nslab) return;
  const int s = item / nslab, c = (item % nslab) * 256 + lane * 4;
  if (c >= W) return;
  const int32_t* e = seg + (size_t)s * SEG_COLS;
  float E[4], O[4], T[4], gE[4], gO[4];
  ws_load<4>(sums + ((size_t)s * 2) * W + c, E);
  ws_load<4>(sums + ((size_t)s * 2 + 1) * W + c, O);
#pragma unroll
  for (int q = 0; q < 4; ++q) { T[q] = E[q] + O[q]; gE[q] = gO[q] = 0.f; }
  const int pp = e[SEG_POS];
  if (pp >= 0 && pp < P) {                         // term 1 - cos(E, O)
    const float* st = stats + (size_t)pp * 4;
    const float cs = st[ST_COS], rs = st[ST_RS], ka = cs * st[ST_INV_A], kb = cs * st[ST_INV_B];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      gE[q] -= O[q] * rs - ka * E[q];
      gO[q] -= E[q] * rs - kb * O[q];
    }
  }
#pragma unroll
  for (int side = 0; side < 2; ++side) {           // term max(cos, 0): side 0 = s is the first member, side 1 = the second
    const int pn = e[side == 0 ? SEG_NEG_FIRST : SEG_NEG_SECOND];
    if (pn < 0 || pn >= P) continue;
    const float* st = stats + (size_t)pn * 4;
    const float cs = st[ST_COS];
    const int other = pair[(size_t)pn * PAIR_COLS + (side == 0 ? PAIR_B : PAIR_A)];
    if (!(cs >= 0.f) || other < 0 || other >= S) continue;     // the clamp passes the gradient where cos >= 0
    const float rs = st[ST_RS], k = cs * st[side == 0 ? ST_INV_A : ST_INV_B];
    float oe[4], oo[4];
    ws_load<4>(sums + ((size_t)other * 2) * W + c, oe);
    ws_load<4>(sums + ((size_t)other * 2 + 1) * W + c, oo);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float v = (oe[q] + oo[q]) * rs - k * T[q];
      gE[q] += v;
      gO[q] += v;
    }
  }
  ws_store<4>(gvec + ((size_t)s * 2) * W + c, gE);
  ws_store<4>(gvec + ((size_t)s * 2 + 1) * W + c, gO);
}

// one wave per row: dx[r] (+)= scale * gvec[row_map[r]] (row_map[r] = 2 * segment + parity, or -1: the row is in no segment)
template <typename T>
__global__ __launch_bounds__(256) void segcos_rows_kernel(int N, int W, int S, const int32_t* __restrict__ row_map, const float* __restrict__ gvec,
                                                          float scale, int accumulate, T* __restrict__ dx, int lddx) {
  constexpr int V = SegVec<T>::N;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * SEGCOS_WAVES + wv;
  if (r >= N) return;
  const int m = row_map[r];
  const bool in = m >= 0 && m < 2 * S;
  if (!in && accumulate) return;
  T* d = dx + (size_t)r * lddx;
  const float* g = gvec + (size_t)(in ? m : 0) * W;
  for (int c = lane * V; c < W; c += 64 * V) {
    float o[V];
    if (in) {
      float gv[V];
      ws_load<V>(g + c, gv);
      if (accumulate) {
        SegVec<T>::load(d + c, o);
#pragma unroll
        for (int q = 0; q < V; ++q) o[q] = o[q] + scale * gv[q];
      } else {
#pragma unroll
        for (int q = 0; q < V; ++q) o[q] = scale * gv[q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < V; ++q) o[q] = 0.f;
    }
    SegVec<T>::store(d + c, o);
  }
}

static bool segcos_aligned(const void* p, int ld, int esize) { return ((uintptr_t)p & 15) == 0 && ((size_t)ld * esize) % 16 == 0; }

static int segcos_check(const char* who, int dtype, int B, int L, int W, int n_seg, int n_pair) {
  MTS_CHECK_ARG(B >= 0 && L >= 0 && W > 0 && n_seg >= 0 && n_pair >= 0, "%s: bad shape B=%d L=%d W=%d segments=%d pairs=%d", who, B, L, W, n_seg, n_pair);
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "%s: bad dtype %d", who, dtype);
  MTS_CHECK_ARG((long long)B * L <= 0x7fffffffLL - SEGCOS_WAVES, "%s: B*L too large", who);
  MTS_CHECK_ARG((long long)n_seg * ceil_div(W, 256) <= 0x7fffffffLL - SEGCOS_WAVES && n_pair <= 0x7fffffff - SEGCOS_WAVES,
                "%s: too many segments", who);
  MTS_UNSUPPORTED(W % (dtype == MTS_F32 ? 4 : 8) == 0, "%s: W=%d must be a multiple of %d (16-byte vectors)", who, W, dtype == MTS_F32 ? 4 : 8);
  return MTS_OK;
}

// workspace layout: sums [n_seg][2][W] | gvec [n_seg][2][W] | stats [n_pair][4], all fp32
extern "C" size_t mts_segment_cosine_workspace(int n_seg, int n_pair, int W) {
  if (n_seg < 0 || n_pair < 0 || W <= 0) return 0;
  return ((size_t)n_seg * 4 * align_up((size_t)W, 4) + (size_t)n_pair * 4) * sizeof(float);
}

extern "C" int mts_segment_cosine_fwd(void* stream, int dtype, int B, int L, int W, const void* x, int ldx, int n_seg,
                                      const int32_t* seg_table, int n_pair, const int32_t* pair_table, float* loss_out, float* pair_cos,
                                      void* workspace) {
  int rc = segcos_check("mts_segment_cosine_fwd", dtype, B, L, W, n_seg, n_pair);
  if (rc) return rc;
  MTS_CHECK_ARG(loss_out, "mts_segment_cosine_fwd: loss_out is NULL");
  hipStream_t st = (hipStream_t)stream;
  if (n_pair == 0) {                               // no pair: the cosine term is 0 (models/CRF.py:90-91), nothing to launch
    if (hipMemsetAsync(loss_out, 0, 2 * sizeof(float), st) != hipSuccess) {
      mts_set_error("mts_segment_cosine_fwd: memset failed");
      return MTS_ERR_LAUNCH;
    }
    return MTS_OK;
  }
  MTS_CHECK_ARG(x && seg_table && pair_table && workspace && n_seg > 0 && ldx >= W, "mts_segment_cosine_fwd: null pointer or leading dimension < W");
  const int es = dtype == MTS_F32 ? 4 : 2;
  MTS_UNSUPPORTED(segcos_aligned(x, ldx, es), "mts_segment_cosine_fwd: x and its leading dimension must be 16-byte aligned");
  MTS_UNSUPPORTED(((uintptr_t)workspace & 15) == 0, "mts_segment_cosine_fwd: the workspace must be 16-byte aligned");
  float* sums = (float*)workspace;
  float* stats = sums + (size_t)n_seg * 4 * W;
  const int nslab = ceil_div(W, 64 * (dtype == MTS_F32 ? 4 : 8));
  const dim3 grid(ceil_div(n_seg * nslab, SEGCOS_WAVES));
  if (dtype == MTS_F32)
    hipLaunchKernelGGL(segcos_sums_kernel<float>, grid, dim3(256), 0, st, B, L, W, (const float*)x, ldx, n_seg, nslab, seg_table, sums);
  else
    hipLaunchKernelGGL(segcos_sums_kernel<bf16_t>, grid, dim3(256), 0, st, B, L, W, (const bf16_t*)x, ldx, n_seg, nslab, seg_table, sums);
  hipLaunchKernelGGL(segcos_pairs_kernel, dim3(ceil_div(n_pair, SEGCOS_WAVES)), dim3(256), 0, st, W, n_seg, n_pair, pair_table, sums, stats, pair_cos);
  hipLaunchKernelGGL(segcos_mean_kernel, dim3(1), dim3(64), 0, st, n_pair, pair_table, stats, loss_out);
  MTS_LAUNCH_CHECK("mts_segment_cosine_fwd");
  return MTS_OK;
}

extern "C" int mts_segment_cosine_bwd(void* stream, int dtype, int B, int L, int W, int n_seg, const int32_t* seg_table, int n_pair,
                                      const int32_t* pair_table, const int32_t* row_map, float scale, int accumulate, void* dx, int lddx,
                                      void* workspace) {
  int rc = segcos_check("mts_segment_cosine_bwd", dtype, B, L, W, n_seg, n_pair);
  if (rc) return rc;
  if (B == 0 || L == 0) return MTS_OK;
  if (n_pair == 0 && accumulate) return MTS_OK;    // nothing to add
  MTS_CHECK_ARG(dx && row_map && lddx >= W, "mts_segment_cosine_bwd: null pointer or leading dimension < W");
  MTS_CHECK_ARG(n_pair == 0 || (seg_table && pair_table && workspace && n_seg > 0), "mts_segment_cosine_bwd: null table or workspace");
  const int es = dtype == MTS_F32 ? 4 : 2;
  MTS_UNSUPPORTED(segcos_aligned(dx, lddx, es), "mts_segment_cosine_bwd: dx and its leading dimension must be 16-byte aligned");
  MTS_UNSUPPORTED(((uintptr_t)workspace & 15) == 0, "mts_segment_cosine_bwd: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const float* sums = (const float*)workspace;
  float* gvec = (float*)workspace + (size_t)n_seg * 2 * W;
  const float* stats = (const float*)workspace + (size_t)n_seg * 4 * W;
  const int S = n_pair ? n_seg : 0;                // without a pair every row is "in no segment": dx is written 0
  if (S) {
    const int nslab = ceil_div(W, 256);
    hipLaunchKernelGGL(segcos_seggrad_kernel, dim3(ceil_div(S * nslab, SEGCOS_WAVES)), dim3(256), 0, st, W, S, n_pair, nslab, seg_table, pair_table,
                       sums, stats, gvec);
  }
  const int N = B * L;
  const dim3 grid(ceil_div(N, SEGCOS_WAVES));
  if (dtype == MTS_F32)
    hipLaunchKernelGGL(segcos_rows_kernel<float>, grid, dim3(256), 0, st, N, W, S, row_map, gvec, scale, accumulate, (float*)dx, lddx);
  else
    hipLaunchKernelGGL(segcos_rows_kernel<bf16_t>, grid, dim3(256), 0, st, N, W, S, row_map, gvec, scale, accumulate, (bf16_t*)dx, lddx);
  MTS_LAUNCH_CHECK("mts_segment_cosine_bwd");
  return MTS_OK;
}
