// Domain-switched tagger heads of SwitchBiLSTM(switch='dense') (models/CRF.py:1132-1139 regroup, :1195-1205, :1248-1258) for gfx950.
//
// Two stacked heads w[2][n_out][D], bias[2][n_out]; per document b two int32 maps built on the host from `domains`:
//   doc_head[b] in {0, 1}: which head scores document b;   doc_src[b] in [0, B): whose encoder rows it is scored FROM (the reference's
//   regroup hands document b the rows of document rank(b), its position inside its own domain group -- see DESIGN.md).
//   forward      scores[b, t, c] = x[doc_src[b], t, :] . w[doc_head[b], c, :] + bias[doc_head[b], c]
//   bwd params   dw[k, c, :] = sum_{b: doc_head[b] = k} sum_t ds[b, t, c] x[doc_src[b], t, :],  db[k, c] likewise
//   bwd data     dx[r, t, :] = sum_k sum_c ds[doc_tgt[k][r], t, c] w[k, c, :]      (gather form: document r is read by at most one
//                document per head, doc_tgt[k][r] or -1, so every dx row is written once by one thread -- no atomics)
//
// Memory-bound row kernels in the mapping of norm.hip's head kernels: one wave per row, 4 elements per lane and step (16 B fp32, 8 B
// bf16), fp32 accumulation, column sums in registers -> per-workgroup slabs -> fixed-order reduce (bitwise reproducible).
// A map entry outside its range contributes nothing: the row is written as 0 (forward, data) or skipped (params), and no address is
// ever formed from it.
#include <algorithm>
#include <type_traits>
#include "common.h"

#define SW_WAVES 4             // rows in flight per workgroup
#define SW_MAX_BLOCKS 512      // workgroups per head of the parameter pass
#define SW_FLAG_BYTES 4096     // workspace prefix: int32 flags[2][SW_MAX_BLOCKS], 1 = that workgroup wrote its slab

template <typename T>
__global__ __launch_bounds__(64 * SW_WAVES) void switch_head_fwd_kernel(const T* __restrict__ x, int ldx, int B, int L, int D, int n_out,
                                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                                      const int32_t* __restrict__ doc_src, const int32_t* __restrict__ doc_head,
                                                                      float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * SW_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the map reads below are scalar loads
  if (row >= B * L) return;
  const int b = row / L, t = row - b * L;
  const int src = doc_src[b], k = doc_head[b];
  if ((unsigned)src >= (unsigned)B || (unsigned)k > 1u) {        // wave-uniform
    if (lane < n_out) scores[(size_t)row * n_out + lane] = 0.f;
    return;
  }
  const T* xr = x + ((size_t)src * L + t) * ldx;
  const float* wk = w + (size_t)k * n_out * D;
  float hs[4] = {0.f, 0.f, 0.f, 0.f};
  for (int e = 4 * lane; e < D; e += 256) {
    float xv[4];
    load4<T>(xr + e, xv);
    for (int c = 0; c < n_out; ++c) {
      float wv[4];
      load4<float>(wk + (size_t)c * D + e, wv);
#pragma unroll
      for (int j = 0; j < 4; ++j) hs[c] += xv[j] * wv[j];
    }
  }
  for (int c = 0; c < n_out; ++c) {
    const float s = wave_sum(hs[c]);
    if (lane == 0) scores[(size_t)row * n_out + c] = s + bias[k * n_out + c];
  }
}

// dx[r, t, :] = sum_k sum_c ds[doc_tgt[k][r], t, c] w[k, c, :]; rows nobody reads are written as zeros
template <typename T>
__global__ __launch_bounds__(256) void switch_head_bwd_data_kernel(const float* __restrict__ ds, const float* __restrict__ w, int B, int L, int D,
                                                                   int n_out, const int32_t* __restrict__ doc_tgt, T* __restrict__ dx, int lddx) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = D / 4;
  const size_t total = (size_t)B * L * per_row;
  if (idx >= total) return;
  const int row = (int)(idx / per_row);
  const int e = 4 * (int)(idx % per_row);
  const int r = row / L, t = row - r * L;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int tg = doc_tgt[k * B + r];
    if ((unsigned)tg < (unsigned)B) {                              // -1 (nobody) and anything out of range: no contribution
      const float* dr = ds + ((size_t)tg * L + t) * n_out;
      for (int c = 0; c < n_out; ++c) {
        const float s = dr[c];
        float wv[4];
        load4<float>(w + ((size_t)k * n_out + c) * D + e, wv);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += s * wv[j];
      }
    }
  }
  store4<T>(dx + (size_t)row * lddx + e, o);
}

// Parameter pass.  blockIdx.z = head k: the workgroup walks the rows (grid stride) and takes those of documents with doc_head == k, so
// the registers hold ONE head's dw (4 x NV x 4, as head_bwd_params_kernel); blockIdx.y = column chunk of NV * 256 when D is wider.
// The next taken row (x and its score gradients) is fetched before the current one is accumulated.  A workgroup that took no row
// writes no slab, only flag 0: a head that no document uses costs no slab traffic and comes out of the reduce as exact zeros.
// slab: [head][block][5][D], slots 0..3 dw rows, slot 4: first 4 entries = db partial.
template <typename T, int NV, bool FULL>
__global__ __launch_bounds__(64 * SW_WAVES) void switch_head_bwd_params_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ ds, int n_out,
                                                                             int B, int L, int D, const int32_t* __restrict__ doc_src,
                                                                             const int32_t* __restrict__ doc_head, int32_t* __restrict__ flags,
                                                                             float* __restrict__ partial) {
  __shared__ float red[SW_WAVES][4][64 * 4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform row index: next_taken's map reads are scalar loads
  const int head = (int)blockIdx.z;
  const int col0 = (int)blockIdx.y * (NV * 256);
  const int rows = B * L;
  float dw[4][NV][4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dw[c][i][j] = 0.f;
  float dbs[4] = {0.f, 0.f, 0.f, 0.f};
  Pack<T, 4> px[NV];
  float dl_n[4] = {0.f, 0.f, 0.f, 0.f};
  const int stride = gridDim.x * SW_WAVES;
  int src_n = 0;
  // first row >= r (in steps of stride) of a document of this head with a source in range; rows if there is none
  auto next_taken = [&](int r) {
    for (; r < rows; r += stride) {
      const int b = r / L;
      const int s = doc_src[b];
      if (doc_head[b] == head && (unsigned)s < (unsigned)B) { src_n = s; return r; }
    }
    return rows;
  };
  auto fetch = [&](int r) {
    const int t = r - (r / L) * L;
    const T* xr = x + ((size_t)src_n * L + t) * ldx;
#pragma unroll
    for (int c = 0; c < 4; ++c) dl_n[c] = ds[(size_t)r * n_out + min(c, n_out - 1)];   // unconditional; columns >= n_out are zeroed at use
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = col0 + 4 * (lane + 64 * i);
      if (FULL || e < D) px[i].load(xr + e);
    }
  };
  int row = next_taken(blockIdx.x * SW_WAVES + wave);
  int taken = row < rows;
  if (row < rows) fetch(row);
  while (row < rows) {
    float dl[4], xv[NV][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) dl[c] = (c < n_out) ? dl_n[c] : 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = col0 + 4 * (lane + 64 * i);
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[i][j] = (FULL || e < D) ? px[i].get(j) : 0.f;
    }
    row = next_taken(row + stride);
    if (row < rows) fetch(row);
#pragma unroll
    for (int c = 0; c < 4; ++c) dbs[c] += dl[c];
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) dw[c][i][j] += dl[c] * xv[i][j];
  }
  const int any = __syncthreads_or(taken);
  if (threadIdx.x == 0 && blockIdx.y == 0) flags[head * SW_MAX_BLOCKS + blockIdx.x] = any ? 1 : 0;
  if (!any) return;                                                   // block-uniform
  float* slab = partial + ((size_t)head * gridDim.x + blockIdx.x) * 5 * D;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave][c][lane * 4 + j] = dw[c][i][j];
    __syncthreads();
    for (int t = threadIdx.x; t < 4 * 256; t += 64 * SW_WAVES) {
      const int slot = t / 256, col = t % 256;
      const int e = col0 + 256 * i + col;
      if (e < D) {
        float s = 0.f;
#pragma unroll
        for (int wv = 0; wv < SW_WAVES; ++wv) s += red[wv][slot][col];
        slab[(size_t)slot * D + e] = s;
      }
    }
  }
  __syncthreads();
  if (lane == 0)
    for (int c = 0; c < 4; ++c) red[wave][c][0] = dbs[c];
  __syncthreads();
  if (threadIdx.x < 4 && blockIdx.y == 0) {
    float s = 0.f;
    for (int wv = 0; wv < SW_WAVES; ++wv) s += red[wv][threadIdx.x][0];
    slab[(size_t)4 * D + threadIdx.x] = s;
  }
}

// out[head][slot][e] = sum over the workgroups whose flag is set of partial[head][block][slot][e], in a fixed order.  Workgroup = 32
// columns (8 lanes x float4) x 32 block groups, 8 loads in flight per lane; a slab whose flag is 0 was never written: its address is
// replaced by slab 0's (inside the workspace) and the loaded value by 0 -- selected, never multiplied.
#define SW_COLS 32
__global__ __launch_bounds__(256) void switch_head_reduce_kernel(const float* __restrict__ partial, const int32_t* __restrict__ flags, int nblocks, int D,
                                                                 int n_out, float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float4 red[32][8];
  const int c4 = threadIdx.x & 7, grp = threadIdx.x >> 3;
  const int e = blockIdx.x * SW_COLS + 4 * c4;
  const int slot = blockIdx.y, head = blockIdx.z;
  if (slot < 4 && slot >= n_out) return;                              // block-uniform
  const int len = slot == 4 ? n_out : D;
  float* o = slot == 4 ? db + (size_t)head * n_out : dw + ((size_t)head * n_out + slot) * D;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e < len) {
    const size_t bs = (size_t)5 * D;
    const float* p = partial + (size_t)head * nblocks * bs + (size_t)slot * D + e;
    const int32_t* fl = flags + head * SW_MAX_BLOCKS;
    for (int b0 = grp; b0 < nblocks; b0 += 32 * 8) {
      float4 v[8];
      bool ok[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b = b0 + 32 * u;
        ok[u] = b < nblocks && fl[b < nblocks ? b : 0] != 0;
        v[u] = *reinterpret_cast<const float4*>(p + (size_t)(ok[u] ? b : 0) * bs);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        s.x += ok[u] ? v[u].x : 0.f; s.y += ok[u] ? v[u].y : 0.f; s.z += ok[u] ? v[u].z : 0.f; s.w += ok[u] ? v[u].w : 0.f;
      }
    }
  }
  red[grp][c4] = s;
  __syncthreads();
  if (grp == 0 && e < len) {
    float4 t = red[0][c4];
#pragma unroll
    for (int gidx = 1; gidx < 32; ++gidx) { const float4 v = red[gidx][c4]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
    if (slot < 4 && e + 3 < len) *reinterpret_cast<float4*>(o + e) = t;      // db (slot 4): scalar stores, no alignment asked of it
    else { const float tv[4] = {t.x, t.y, t.z, t.w}; for (int j = 0; j < 4 && e + j < len; ++j) o[e + j] = tv[j]; }
  }
}

// ------------------------------------------------------------------------------------------------ host side
static inline int sw_pick_nv(int D) {
  const int need = ceil_div(D, 256);
  if (need <= 1) return 1;
  if (need <= 2) return 2;
  if (need <= 4) return 4;
  if (need <= 16) return 8;            // 2048 < D <= 4096: two column chunks of 8 x 256
  return 0;
}

static int sw_check(const char* who, int dtype, int B, int L, int D, int n_out, const void* act, int ld) {
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "%s: bad dtype %d", who, dtype);
  MTS_CHECK_ARG(B > 0 && L > 0 && D > 0 && n_out >= 1 && n_out <= 4, "%s: bad shape B=%d L=%d D=%d n_out=%d", who, B, L, D, n_out);
  MTS_CHECK_ARG((long long)B * L <= 0x7fffffffLL / 8, "%s: B*L too large", who);
  MTS_CHECK_ARG(D % 4 == 0, "%s: D=%d must be a multiple of 4 (4-element vectors)", who, D);
  MTS_CHECK_ARG(act && ld >= D && ld % 4 == 0, "%s: null activation pointer, or its leading dimension %d is below D or no multiple of 4", who, ld);
  const uintptr_t al = dtype == MTS_F32 ? 16 : 8;
  MTS_CHECK_ARG(((uintptr_t)act & (al - 1)) == 0, "%s: the activation pointer must be %d-byte aligned (4-element vectors)", who, (int)al);
  return MTS_OK;
}

extern "C" int mts_switch_head_fwd(void* stream, int dtype, int B, int L, int D, int n_out, const void* x, int ldx, const float* w,
                                   const float* bias, const int32_t* doc_src, const int32_t* doc_head, float* scores) {
  int rc = sw_check("mts_switch_head_fwd", dtype, B, L, D, n_out, x, ldx);
  if (rc) return rc;
  MTS_CHECK_ARG(w && bias && doc_src && doc_head && scores && ((uintptr_t)w & 15) == 0, "mts_switch_head_fwd: null pointer or w not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ceil_div(B * L, SW_WAVES)), block(64 * SW_WAVES);
  if (dtype == MTS_F32)
    hipLaunchKernelGGL(switch_head_fwd_kernel<float>, grid, block, 0, st, (const float*)x, ldx, B, L, D, n_out, w, bias, doc_src, doc_head, scores);
  else
    hipLaunchKernelGGL(switch_head_fwd_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)x, ldx, B, L, D, n_out, w, bias, doc_src, doc_head, scores);
  MTS_LAUNCH_CHECK("mts_switch_head_fwd");
  return MTS_OK;
}

extern "C" size_t mts_switch_head_bwd_workspace(int D) {
  return (size_t)SW_FLAG_BYTES + (size_t)2 * SW_MAX_BLOCKS * 5 * (size_t)std::max(D, 0) * sizeof(float);
}

template <typename T>
static void sw_params_launch(hipStream_t st, int nv, int blocks, int chunks, const void* x, int ldx, const float* ds, int n_out, int B, int L, int D,
                             const int32_t* doc_src, const int32_t* doc_head, int32_t* flags, float* partial) {
  const dim3 grid(blocks, chunks, 2), block(64 * SW_WAVES);
  auto go = [&](auto nvc) {
    constexpr int NV = decltype(nvc)::value;
    if (D == NV * 256)
      hipLaunchKernelGGL((switch_head_bwd_params_kernel<T, NV, true>), grid, block, 0, st, (const T*)x, ldx, ds, n_out, B, L, D, doc_src, doc_head, flags,
                         partial);
    else
      hipLaunchKernelGGL((switch_head_bwd_params_kernel<T, NV, false>), grid, block, 0, st, (const T*)x, ldx, ds, n_out, B, L, D, doc_src, doc_head, flags,
                         partial);
  };
  switch (nv) {
    case 1: go(std::integral_constant<int, 1>{}); break;
    case 2: go(std::integral_constant<int, 2>{}); break;
    case 4: go(std::integral_constant<int, 4>{}); break;
    default: go(std::integral_constant<int, 8>{}); break;
  }
}

extern "C" int mts_switch_head_bwd_params(void* stream, int dtype, int B, int L, int D, int n_out, const void* x, int ldx, const float* dscores,
                                          const int32_t* doc_src, const int32_t* doc_head, float* dw, float* db, void* workspace) {
  int rc = sw_check("mts_switch_head_bwd_params", dtype, B, L, D, n_out, x, ldx);
  if (rc) return rc;
  MTS_CHECK_ARG(dscores && doc_src && doc_head && dw && db && workspace && ((uintptr_t)dw & 15) == 0 && ((uintptr_t)workspace & 15) == 0,
                "mts_switch_head_bwd_params: null pointer, or dw / workspace not 16-byte aligned");
  const int nv = sw_pick_nv(D);
  MTS_UNSUPPORTED(nv > 0, "mts_switch_head_bwd_params: D=%d must be <= 4096", D);
  hipStream_t st = (hipStream_t)stream;
  const int blocks = std::min(SW_MAX_BLOCKS, ceil_div(B * L, SW_WAVES));
  const int chunks = ceil_div(D, nv * 256);
  int32_t* flags = (int32_t*)workspace;
  float* partial = (float*)((char*)workspace + SW_FLAG_BYTES);
  if (dtype == MTS_F32) sw_params_launch<float>(st, nv, blocks, chunks, x, ldx, dscores, n_out, B, L, D, doc_src, doc_head, flags, partial);
  else sw_params_launch<bf16_t>(st, nv, blocks, chunks, x, ldx, dscores, n_out, B, L, D, doc_src, doc_head, flags, partial);
  hipLaunchKernelGGL(switch_head_reduce_kernel, dim3(ceil_div(D, SW_COLS), 5, 2), dim3(256), 0, st, (const float*)partial, (const int32_t*)flags, blocks, D,
                     n_out, dw, db);
  MTS_LAUNCH_CHECK("mts_switch_head_bwd_params");
  return MTS_OK;
}

extern "C" int mts_switch_head_bwd_data(void* stream, int dtype, int B, int L, int D, int n_out, const float* dscores, const float* w,
                                        const int32_t* doc_tgt, void* dx, int lddx) {
  int rc = sw_check("mts_switch_head_bwd_data", dtype, B, L, D, n_out, dx, lddx);
  if (rc) return rc;
  MTS_CHECK_ARG(dscores && w && doc_tgt && ((uintptr_t)w & 15) == 0, "mts_switch_head_bwd_data: null pointer or w not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)B * L * (D / 4);
  MTS_CHECK_ARG(total <= (size_t)0x7fffffff * 256, "mts_switch_head_bwd_data: too many elements");
  const dim3 grid((unsigned)((total + 255) / 256));
  if (dtype == MTS_F32)
    hipLaunchKernelGGL(switch_head_bwd_data_kernel<float>, grid, dim3(256), 0, st, dscores, w, B, L, D, n_out, doc_tgt, (float*)dx, lddx);
  else
    hipLaunchKernelGGL(switch_head_bwd_data_kernel<bf16_t>, grid, dim3(256), 0, st, dscores, w, B, L, D, n_out, doc_tgt, (bf16_t*)dx, lddx);
  MTS_LAUNCH_CHECK("mts_switch_head_bwd_data");
  return MTS_OK;
}
