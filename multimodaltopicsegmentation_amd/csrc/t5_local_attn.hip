// LongT5 local self-attention for gfx950: learned, bucketed relative-position bias inside a band softmax, forward saving the
// per-row log-sum-exp, backward recomputing P from it, and the gradient of the bias table.
//
// The encoder layer of RecurrentLongT5 (models/CRF.py:613-762 -> LongT5EncoderModel, HF modeling_longt5.py LongT5LocalAttention):
// per head, no 1/sqrt(d) scaling,
//     s_ij = q_i . k_j + T[bucket(j - i), h]
// Valid query rows i < len_b take the softmax over keys j in [i - r, i + r] and j < len_b.  Padded query rows (len_b <= i < L) have
// every key masked with -1e10, which absorbs the scores in fp32: the row is the UNIFORM mean
//     ctx_i = sum_{j in [(floor(i/(r+1)) - 1)(r+1), (floor(i/(r+1)) + 2)(r+1)) and 0 <= j < L} v_j / (3 (r + 1))
// (padded v rows included).  Padded rows carry no gradient (they never reach a valid row or the loss), so the backward writes dq = 0
// for them, dk = dv = 0 for padded keys, and never reads their dctx.
//
// Work decomposition on the helpers of attn_tile.h: one 256-thread workgroup per (document, head, tile of 32 rows); lane = (row
// t = tid/8, group g = tid%8); score-type products are 16-byte LDS dot products (v_dot2_f32_bf16 on bf16 pairs), accumulations stream
// 4-element chunks of the head dim.  The key (query) tiles a workgroup visits start at the first key (query) any of its rows can
// reach and stop after the last one; the mask removes the tiles' slack.
//
//   forward : per key tile S = Q K^T + bias, online softmax, acc += P V; ctx = acc / l, lse = m + log l.  Padded rows: the mean above.
//   dq      : per query tile; delta = rowsum(dCtx . ctx) saved; per key tile P = exp(S - lse), dS = P (dP - delta), dQ += dS K; the
//             tile's dS summed along each diagonal (fixed order) into per-offset sums -> this workgroup's slab of the workspace.
//   dk / dv : per key tile; per query tile the same P and dS, transposed; dV += P_dropped^T dCtx, dK += dS^T Q.
//   dtable  : per (head, offset) the slabs summed in a fixed order; then per (bucket, head) the offsets mapped to it, ascending.
// No atomics anywhere: bitwise reproducible.  Nothing L x L (or L x (2r+1)) ever touches memory.
#include "attn_tile.h"

#define TT 32            // rows per tile (queries and keys)
#define T5_MAX_RADIUS 1024

struct T5Args {
  const void* qkv; const int32_t* lengths; void* ctx; float* lse;
  const void* dctx; void* dqkv; float* delta;
  const float* table; const int32_t* bkt;   // [buckets, heads], [2r + 1]
  float* slab;                               // [B * ntiles * heads][2r + 1] per-workgroup diagonal sums of dS
  int B, L, heads, hd, inner, radius, buckets;
  int rs;                                    // LDS row stride (bytes) of staged rows
  float drop_scale; uint32_t drop_thr; uint64_t drop_seed;
};

// attention-probability dropout: keep decision of (activation row of the query, head, offset j - i)
__device__ __forceinline__ bool t5_keep(const T5Args& a, int grow, int h, int off) {
  return mts_hash32(a.drop_seed, ((uint64_t)grow * a.heads + h) * (uint64_t)(2 * a.radius + 1) + (uint64_t)(off + a.radius)) >= a.drop_thr;
}

__device__ __forceinline__ void t5_decode(const T5Args& a, int& tile, int& h, int& b) {
  const int ntiles = (a.L + TT - 1) / TT;
  decode_block(ntiles, a.heads, ntiles * a.heads * a.B, tile, h, b);
}

__device__ __forceinline__ int t5_len(const T5Args& a, int b) { return a.lengths ? max(1, min(a.lengths[b], a.L)) : a.L; }

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void t5_fwd_kernel(const T5Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;
  char* KVs = Qs + TT * a.rs;
  float* Ps = reinterpret_cast<float*>(KVs + TT * a.rs);
  float* bias_s = Ps + TT * PS;                       // [2r + 1] this head's bias per offset

  int tile, h, b;
  t5_decode(a, tile, h, b);
  const int len = t5_len(a, b), base = b * a.L, r = a.radius;
  const int i0 = tile * TT;
  const int t = threadIdx.x >> 3, g = threadIdx.x & 7;
  const int i = i0 + t;
  const int hd = a.hd, ld = 3 * a.inner;
  const T* qbase = reinterpret_cast<const T*>(a.qkv) + (size_t)base * ld + h * hd;
  float acc[2][4];
#pragma unroll
  for (int u = 0; u < 2; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.f;
  float m = -INFINITY, l = 0.f;

  if (i0 < len) {
    for (int d = threadIdx.x; d <= 2 * r; d += 256) bias_s[d] = a.table[(size_t)a.bkt[d] * a.heads + h];
    attn_stage_rows<T>(Qs, a.rs, qbase, ld, i0, TT, len, hd);
    const int jlo = max(0, i0 - r), jhi = min(len, min(i0 + TT, len) + r);
    for (int j0 = jlo; j0 < jhi; j0 += TT) {
      __syncthreads();                                 // previous tile's readers are done with KVs (first pass: bias_s, Qs are in)
      attn_stage_rows<T>(KVs, a.rs, qbase + a.inner, ld, j0, TT, jhi, hd);
      __syncthreads();
      float s[4];
      attn_scores<T>(Qs + t * a.rs, KVs + g * a.rs, a.rs, hd, s);
      float mt = -INFINITY;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int off = j0 + g + 8 * c - i;
        s[c] = (i < len && j0 + g + 8 * c < jhi && off >= -r && off <= r) ? s[c] + bias_s[off + r] : -INFINITY;
        mt = fmaxf(mt, s[c]);
      }
      const float mn = fmaxf(m, lanes8_max(mt));
      const float ms = mn == -INFINITY ? 0.f : mn;     // no key of this row in the tiles so far: p = 0 and nothing to rescale
      const float alpha = __expf(m - ms);
      float ps = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float p = __expf(s[c] - ms);
        ps += p;
        Ps[t * PS + g + 8 * c] = (a.drop_thr && p != 0.f) ? (t5_keep(a, base + i, h, j0 + g + 8 * c - i) ? p * a.drop_scale : 0.f) : p;
      }
      l = l * alpha + lanes8_sum(ps);
      m = mn;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u][e] *= alpha;
      __syncthreads();                                 // K scores done: KVs takes V
      attn_stage_rows<T>(KVs, a.rs, qbase + 2 * a.inner, ld, j0, TT, jhi, hd);
      __syncthreads();
      attn_accum<T, 2>(Ps + t * PS, 1, KVs, a.rs, 64, g, min(TT, jhi - j0), acc);
    }
  }
  if (i >= a.L) return;
  T* o = reinterpret_cast<T*>(a.ctx) + (size_t)(base + i) * a.inner + h * hd;
  if (i < len) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float v[4] = {acc[u][0] * inv, acc[u][1] * inv, acc[u][2] * inv, acc[u][3] * inv};
      store4<T>(o + 4 * (g + 8 * u), v);
    }
    if (g == 0) a.lse[(size_t)(base + i) * a.heads + h] = m + __logf(l);
  } else {                                             // padded row: uniform mean over its three blocks of r + 1 keys
    const int blk = r + 1, lo = (i / blk - 1) * blk;
    float sum[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const T* vb = qbase + 2 * a.inner;
    const int jend = min(a.L, lo + 3 * blk);
    for (int j = max(0, lo); j < jend; ++j) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float v[4];
        load4<T>(vb + (size_t)j * ld + 4 * (g + 8 * u), v);
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[u][e] += v[e];
      }
    }
    const float inv = 1.0f / (float)(3 * blk);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float v[4] = {sum[u][0] * inv, sum[u][1] * inv, sum[u][2] * inv, sum[u][3] * inv};
      store4<T>(o + 4 * (g + 8 * u), v);
    }
    if (g == 0) a.lse[(size_t)(base + i) * a.heads + h] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// backward, kernel 1: delta, dQ and the per-offset dS sums per query tile
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void t5_bwd_q_kernel(const T5Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;
  char* dOs = Qs + TT * a.rs;
  char* Ks = dOs + TT * a.rs;
  char* Vs = Ks + TT * a.rs;
  float* Ps = reinterpret_cast<float*>(Vs + TT * a.rs);
  float* bias_s = Ps + TT * PS;
  float* dsum = bias_s + (2 * a.radius + 1);           // [2r + 1] this workgroup's diagonal sums of dS

  int tile, h, b;
  t5_decode(a, tile, h, b);
  const int len = t5_len(a, b), base = b * a.L, r = a.radius, nd = 2 * r + 1;
  const int ntiles = (a.L + TT - 1) / TT;
  const int i0 = tile * TT;
  const int t = threadIdx.x >> 3, g = threadIdx.x & 7;
  const int i = i0 + t;
  const bool qok = i < len;
  const int hd = a.hd, ld = 3 * a.inner;
  const T* qbase = reinterpret_cast<const T*>(a.qkv) + (size_t)base * ld + h * hd;
  const T* dobase = reinterpret_cast<const T*>(a.dctx) + (size_t)base * a.inner + h * hd;
  const T* obase = reinterpret_cast<const T*>(a.ctx) + (size_t)base * a.inner + h * hd;
  float* slab = a.slab + ((size_t)(b * ntiles + tile) * a.heads + h) * nd;

  for (int d = threadIdx.x; d < nd; d += 256) {
    dsum[d] = 0.f;
    if (i0 < len) bias_s[d] = a.table[(size_t)a.bkt[d] * a.heads + h];
  }
  float acc[2][4];
#pragma unroll
  for (int u = 0; u < 2; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.f;
  if (i0 < len) {
    attn_stage_rows<T>(Qs, a.rs, qbase, ld, i0, TT, len, hd);
    attn_stage_rows<T>(dOs, a.rs, dobase, a.inner, i0, TT, len, hd);   // padded rows' dCtx is never read
    float delta = 0.f;
    if (qok) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float x[4], y[4];
        load4<T>(dobase + (size_t)i * a.inner + 4 * (g + 8 * u), x);
        load4<T>(obase + (size_t)i * a.inner + 4 * (g + 8 * u), y);
#pragma unroll
        for (int e = 0; e < 4; ++e) delta = fmaf(x[e], y[e], delta);
      }
    }
    delta = lanes8_sum(delta);
    const float lse = qok ? a.lse[(size_t)(base + i) * a.heads + h] : 0.f;
    if (qok && g == 0) a.delta[(size_t)(base + i) * a.heads + h] = delta;
    const int jlo = max(0, i0 - r), jhi = min(len, min(i0 + TT, len) + r);
    for (int j0 = jlo; j0 < jhi; j0 += TT) {
      __syncthreads();
      attn_stage_rows<T>(Ks, a.rs, qbase + a.inner, ld, j0, TT, jhi, hd);
      attn_stage_rows<T>(Vs, a.rs, qbase + 2 * a.inner, ld, j0, TT, jhi, hd);
      __syncthreads();
      float s[4], dp[4];
      attn_scores<T>(Qs + t * a.rs, Ks + g * a.rs, a.rs, hd, s);
      attn_scores<T>(dOs + t * a.rs, Vs + g * a.rs, a.rs, hd, dp);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + g + 8 * c, off = j - i;
        const bool in = qok && j < jhi && off >= -r && off <= r;
        const float p = in ? __expf(s[c] + bias_s[off + r] - lse) : 0.f;
        float d = dp[c];
        if (a.drop_thr) d = (in && t5_keep(a, base + i, h, off)) ? d * a.drop_scale : 0.f;
        Ps[t * PS + g + 8 * c] = p * (d - delta);
      }
      __syncthreads();
      // the tile's dS summed along each diagonal: thread q < 63 owns offset j0 - i0 - 31 + q (distinct per thread), rows in order
      if (threadIdx.x < 2 * TT - 1) {
        const int off = j0 - i0 - (TT - 1) + (int)threadIdx.x;
        if (off >= -r && off <= r) {
          float sacc = 0.f;
          for (int tt = 0; tt < TT; ++tt) {
            const int jj = i0 + tt + off - j0;
            if (jj >= 0 && jj < TT) sacc += Ps[tt * PS + jj];
          }
          dsum[off + r] += sacc;
        }
      }
      attn_accum<T, 2>(Ps + t * PS, 1, Ks, a.rs, 64, g, min(TT, jhi - j0), acc);
    }
  }
  __syncthreads();
  for (int d = threadIdx.x; d < nd; d += 256) slab[d] = dsum[d];
  if (i < a.L) {                                       // dq (0 for padded rows)
    T* o = reinterpret_cast<T*>(a.dqkv) + (size_t)(base + i) * ld + h * hd;
#pragma unroll
    for (int u = 0; u < 2; ++u) store4<T>(o + 4 * (g + 8 * u), acc[u]);
  }
}

// ------------------------------------------------------------------------------------------------
// backward, kernel 2: dK and dV per key tile (reads the delta kernel 1 saved)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void t5_bwd_kv_kernel(const T5Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = Ks + TT * a.rs;
  char* Qs = Vs + TT * a.rs;
  char* dOs = Qs + TT * a.rs;
  float* PT = reinterpret_cast<float*>(dOs + TT * a.rs);   // [key][query] dropped probabilities
  float* ST = PT + TT * PS;                                // [key][query] dS
  float* lse_s = ST + TT * PS;
  float* del_s = lse_s + TT;
  float* bias_s = del_s + TT;

  int tile, h, b;
  t5_decode(a, tile, h, b);
  const int len = t5_len(a, b), base = b * a.L, r = a.radius;
  const int j0 = tile * TT;
  const int t = threadIdx.x >> 3, g = threadIdx.x & 7;
  const int j = j0 + t;
  const int hd = a.hd, ld = 3 * a.inner;
  const T* qbase = reinterpret_cast<const T*>(a.qkv) + (size_t)base * ld + h * hd;
  const T* dobase = reinterpret_cast<const T*>(a.dctx) + (size_t)base * a.inner + h * hd;
  float dk[2][4], dv[2][4];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) dk[u][e] = dv[u][e] = 0.f;

  if (j0 < len) {                                      // padded keys: probability 0, gradient 0
    for (int d = threadIdx.x; d <= 2 * r; d += 256) bias_s[d] = a.table[(size_t)a.bkt[d] * a.heads + h];
    attn_stage_rows<T>(Ks, a.rs, qbase + a.inner, ld, j0, TT, len, hd);
    attn_stage_rows<T>(Vs, a.rs, qbase + 2 * a.inner, ld, j0, TT, len, hd);
    const int ilo = max(0, j0 - r), ihi = min(len, min(j0 + TT, len) + r);
    for (int q0 = ilo; q0 < ihi; q0 += TT) {
      __syncthreads();
      attn_stage_rows<T>(Qs, a.rs, qbase, ld, q0, TT, ihi, hd);
      attn_stage_rows<T>(dOs, a.rs, dobase, a.inner, q0, TT, ihi, hd);
      if (threadIdx.x < TT) {
        const int i = q0 + threadIdx.x;
        const bool ok = i < ihi;
        lse_s[threadIdx.x] = ok ? a.lse[(size_t)(base + i) * a.heads + h] : 0.f;
        del_s[threadIdx.x] = ok ? a.delta[(size_t)(base + i) * a.heads + h] : 0.f;
      }
      __syncthreads();
      float s[4], dp[4];
      attn_scores<T>(Ks + t * a.rs, Qs + g * a.rs, a.rs, hd, s);
      attn_scores<T>(Vs + t * a.rs, dOs + g * a.rs, a.rs, hd, dp);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ci = g + 8 * c, i = q0 + ci, off = j - i;
        const bool in = j < len && i < ihi && off >= -r && off <= r;
        const float p = in ? __expf(s[c] + bias_s[off + r] - lse_s[ci]) : 0.f;
        float keep = 1.f;
        if (a.drop_thr) keep = (in && t5_keep(a, base + i, h, off)) ? a.drop_scale : 0.f;
        PT[t * PS + ci] = p * keep;
        ST[t * PS + ci] = p * (dp[c] * keep - del_s[ci]);
      }
      __syncthreads();
      const int ncq = min(TT, ihi - q0);
      attn_accum<T, 2>(PT + t * PS, 1, dOs, a.rs, 64, g, ncq, dv);
      attn_accum<T, 2>(ST + t * PS, 1, Qs, a.rs, 64, g, ncq, dk);
    }
  }
  if (j < a.L) {
    T* o = reinterpret_cast<T*>(a.dqkv) + (size_t)(base + j) * ld + h * hd;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      store4<T>(o + a.inner + 4 * (g + 8 * u), dk[u]);
      store4<T>(o + 2 * a.inner + 4 * (g + 8 * u), dv[u]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward, dtable: offsets summed over the slabs (fixed order), then scattered to buckets in ascending offset
// ------------------------------------------------------------------------------------------------
// grid (ceil((2r + 1) / 16), heads); thread = (part p = tid / 16, offset = 16 blockIdx.x + tid % 16): part p sums slabs p, p + 16, ...
// in order, then parts 0 .. 15 in order
__global__ __launch_bounds__(256) void t5_offset_sum_kernel(const T5Args a, int nslabs, float* __restrict__ osum) {
  __shared__ float part[16][16];
  const int nd = 2 * a.radius + 1, h = blockIdx.y;
  const int q = threadIdx.x & 15, p = threadIdx.x >> 4, d = blockIdx.x * 16 + q;
  float s = 0.f;
  if (d < nd)
    for (int w = p; w < nslabs; w += 16) s += a.slab[((size_t)w * a.heads + h) * nd + d];
  part[p][q] = s;
  __syncthreads();
  if (p == 0 && d < nd) {
    float t = part[0][q];
    for (int k = 1; k < 16; ++k) t += part[k][q];
    osum[(size_t)h * nd + d] = t;
  }
}

__global__ __launch_bounds__(256) void t5_bucket_scatter_kernel(const T5Args a, const float* __restrict__ osum, float* __restrict__ dtable) {
  const int idx = blockIdx.x * 256 + threadIdx.x;     // = bucket * heads + h
  if (idx >= a.buckets * a.heads) return;
  const int bucket = idx / a.heads, h = idx % a.heads, nd = 2 * a.radius + 1;
  float s = 0.f;                                      // buckets no offset maps to: exactly 0
  for (int d = 0; d < nd; ++d)
    if (a.bkt[d] == bucket) s += osum[(size_t)h * nd + d];
  dtable[idx] = s;
}

// ------------------------------------------------------------------------------------------------
// bf16 matrix-core path (head dim 64): v_mfma_f32_16x16x32_bf16, 4 waves x 16 rows per workgroup -- the fragment layout of
// attn_tile.h (every product X . Y^T from row-major LDS images) restricted to the band, plus the bias and the padded-row rule.
//   forward : workgroup = 64 queries; per 32-key tile of the band S = Q K^T + bias, online softmax on the C fragments, P (bf16) ->
//             LDS, ctx += P Vt^T.  Padded rows of the tile: the uniform mean, one thread per (row, 4 dims).
//   dq      : workgroup = 64 queries; dS (bf16) -> LDS for dQ += dS Kt^T, and in fp32 to a second tile whose 95 diagonals threads
//             < 95 sum (one per offset, rows in order) into the workgroup's slab, as the generic kernel does.
//   dk / dv : workgroup = 64 keys; per 32-query tile of the band S^T = K Q^T, dP^T = V dO^T, dV += P^T dOt^T, dK += dS^T Qt^T.
// Fixed tiles and loop orders, no atomics: bitwise reproducible.  mts_set_option("t5_mfma", 0) sends bf16 to the generic kernels.
// ------------------------------------------------------------------------------------------------
#define MKK 2                   // 32-wide k-steps of the head dim
#define MNT 4                   // 16-wide tiles of the head dim
#define DSS (MK + 1)            // LDS row stride (floats) of the fp32 dS tile

// padded query rows [first, end) of document b (activation rows base + i), head h: the uniform mean of their three blocks of r + 1
// rows of v, j in order; one thread per (row, 4 dims)
__device__ void t5m_padded_mean(const T5Args& a, int base, int h, int first, int end) {
  const int blk = a.radius + 1, ld = 3 * a.inner;
  const bf16_t* vb = reinterpret_cast<const bf16_t*>(a.qkv) + (size_t)base * ld + 2 * a.inner + h * 64;
  const float inv = 1.0f / (float)(3 * blk);
  for (int idx = threadIdx.x; idx < (end - first) * 16; idx += 256) {
    const int i = first + (idx >> 4), ch = idx & 15;
    const int lo = (i / blk - 1) * blk, jend = min(a.L, lo + 3 * blk);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = max(0, lo); j < jend; ++j) {
      float v[4];
      load4<bf16_t>(vb + (size_t)j * ld + 4 * ch, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += v[e];
    }
    float o[4] = {s[0] * inv, s[1] * inv, s[2] * inv, s[3] * inv};
    store4<bf16_t>(reinterpret_cast<bf16_t*>(a.ctx) + (size_t)(base + i) * a.inner + h * 64 + 4 * ch, o);
    if (ch == 0) a.lse[(size_t)(base + i) * a.heads + h] = 0.f;
  }
}

__global__ __launch_bounds__(256) void t5m_fwd_kernel(const T5Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;                                   // [64][rs]
  char* Ks = Qs + MQ * a.rs;                         // [32][rs]
  char* Vt = Ks + MK * a.rs;                         // [64 dims][TRS]
  char* Pw = Vt + 64 * TRS;                          // [wave][16][TRS]
  float* bias_s = reinterpret_cast<float*>(Pw + 4 * 16 * TRS);
  const int ntiles = (a.L + MQ - 1) / MQ;
  int tile, h, b;
  decode_block(ntiles, a.heads, ntiles * a.heads * a.B, tile, h, b);
  const int len = t5_len(a, b), base = b * a.L, r = a.radius;
  const int q0 = tile * MQ;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int ld = 3 * a.inner;
  const bf16_t* qbase = reinterpret_cast<const bf16_t*>(a.qkv) + (size_t)base * ld + h * 64;
  char* W = Pw + w * 16 * TRS;
  if (q0 < len) {
    for (int d = threadIdx.x; d <= 2 * r; d += 256) bias_s[d] = a.table[(size_t)a.bkt[d] * a.heads + h];
    attn_mstage(Qs, a.rs, nullptr, qbase, ld, q0, MQ / 2, len, 64);
    attn_mstage(Qs + (MQ / 2) * a.rs, a.rs, nullptr, qbase, ld, q0 + MQ / 2, MQ / 2, len, 64);
    float m[4], l[4];
    f32x4 acc[MNT];
#pragma unroll
    for (int q = 0; q < 4; ++q) { m[q] = -INFINITY; l[q] = 0.f; }
#pragma unroll
    for (int n = 0; n < MNT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int jlo = max(0, q0 - r), jhi = min(len, min(q0 + MQ, len) + r);
    for (int j0 = jlo; j0 < jhi; j0 += MK) {
      __syncthreads();                               // previous step's readers are done with Ks / Vt (first pass: bias_s, Qs are in)
      attn_mstage(Ks, a.rs, nullptr, qbase + a.inner, ld, j0, MK, jhi, 64);
      attn_mstage(nullptr, 0, Vt, qbase + 2 * a.inner, ld, j0, MK, jhi, 64);
      __syncthreads();
      f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      attn_mm_xyt<2>(Qs, a.rs, 16 * w, Ks, a.rs, MKK, lane, s);
      float p[2][4], alpha[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = q0 + 16 * w + 4 * g + q;
        float mt = -INFINITY;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int j = j0 + 16 * ct + l15, off = j - i;
          s[ct][q] = (i < len && j < jhi && off >= -r && off <= r) ? s[ct][q] + bias_s[off + r] : -INFINITY;
          mt = fmaxf(mt, s[ct][q]);
        }
        const float mn = fmaxf(m[q], lanes16_max(mt));
        const float ms = mn == -INFINITY ? 0.f : mn;   // no key of this row so far: p = 0 and nothing to rescale
        alpha[q] = __expf(m[q] - ms);
        float ps = 0.f;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const float e = __expf(s[ct][q] - ms);
          ps += e;
          const int off = j0 + 16 * ct + l15 - i;
          p[ct][q] = (a.drop_thr && e != 0.f) ? (t5_keep(a, base + i, h, off) ? e * a.drop_scale : 0.f) : e;
        }
        l[q] = l[q] * alpha[q] + lanes16_sum(ps);
        m[q] = mn;
      }
#pragma unroll
      for (int n = 0; n < MNT; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[n][q] *= alpha[q];
      attn_put_coef(W, lane, p);
      __syncthreads();
      attn_mm_xyt<MNT>(W, TRS, 0, Vt, TRS, 1, lane, acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = q0 + 16 * w + 4 * g + q;
      if (i < len) {
        const float inv = 1.0f / l[q];
        bf16_t* o = reinterpret_cast<bf16_t*>(a.ctx) + (size_t)(base + i) * a.inner + h * 64;
#pragma unroll
        for (int n = 0; n < MNT; ++n) o[16 * n + l15] = (bf16_t)(acc[n][q] * inv);
        if (l15 == 0) a.lse[(size_t)(base + i) * a.heads + h] = m[q] + __logf(l[q]);
      }
    }
  }
  const int pfirst = max(q0, len), pend = min(a.L, q0 + MQ);
  if (pfirst < pend) t5m_padded_mean(a, base, h, pfirst, pend);
}

__global__ __launch_bounds__(256) void t5m_bwd_q_kernel(const T5Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;                                   // [64][rs]
  char* dOs = Qs + MQ * a.rs;                        // [64][rs]
  char* Ks = dOs + MQ * a.rs;                        // [32][rs]
  char* Vs = Ks + MK * a.rs;                         // [32][rs]
  char* Kt = Vs + MK * a.rs;                         // [64 dims][TRS]
  char* Pw = Kt + 64 * TRS;                          // [wave][16][TRS] dS (bf16)
  float* row_s = reinterpret_cast<float*>(Pw + 4 * 16 * TRS);   // [64] lse, [64] delta
  float* DS = row_s + 2 * MQ;                        // [64][DSS] dS (fp32)
  float* bias_s = DS + MQ * DSS;                     // [2r + 1]
  float* dsum = bias_s + (2 * a.radius + 1);         // [2r + 1]
  const int ntiles = (a.L + MQ - 1) / MQ;
  int tile, h, b;
  decode_block(ntiles, a.heads, ntiles * a.heads * a.B, tile, h, b);
  const int len = t5_len(a, b), base = b * a.L, r = a.radius, nd = 2 * r + 1;
  const int q0 = tile * MQ;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int ld = 3 * a.inner;
  const bf16_t* qbase = reinterpret_cast<const bf16_t*>(a.qkv) + (size_t)base * ld + h * 64;
  const bf16_t* dobase = reinterpret_cast<const bf16_t*>(a.dctx) + (size_t)base * a.inner + h * 64;
  const bf16_t* obase = reinterpret_cast<const bf16_t*>(a.ctx) + (size_t)base * a.inner + h * 64;
  float* slab = a.slab + ((size_t)(b * ntiles + tile) * a.heads + h) * nd;
  char* W = Pw + w * 16 * TRS;
  for (int d = threadIdx.x; d < nd; d += 256) {
    dsum[d] = 0.f;
    if (q0 < len) bias_s[d] = a.table[(size_t)a.bkt[d] * a.heads + h];
  }
  f32x4 acc[MNT];
#pragma unroll
  for (int n = 0; n < MNT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (q0 < len) {
    attn_mstage(Qs, a.rs, nullptr, qbase, ld, q0, MQ / 2, len, 64);
    attn_mstage(Qs + (MQ / 2) * a.rs, a.rs, nullptr, qbase, ld, q0 + MQ / 2, MQ / 2, len, 64);
    attn_mstage(dOs, a.rs, nullptr, dobase, a.inner, q0, MQ / 2, len, 64);              // padded rows' dCtx is never read
    attn_mstage(dOs + (MQ / 2) * a.rs, a.rs, nullptr, dobase, a.inner, q0 + MQ / 2, MQ / 2, len, 64);
    if (threadIdx.x < MQ) {                          // delta = dCtx . ctx (fixed order) and lse of valid rows
      const int i = q0 + threadIdx.x;
      float dl = 0.f, lv = 0.f;
      if (i < len) {
        for (int c = 0; c < 64; c += 4) {
          float x[4], y[4];
          load4<bf16_t>(dobase + (size_t)i * a.inner + c, x);
          load4<bf16_t>(obase + (size_t)i * a.inner + c, y);
#pragma unroll
          for (int e = 0; e < 4; ++e) dl = fmaf(x[e], y[e], dl);
        }
        lv = a.lse[(size_t)(base + i) * a.heads + h];
        a.delta[(size_t)(base + i) * a.heads + h] = dl;
      }
      row_s[threadIdx.x] = lv;
      row_s[MQ + threadIdx.x] = dl;
    }
    const int jlo = max(0, q0 - r), jhi = min(len, min(q0 + MQ, len) + r);
    for (int j0 = jlo; j0 < jhi; j0 += MK) {
      __syncthreads();
      attn_mstage(Ks, a.rs, Kt, qbase + a.inner, ld, j0, MK, jhi, 64);
      attn_mstage(Vs, a.rs, nullptr, qbase + 2 * a.inner, ld, j0, MK, jhi, 64);
      __syncthreads();
      f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      f32x4 dp[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      attn_mm_xyt<2>(Qs, a.rs, 16 * w, Ks, a.rs, MKK, lane, s);
      attn_mm_xyt<2>(dOs, a.rs, 16 * w, Vs, a.rs, MKK, lane, dp);
      float ds[2][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ri = 16 * w + 4 * g + q, i = q0 + ri;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int j = j0 + 16 * ct + l15, off = j - i;
          const bool in = i < len && j < jhi && off >= -r && off <= r;
          const float p = in ? __expf(s[ct][q] + bias_s[off + r] - row_s[ri]) : 0.f;
          float d = dp[ct][q];
          if (a.drop_thr) d = (in && t5_keep(a, base + i, h, off)) ? d * a.drop_scale : 0.f;
          ds[ct][q] = p * (d - row_s[MQ + ri]);
          DS[ri * DSS + 16 * ct + l15] = ds[ct][q];
        }
      }
      attn_put_coef(W, lane, ds);
      __syncthreads();
      // the step's dS summed along each diagonal: thread q < 95 owns offset j0 - q0 - 63 + q (distinct per thread), rows in order
      if (threadIdx.x < MQ + MK - 1) {
        const int off = j0 - q0 - (MQ - 1) + (int)threadIdx.x;
        if (off >= -r && off <= r) {
          float sacc = 0.f;
          for (int tt = 0; tt < MQ; ++tt) {
            const int jj = q0 + tt + off - j0;
            if (jj >= 0 && jj < MK) sacc += DS[tt * DSS + jj];
          }
          dsum[off + r] += sacc;
        }
      }
      attn_mm_xyt<MNT>(W, TRS, 0, Kt, TRS, 1, lane, acc);
    }
  }
  __syncthreads();
  for (int d = threadIdx.x; d < nd; d += 256) slab[d] = dsum[d];
#pragma unroll
  for (int q = 0; q < 4; ++q) {                      // dq (0 for padded rows)
    const int i = q0 + 16 * w + 4 * g + q;
    if (i < a.L) {
      bf16_t* o = reinterpret_cast<bf16_t*>(a.dqkv) + (size_t)(base + i) * ld + h * 64;
#pragma unroll
      for (int n = 0; n < MNT; ++n) o[16 * n + l15] = (bf16_t)acc[n][q];
    }
  }
}

__global__ __launch_bounds__(256) void t5m_bwd_kv_kernel(const T5Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;                                   // [64][rs]
  char* Vs = Ks + MQ * a.rs;                         // [64][rs]
  char* Qs = Vs + MQ * a.rs;                         // [32][rs]
  char* dOs = Qs + MK * a.rs;                        // [32][rs]
  char* Qt = dOs + MK * a.rs;                        // [64 dims][TRS]
  char* dOt = Qt + 64 * TRS;                         // [64 dims][TRS]
  char* Pw = dOt + 64 * TRS;                         // [wave][16 keys][32 queries] P^T (dropped)
  char* Sw = Pw + 4 * 16 * TRS;                      // ... dS^T
  float* lse_s = reinterpret_cast<float*>(Sw + 4 * 16 * TRS);
  float* del_s = lse_s + MK;
  float* bias_s = del_s + MK;
  const int ntiles = (a.L + MQ - 1) / MQ;
  int tile, h, b;
  decode_block(ntiles, a.heads, ntiles * a.heads * a.B, tile, h, b);
  const int len = t5_len(a, b), base = b * a.L, r = a.radius;
  const int k0 = tile * MQ;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int ld = 3 * a.inner;
  const bf16_t* qbase = reinterpret_cast<const bf16_t*>(a.qkv) + (size_t)base * ld + h * 64;
  const bf16_t* dobase = reinterpret_cast<const bf16_t*>(a.dctx) + (size_t)base * a.inner + h * 64;
  f32x4 dk[MNT], dv[MNT];
#pragma unroll
  for (int n = 0; n < MNT; ++n) dk[n] = dv[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (k0 < len) {                                    // padded keys: gradient 0
    for (int d = threadIdx.x; d <= 2 * r; d += 256) bias_s[d] = a.table[(size_t)a.bkt[d] * a.heads + h];
    attn_mstage(Ks, a.rs, nullptr, qbase + a.inner, ld, k0, MQ / 2, len, 64);
    attn_mstage(Ks + (MQ / 2) * a.rs, a.rs, nullptr, qbase + a.inner, ld, k0 + MQ / 2, MQ / 2, len, 64);
    attn_mstage(Vs, a.rs, nullptr, qbase + 2 * a.inner, ld, k0, MQ / 2, len, 64);
    attn_mstage(Vs + (MQ / 2) * a.rs, a.rs, nullptr, qbase + 2 * a.inner, ld, k0 + MQ / 2, MQ / 2, len, 64);
    char* PW = Pw + w * 16 * TRS;
    char* SW = Sw + w * 16 * TRS;
    const int ilo = max(0, k0 - r), ihi = min(len, min(k0 + MQ, len) + r);
    for (int i0 = ilo; i0 < ihi; i0 += MK) {
      __syncthreads();
      attn_mstage(Qs, a.rs, Qt, qbase, ld, i0, MK, ihi, 64);
      attn_mstage(dOs, a.rs, dOt, dobase, a.inner, i0, MK, ihi, 64);
      if (threadIdx.x < MK) {
        const int i = i0 + threadIdx.x;
        const bool ok = i < ihi;
        lse_s[threadIdx.x] = ok ? a.lse[(size_t)(base + i) * a.heads + h] : 0.f;
        del_s[threadIdx.x] = ok ? a.delta[(size_t)(base + i) * a.heads + h] : 0.f;
      }
      __syncthreads();
      f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      f32x4 dp[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      attn_mm_xyt<2>(Ks, a.rs, 16 * w, Qs, a.rs, MKK, lane, s);      // S^T: rows = keys, columns = queries
      attn_mm_xyt<2>(Vs, a.rs, 16 * w, dOs, a.rs, MKK, lane, dp);    // dP^T
      float pt[2][4], st[2][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = k0 + 16 * w + 4 * g + q;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int ci = 16 * ct + l15, i = i0 + ci, off = j - i;
          const bool in = j < len && i < ihi && off >= -r && off <= r;
          const float p = in ? __expf(s[ct][q] + bias_s[off + r] - lse_s[ci]) : 0.f;
          float keep = 1.f;
          if (a.drop_thr) keep = (in && t5_keep(a, base + i, h, off)) ? a.drop_scale : 0.f;
          pt[ct][q] = p * keep;
          st[ct][q] = p * (dp[ct][q] * keep - del_s[ci]);
        }
      }
      attn_put_coef(PW, lane, pt);
      attn_put_coef(SW, lane, st);
      __syncthreads();
      attn_mm_xyt<MNT>(PW, TRS, 0, dOt, TRS, 1, lane, dv);
      attn_mm_xyt<MNT>(SW, TRS, 0, Qt, TRS, 1, lane, dk);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = k0 + 16 * w + 4 * g + q;
    if (j < a.L) {
      bf16_t* o = reinterpret_cast<bf16_t*>(a.dqkv) + (size_t)(base + j) * ld + h * 64;
#pragma unroll
      for (int n = 0; n < MNT; ++n) {
        o[a.inner + 16 * n + l15] = (bf16_t)dk[n][q];
        o[2 * a.inner + 16 * n + l15] = (bf16_t)dv[n][q];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int t5_fill(T5Args& a, int dtype, int B, int L, int heads, int head_dim, int radius, int buckets, const char* who) {
  MTS_CHECK_ARG(B > 0 && L > 0 && heads > 0 && radius >= 1 && buckets >= 1, "%s: bad shape", who);
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "%s: bad dtype %d", who, dtype);
  MTS_UNSUPPORTED(head_dim == 64, "%s: head dim %d (only 64, LongT5's d_kv, is covered)", who, head_dim);
  MTS_UNSUPPORTED(radius <= T5_MAX_RADIUS, "%s: radius %d > %d", who, radius, T5_MAX_RADIUS);
  MTS_UNSUPPORTED((long)B * L * heads * 64 * 3 < (1L << 31), "%s: problem too large for 32-bit row indexing", who);
  memset(&a, 0, sizeof(a));
  a.B = B; a.L = L; a.heads = heads; a.hd = head_dim; a.inner = heads * head_dim; a.radius = radius; a.buckets = buckets;
  a.rs = attn_row_stride(head_dim, dtype == MTS_F32 ? 4 : 2);
  a.drop_scale = 1.f;
  return MTS_OK;
}

// LDS of the generic kernels (at most 56 KiB at the largest radius: no attribute call needed)
static size_t t5_fwd_lds(const T5Args& a) { return (size_t)2 * TT * a.rs + (size_t)(TT * PS + 2 * a.radius + 1) * sizeof(float); }
static size_t t5_bwd_q_lds(const T5Args& a) { return (size_t)4 * TT * a.rs + (size_t)(TT * PS + 2 * (2 * a.radius + 1)) * sizeof(float); }
static size_t t5_bwd_kv_lds(const T5Args& a) {
  return (size_t)4 * TT * a.rs + (size_t)(2 * TT * PS + 2 * TT + 2 * a.radius + 1) * sizeof(float);
}

// matrix-core kernels (bf16): at most 62 KiB at the largest radius
static size_t t5m_fwd_lds(const T5Args& a) { return (size_t)(MQ + MK) * a.rs + (size_t)2 * 64 * TRS + (size_t)(2 * a.radius + 1) * sizeof(float); }
static size_t t5m_bwd_q_lds(const T5Args& a) {
  return (size_t)2 * (MQ + MK) * a.rs + (size_t)2 * 64 * TRS + (size_t)(2 * MQ + MQ * DSS + 2 * (2 * a.radius + 1)) * sizeof(float);
}
static size_t t5m_bwd_kv_lds(const T5Args& a) {
  return (size_t)2 * (MQ + MK) * a.rs + (size_t)4 * 64 * TRS + (size_t)(2 * MK + 2 * a.radius + 1) * sizeof(float);
}

static thread_local int g_t5_mfma = 1;     // mts_set_option("t5_mfma", 0) sends bf16 to the generic kernels (A/B testing)
void mts_t5_set_mfma(int on) { g_t5_mfma = on; }
static bool t5_use_mfma(const T5Args& a, int dtype) { return dtype == MTS_BF16 && g_t5_mfma && a.hd == 64; }

static bool t5_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static size_t t5_slab_floats(int B, int L, int heads, int radius) {
  return (size_t)B * ceil_div(L, TT) * heads * (2 * (size_t)radius + 1);
}

extern "C" int mts_t5_local_attn_fwd(void* stream, int dtype, int B, int L, int heads, int head_dim, int radius, const void* qkv,
                                     const int32_t* lengths, const float* table, int buckets, const int32_t* bucket_of_offset, void* ctx,
                                     float* lse, float drop_p, uint64_t drop_seed) {
  T5Args a;
  int rc = t5_fill(a, dtype, B, L, heads, head_dim, radius, buckets, "mts_t5_local_attn_fwd");
  if (rc) return rc;
  MTS_CHECK_ARG(qkv && table && bucket_of_offset && ctx && lse, "mts_t5_local_attn_fwd: null pointer");
  MTS_UNSUPPORTED(t5_aligned16(qkv) && t5_aligned16(ctx), "mts_t5_local_attn_fwd: qkv and ctx must be 16-byte aligned");
  rc = attn_set_dropout(a, drop_p, drop_seed, "mts_t5_local_attn_fwd");
  if (rc) return rc;
  a.qkv = qkv; a.lengths = lengths; a.table = table; a.bkt = bucket_of_offset; a.ctx = ctx; a.lse = lse;
  if (t5_use_mfma(a, dtype)) {
    hipLaunchKernelGGL(t5m_fwd_kernel, dim3(ceil_div(L, MQ) * heads * B), dim3(256), t5m_fwd_lds(a), (hipStream_t)stream, a);
    MTS_LAUNCH_CHECK("mts_t5_local_attn_fwd");
    return MTS_OK;
  }
  const size_t lds = t5_fwd_lds(a);
  const dim3 grid(ceil_div(L, TT) * heads * B);
  if (dtype == MTS_F32) hipLaunchKernelGGL(t5_fwd_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(t5_fwd_kernel<bf16_t>, grid, dim3(256), lds, (hipStream_t)stream, a);
  MTS_LAUNCH_CHECK("mts_t5_local_attn_fwd");
  return MTS_OK;
}

extern "C" size_t mts_t5_local_attn_bwd_workspace(int B, int L, int heads, int radius) {
  B = std::max(B, 1); L = std::max(L, 1); heads = std::max(heads, 1); radius = std::max(radius, 1);
  return align_up((size_t)B * L * heads * sizeof(float), 256) + align_up(t5_slab_floats(B, L, heads, radius) * sizeof(float), 256) +
         align_up((size_t)heads * (2 * radius + 1) * sizeof(float), 256);
}

extern "C" int mts_t5_local_attn_bwd(void* stream, int dtype, int B, int L, int heads, int head_dim, int radius, const void* qkv,
                                     const int32_t* lengths, const float* table, int buckets, const int32_t* bucket_of_offset,
                                     const float* lse, const void* ctx, const void* dctx, void* dqkv, float* dtable, void* workspace,
                                     float drop_p, uint64_t drop_seed) {
  T5Args a;
  int rc = t5_fill(a, dtype, B, L, heads, head_dim, radius, buckets, "mts_t5_local_attn_bwd");
  if (rc) return rc;
  MTS_CHECK_ARG(qkv && table && bucket_of_offset && lse && ctx && dctx && dqkv && dtable && workspace,
                "mts_t5_local_attn_bwd: null pointer (workspace is required)");
  MTS_UNSUPPORTED(t5_aligned16(qkv) && t5_aligned16(ctx) && t5_aligned16(dctx) && t5_aligned16(dqkv),
                  "mts_t5_local_attn_bwd: qkv, ctx, dctx and dqkv must be 16-byte aligned");
  rc = attn_set_dropout(a, drop_p, drop_seed, "mts_t5_local_attn_bwd");
  if (rc) return rc;
  a.qkv = qkv; a.lengths = lengths; a.table = table; a.bkt = bucket_of_offset; a.lse = const_cast<float*>(lse);
  a.ctx = const_cast<void*>(ctx); a.dctx = dctx; a.dqkv = dqkv;
  char* ws = (char*)workspace;
  a.delta = (float*)ws;
  ws += align_up((size_t)B * L * heads * sizeof(float), 256);
  a.slab = (float*)ws;
  ws += align_up(t5_slab_floats(B, L, heads, radius) * sizeof(float), 256);
  float* osum = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  int nslabs = B * ceil_div(L, TT);
  if (t5_use_mfma(a, dtype)) {
    const dim3 grid(ceil_div(L, MQ) * heads * B);
    hipLaunchKernelGGL(t5m_bwd_q_kernel, grid, dim3(256), t5m_bwd_q_lds(a), st, a);
    hipLaunchKernelGGL(t5m_bwd_kv_kernel, grid, dim3(256), t5m_bwd_kv_lds(a), st, a);
    nslabs = B * ceil_div(L, MQ);
  } else {
    const dim3 grid(ceil_div(L, TT) * heads * B);
    const size_t lq = t5_bwd_q_lds(a), lkv = t5_bwd_kv_lds(a);
    if (dtype == MTS_F32) {
      hipLaunchKernelGGL(t5_bwd_q_kernel<float>, grid, dim3(256), lq, st, a);
      hipLaunchKernelGGL(t5_bwd_kv_kernel<float>, grid, dim3(256), lkv, st, a);
    } else {
      hipLaunchKernelGGL(t5_bwd_q_kernel<bf16_t>, grid, dim3(256), lq, st, a);
      hipLaunchKernelGGL(t5_bwd_kv_kernel<bf16_t>, grid, dim3(256), lkv, st, a);
    }
  }
  hipLaunchKernelGGL(t5_offset_sum_kernel, dim3(ceil_div(2 * radius + 1, 16), heads), dim3(256), 0, st, a, nslabs, osum);
  hipLaunchKernelGGL(t5_bucket_scatter_kernel, dim3(ceil_div(buckets * heads, 256)), dim3(256), 0, st, a, (const float*)osum, dtable);
  MTS_LAUNCH_CHECK("mts_t5_local_attn_bwd");
  return MTS_OK;
}
