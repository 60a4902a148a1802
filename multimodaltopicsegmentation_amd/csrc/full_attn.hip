// Full (all-keys) self-attention for gfx950: forward saving the per-row log-sum-exp, backward recomputing P from it.
//
// The encoder of Transformer_segmenter(restricted=False) (models/CRF.py:543-549, models/RestrictedTransformerLayer.py:16-63:
// a BertModel): per head, softmax over every VALID key of the document (j < len_b; padded keys get probability 0, so key tiles
// at or past len_b are never visited), q pre-scaled by 1/sqrt(hd).  Padded query rows are NOT zeroed (BERT has no such step):
// on the padded [B, L] layout they attend to the document's valid keys like any other row.
//
// Work decomposition (the lane layout and helpers of attn_tile.h): one 256-thread workgroup per (document, head, tile of 32
// rows); lane = (row t = tid/8, group g = tid%8).  Score-type products <A[t], B[g + 8c]>, c = 0..3, are 16-byte LDS dot products
// (v_dot2_f32_bf16 on bf16 pairs); accumulations over 32 coefficients stream 4-element chunks g + 8u of the head dim.
//
//   forward     : per key tile, stage K -> scores -> online softmax (running max m, sum l; the accumulator is rescaled by
//                 exp(m_old - m_new)) -> stage V -> acc += p V.  ctx = acc / l, lse = m + log l.
//   backward dq : per query tile; delta = rowsum(dCtx . ctx), saved for the second kernel; per key tile P = exp(S - lse),
//                 dP = dCtx V^T (through the dropout mask), dS = P (dP - delta), dQ += dS K.
//   backward kv : per KEY tile; per query tile the same P and dS, transposed through LDS; dV += P_dropped^T dCtx, dK += dS^T Q.
// Two kernels, fixed loop orders, no atomics: bitwise reproducible.  Nothing N x N ever touches memory.
// bf16 at head dims that are multiples of 32 (<= 256) takes the matrix-core kernels further down instead (option "full_mfma").
#include "attn_tile.h"

#define FT 32   // rows per tile (queries and keys)

struct FullArgs {
  const void* qkv; const int32_t* lengths; void* ctx; float* lse;
  const void* dctx; void* dqkv; float* delta;
  int B, L, D, heads, hd;
  int rs;      // LDS row stride (bytes) of staged rows
  float q_scale;
  const int32_t* row0;
  float drop_scale; uint32_t drop_thr; uint64_t drop_seed;
};

struct FullDoc { int base; int nrows; int len; };   // first activation row, rows that exist, valid keys
__device__ __forceinline__ FullDoc full_doc(const FullArgs& a, int b) {
  const int len = a.lengths ? min(a.lengths[b], a.L) : a.L;
  if (a.row0) return FullDoc{a.row0[b], len, len};
  return FullDoc{b * a.L, a.L, len};
}

// attention-probability dropout: keep decision of (activation row of the query, head, key position in the document)
__device__ __forceinline__ bool full_keep(const FullArgs& a, int grow, int h, int j) {
  return mts_hash32(a.drop_seed, ((uint64_t)grow * a.heads + h) * (uint64_t)a.L + (uint64_t)j) >= a.drop_thr;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <typename T, int MAXU>
__global__ __launch_bounds__(256) void full_fwd_kernel(const FullArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;
  char* KVs = Qs + FT * a.rs;
  float* Ps = reinterpret_cast<float*>(KVs + FT * a.rs);

  const int ntiles = (a.L + FT - 1) / FT;
  int tile, h, b;
  decode_block(ntiles, a.heads, ntiles * a.heads * a.B, tile, h, b);
  const FullDoc doc = full_doc(a, b);
  const int i0 = tile * FT;
  if (i0 >= doc.nrows) return;                       // packed batch: rows past the document do not exist (whole workgroup)
  const int t = threadIdx.x >> 3, g = threadIdx.x & 7;
  const int i = i0 + t;
  const int hd = a.hd, ld = 3 * a.D;
  const T* qbase = reinterpret_cast<const T*>(a.qkv) + (size_t)doc.base * ld + h * hd;

  attn_stage_rows<T>(Qs, a.rs, qbase, ld, i0, FT, doc.nrows, hd);
  float m = -INFINITY, l = 0.f;
  float acc[MAXU][4];
#pragma unroll
  for (int u = 0; u < MAXU; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.f;
  const int nkt = (doc.len + FT - 1) / FT;
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * FT;
    __syncthreads();                                 // previous tile's readers are done with KVs
    attn_stage_rows<T>(KVs, a.rs, qbase + a.D, ld, j0, FT, doc.len, hd);
    __syncthreads();
    float s[4];
    attn_scores<T>(Qs + t * a.rs, KVs + g * a.rs, a.rs, hd, s);
    float mt = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (j0 + g + 8 * c >= doc.len) s[c] = -INFINITY;
      mt = fmaxf(mt, s[c]);
    }
    const float mn = fmaxf(m, lanes8_max(mt));           // finite: key j0 < len is in every visited tile
    const float alpha = __expf(m - mn);              // 0 on the first tile (m = -inf)
    float ps = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float p = __expf(s[c] - mn);
      ps += p;
      const int j = j0 + g + 8 * c;
      Ps[t * PS + g + 8 * c] = a.drop_thr ? (full_keep(a, doc.base + i, h, j) ? p * a.drop_scale : 0.f) : p;
    }
    l = l * alpha + lanes8_sum(ps);
    m = mn;
#pragma unroll
    for (int u = 0; u < MAXU; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[u][e] *= alpha;
    __syncthreads();                                 // K scores done: KVs takes V
    attn_stage_rows<T>(KVs, a.rs, qbase + 2 * a.D, ld, j0, FT, doc.len, hd);
    __syncthreads();
    attn_accum<T, MAXU>(Ps + t * PS, 1, KVs, a.rs, hd, g, min(FT, doc.len - j0), acc);
  }
  if (i < doc.nrows) {
    const float inv = 1.0f / l;
    T* o = reinterpret_cast<T*>(a.ctx) + (size_t)(doc.base + i) * a.D + h * hd;
    const int nch = hd / 4;
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      const int ch = g + 8 * u;
      if (ch < nch) {
        float v[4] = {acc[u][0] * inv, acc[u][1] * inv, acc[u][2] * inv, acc[u][3] * inv};
        store4<T>(o + 4 * ch, v);
      }
    }
    if (g == 0) a.lse[(size_t)(doc.base + i) * a.heads + h] = m + __logf(l);
  }
}

// ------------------------------------------------------------------------------------------------
// backward, kernel 1: delta and dQ per query tile
// ------------------------------------------------------------------------------------------------
template <typename T, int MAXU>
__global__ __launch_bounds__(256) void full_bwd_q_kernel(const FullArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;
  char* dOs = Qs + FT * a.rs;
  char* Ks = dOs + FT * a.rs;
  char* Vs = Ks + FT * a.rs;
  float* Ps = reinterpret_cast<float*>(Vs + FT * a.rs);

  const int ntiles = (a.L + FT - 1) / FT;
  int tile, h, b;
  decode_block(ntiles, a.heads, ntiles * a.heads * a.B, tile, h, b);
  const FullDoc doc = full_doc(a, b);
  const int i0 = tile * FT;
  if (i0 >= doc.nrows) return;
  const int t = threadIdx.x >> 3, g = threadIdx.x & 7;
  const int i = i0 + t;
  const bool qok = i < doc.nrows;
  const int hd = a.hd, ld = 3 * a.D, nch = hd / 4;
  const T* qbase = reinterpret_cast<const T*>(a.qkv) + (size_t)doc.base * ld + h * hd;
  const T* dobase = reinterpret_cast<const T*>(a.dctx) + (size_t)doc.base * a.D + h * hd;
  const T* obase = reinterpret_cast<const T*>(a.ctx) + (size_t)doc.base * a.D + h * hd;

  attn_stage_rows<T>(Qs, a.rs, qbase, ld, i0, FT, doc.nrows, hd);
  attn_stage_rows<T>(dOs, a.rs, dobase, a.D, i0, FT, doc.nrows, hd);
  // delta_i = dCtx_i . ctx_i (= rowsum(P o dP) of the dropped probabilities: ctx is what they produced)
  float delta = 0.f;
  if (qok) {
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      const int ch = g + 8 * u;
      if (ch < nch) {
        float x[4], y[4];
        load4<T>(dobase + (size_t)i * a.D + 4 * ch, x);
        load4<T>(obase + (size_t)i * a.D + 4 * ch, y);
#pragma unroll
        for (int e = 0; e < 4; ++e) delta = fmaf(x[e], y[e], delta);
      }
    }
  }
  delta = lanes8_sum(delta);
  const float lse = qok ? a.lse[(size_t)(doc.base + i) * a.heads + h] : INFINITY;
  if (qok && g == 0) a.delta[(size_t)(doc.base + i) * a.heads + h] = delta;

  float acc[MAXU][4];
#pragma unroll
  for (int u = 0; u < MAXU; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.f;
  const int nkt = (doc.len + FT - 1) / FT;
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * FT;
    __syncthreads();
    attn_stage_rows<T>(Ks, a.rs, qbase + a.D, ld, j0, FT, doc.len, hd);
    attn_stage_rows<T>(Vs, a.rs, qbase + 2 * a.D, ld, j0, FT, doc.len, hd);
    __syncthreads();
    float s[4], dp[4];
    attn_scores<T>(Qs + t * a.rs, Ks + g * a.rs, a.rs, hd, s);
    attn_scores<T>(dOs + t * a.rs, Vs + g * a.rs, a.rs, hd, dp);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + g + 8 * c;
      const float p = (j < doc.len) ? __expf(s[c] - lse) : 0.f;
      float d = dp[c];
      if (a.drop_thr) d = (qok && full_keep(a, doc.base + i, h, j)) ? d * a.drop_scale : 0.f;
      Ps[t * PS + g + 8 * c] = p * (d - delta);
    }
    __syncthreads();
    attn_accum<T, MAXU>(Ps + t * PS, 1, Ks, a.rs, hd, g, min(FT, doc.len - j0), acc);
  }
  if (qok) {
    T* o = reinterpret_cast<T*>(a.dqkv) + (size_t)(doc.base + i) * ld + h * hd;
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      const int ch = g + 8 * u;
      if (ch < nch) {
        float v[4] = {acc[u][0] * a.q_scale, acc[u][1] * a.q_scale, acc[u][2] * a.q_scale, acc[u][3] * a.q_scale};
        store4<T>(o + 4 * ch, v);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward, kernel 2: dK and dV per key tile (reads the delta kernel 1 saved)
// ------------------------------------------------------------------------------------------------
template <typename T, int MAXU>
__global__ __launch_bounds__(256) void full_bwd_kv_kernel(const FullArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = Ks + FT * a.rs;
  char* Qs = Vs + FT * a.rs;
  char* dOs = Qs + FT * a.rs;
  float* PT = reinterpret_cast<float*>(dOs + FT * a.rs);   // [key][query] dropped probabilities
  float* ST = PT + FT * PS;                                 // [key][query] dS
  float* lse_s = ST + FT * PS;
  float* del_s = lse_s + FT;

  const int ntiles = (a.L + FT - 1) / FT;
  int tile, h, b;
  decode_block(ntiles, a.heads, ntiles * a.heads * a.B, tile, h, b);
  const FullDoc doc = full_doc(a, b);
  const int j0 = tile * FT;
  if (j0 >= doc.nrows) return;
  const int t = threadIdx.x >> 3, g = threadIdx.x & 7;
  const int j = j0 + t;
  const int hd = a.hd, ld = 3 * a.D, nch = hd / 4;
  const T* qbase = reinterpret_cast<const T*>(a.qkv) + (size_t)doc.base * ld + h * hd;
  const T* dobase = reinterpret_cast<const T*>(a.dctx) + (size_t)doc.base * a.D + h * hd;

  float dk[MAXU][4], dv[MAXU][4];
#pragma unroll
  for (int u = 0; u < MAXU; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) dk[u][e] = dv[u][e] = 0.f;

  if (j0 < doc.len) {                                 // padded keys (padded layout only): probability 0, gradient 0
    attn_stage_rows<T>(Ks, a.rs, qbase + a.D, ld, j0, FT, doc.len, hd);
    attn_stage_rows<T>(Vs, a.rs, qbase + 2 * a.D, ld, j0, FT, doc.len, hd);
    const int nqt = (doc.nrows + FT - 1) / FT;
    for (int qt = 0; qt < nqt; ++qt) {
      const int i0 = qt * FT;
      __syncthreads();
      attn_stage_rows<T>(Qs, a.rs, qbase, ld, i0, FT, doc.nrows, hd);
      attn_stage_rows<T>(dOs, a.rs, dobase, a.D, i0, FT, doc.nrows, hd);
      if (threadIdx.x < FT) {
        const int i = i0 + threadIdx.x;
        const bool ok = i < doc.nrows;
        lse_s[threadIdx.x] = ok ? a.lse[(size_t)(doc.base + i) * a.heads + h] : INFINITY;   // rows past the document: P = 0
        del_s[threadIdx.x] = ok ? a.delta[(size_t)(doc.base + i) * a.heads + h] : 0.f;
      }
      __syncthreads();
      float s[4], dp[4];
      attn_scores<T>(Ks + t * a.rs, Qs + g * a.rs, a.rs, hd, s);
      attn_scores<T>(Vs + t * a.rs, dOs + g * a.rs, a.rs, hd, dp);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ci = g + 8 * c, i = i0 + ci;
        const float p = (j < doc.len) ? __expf(s[c] - lse_s[ci]) : 0.f;
        float keep = 1.f;
        if (a.drop_thr) keep = (i < doc.nrows && full_keep(a, doc.base + i, h, j)) ? a.drop_scale : 0.f;
        PT[t * PS + ci] = p * keep;
        ST[t * PS + ci] = p * (dp[c] * keep - del_s[ci]);
      }
      __syncthreads();
      const int ncq = min(FT, doc.nrows - i0);
      attn_accum<T, MAXU>(PT + t * PS, 1, dOs, a.rs, hd, g, ncq, dv);
      attn_accum<T, MAXU>(ST + t * PS, 1, Qs, a.rs, hd, g, ncq, dk);
    }
  }
  if (j < doc.nrows) {
    T* o = reinterpret_cast<T*>(a.dqkv) + (size_t)(doc.base + j) * ld + h * hd;
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      const int ch = g + 8 * u;
      if (ch < nch) { store4<T>(o + a.D + 4 * ch, dk[u]); store4<T>(o + 2 * a.D + 4 * ch, dv[u]); }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// bf16 matrix-core path (head dim a multiple of 32, <= 256): v_mfma_f32_16x16x32_bf16, 4 waves x 16 rows per workgroup.
//
// Every product is X . Y^T in the fragment layout of attn_tile.h.  Products that sum over keys (P V, dS K) or over queries
// (P^T dO, dS^T Q) read transposed images ([dim][key] / [dim][query]) written while staging, and P / dS cross LDS once per wave
// to become A fragments.  Same tiles and loop orders on every run, no atomics: bitwise reproducible.
//
//   forward : workgroup = 64 queries; per 32-key tile S = Q K^T, online softmax on the C fragments (the rows of S are the rows of
//             the ctx accumulators), P (bf16) -> LDS, ctx += P Vt^T.
//   dq      : workgroup = 64 queries; per 32-key tile S = Q K^T, dP = dO V^T, dS = P (dP - delta) (bf16) -> LDS, dQ += dS Kt^T.
//   dk / dv : workgroup = 64 keys; per 32-query tile S^T = K Q^T, dP^T = V dO^T, dV += P^T dOt^T, dK += dS^T Qt^T.
// ------------------------------------------------------------------------------------------------
template <int KK>
__global__ __launch_bounds__(256) void full_mfma_fwd_kernel(const FullArgs a) {
  constexpr int NT = 2 * KK;          // 16-wide dim tiles of the head dim
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;
  char* Ks = Qs + MQ * a.rs;
  char* Vt = Ks + MK * a.rs;
  char* Pw = Vt + 32 * KK * TRS;
  const int ntiles = (a.L + MQ - 1) / MQ;
  int tile, h, b;
  decode_block(ntiles, a.heads, ntiles * a.heads * a.B, tile, h, b);
  const FullDoc doc = full_doc(a, b);
  const int q0 = tile * MQ;
  if (q0 >= doc.nrows) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int hd = a.hd, ld = 3 * a.D;
  const bf16_t* qbase = reinterpret_cast<const bf16_t*>(a.qkv) + (size_t)doc.base * ld + h * hd;
  char* W = Pw + w * 16 * TRS;
  attn_mstage(Qs, a.rs, nullptr, qbase, ld, q0, MQ, doc.nrows, hd);
  float m[4], l[4];
  f32x4 acc[NT];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nkt = (doc.len + MK - 1) / MK;
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * MK;
    __syncthreads();
    attn_mstage(Ks, a.rs, nullptr, qbase + a.D, ld, j0, MK, doc.len, hd);
    attn_mstage(nullptr, 0, Vt, qbase + 2 * a.D, ld, j0, MK, doc.len, hd);   // V only as its transpose [dim][key]
    __syncthreads();
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    attn_mm_xyt<2>(Qs, a.rs, 16 * w, Ks, a.rs, KK, lane, s);
    float p[2][4], alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mt = -INFINITY;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        if (j0 + 16 * ct + l15 >= doc.len) s[ct][r] = -INFINITY;
        mt = fmaxf(mt, s[ct][r]);
      }
      const float mn = fmaxf(m[r], lanes16_max(mt));       // finite: key j0 < len is in every visited tile
      alpha[r] = __expf(m[r] - mn);
      float ps = 0.f;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const float e = __expf(s[ct][r] - mn);
        ps += e;
        const int i = q0 + 16 * w + 4 * g + r, j = j0 + 16 * ct + l15;
        p[ct][r] = a.drop_thr ? (full_keep(a, doc.base + i, h, j) ? e * a.drop_scale : 0.f) : e;
      }
      l[r] = l[r] * alpha[r] + lanes16_sum(ps);
      m[r] = mn;
    }
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[n][r] *= alpha[r];
    attn_put_coef(W, lane, p);
    __syncthreads();
    attn_mm_xyt<NT>(W, TRS, 0, Vt, TRS, 1, lane, acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + 16 * w + 4 * g + r;
    if (i < doc.nrows) {
      const float inv = 1.0f / l[r];
      bf16_t* o = reinterpret_cast<bf16_t*>(a.ctx) + (size_t)(doc.base + i) * a.D + h * hd;
#pragma unroll
      for (int n = 0; n < NT; ++n) o[16 * n + l15] = (bf16_t)(acc[n][r] * inv);
      if (l15 == 0) a.lse[(size_t)(doc.base + i) * a.heads + h] = m[r] + __logf(l[r]);
    }
  }
}

template <int KK>
__global__ __launch_bounds__(256) void full_mfma_bwd_q_kernel(const FullArgs a) {
  constexpr int NT = 2 * KK;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;
  char* dOs = Qs + MQ * a.rs;
  char* Ks = dOs + MQ * a.rs;
  char* Vs = Ks + MK * a.rs;
  char* Kt = Vs + MK * a.rs;
  char* Pw = Kt + 32 * KK * TRS;
  float* row_s = reinterpret_cast<float*>(Pw + 4 * 16 * TRS);    // [64] lse, [64] delta
  const int ntiles = (a.L + MQ - 1) / MQ;
  int tile, h, b;
  decode_block(ntiles, a.heads, ntiles * a.heads * a.B, tile, h, b);
  const FullDoc doc = full_doc(a, b);
  const int q0 = tile * MQ;
  if (q0 >= doc.nrows) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int hd = a.hd, ld = 3 * a.D;
  const bf16_t* qbase = reinterpret_cast<const bf16_t*>(a.qkv) + (size_t)doc.base * ld + h * hd;
  const bf16_t* dobase = reinterpret_cast<const bf16_t*>(a.dctx) + (size_t)doc.base * a.D + h * hd;
  const bf16_t* obase = reinterpret_cast<const bf16_t*>(a.ctx) + (size_t)doc.base * a.D + h * hd;
  char* W = Pw + w * 16 * TRS;
  attn_mstage(Qs, a.rs, nullptr, qbase, ld, q0, MQ, doc.nrows, hd);
  attn_mstage(dOs, a.rs, nullptr, dobase, a.D, q0, MQ, doc.nrows, hd);
  if (threadIdx.x < MQ) {                               // delta = dCtx . ctx (fixed order), lse; rows past the document: P = 0
    const int i = q0 + threadIdx.x;
    float d = 0.f, lv = INFINITY;
    if (i < doc.nrows) {
      for (int c = 0; c < hd; c += 4) {
        float x[4], y[4];
        load4<bf16_t>(dobase + (size_t)i * a.D + c, x);
        load4<bf16_t>(obase + (size_t)i * a.D + c, y);
#pragma unroll
        for (int e = 0; e < 4; ++e) d = fmaf(x[e], y[e], d);
      }
      lv = a.lse[(size_t)(doc.base + i) * a.heads + h];
      a.delta[(size_t)(doc.base + i) * a.heads + h] = d;
    }
    row_s[threadIdx.x] = lv;
    row_s[MQ + threadIdx.x] = d;
  }
  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nkt = (doc.len + MK - 1) / MK;
  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * MK;
    __syncthreads();
    attn_mstage(Ks, a.rs, Kt, qbase + a.D, ld, j0, MK, doc.len, hd);
    attn_mstage(Vs, a.rs, nullptr, qbase + 2 * a.D, ld, j0, MK, doc.len, hd);
    __syncthreads();
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 dp[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    attn_mm_xyt<2>(Qs, a.rs, 16 * w, Ks, a.rs, KK, lane, s);
    attn_mm_xyt<2>(dOs, a.rs, 16 * w, Vs, a.rs, KK, lane, dp);
    float ds[2][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ri = 16 * w + 4 * g + r, i = q0 + ri;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int j = j0 + 16 * ct + l15;
        const float p = (j < doc.len) ? __expf(s[ct][r] - row_s[ri]) : 0.f;
        float d = dp[ct][r];
        if (a.drop_thr) d = (i < doc.nrows && full_keep(a, doc.base + i, h, j)) ? d * a.drop_scale : 0.f;
        ds[ct][r] = p * (d - row_s[MQ + ri]);
      }
    }
    attn_put_coef(W, lane, ds);
    __syncthreads();
    attn_mm_xyt<NT>(W, TRS, 0, Kt, TRS, 1, lane, acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + 16 * w + 4 * g + r;
    if (i < doc.nrows) {
      bf16_t* o = reinterpret_cast<bf16_t*>(a.dqkv) + (size_t)(doc.base + i) * ld + h * hd;
#pragma unroll
      for (int n = 0; n < NT; ++n) o[16 * n + l15] = (bf16_t)(acc[n][r] * a.q_scale);
    }
  }
}

template <int KK>
__global__ __launch_bounds__(256) void full_mfma_bwd_kv_kernel(const FullArgs a) {
  constexpr int NT = 2 * KK;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = Ks + MQ * a.rs;
  char* Qs = Vs + MQ * a.rs;
  char* dOs = Qs + MK * a.rs;
  char* Qt = dOs + MK * a.rs;
  char* dOt = Qt + 32 * KK * TRS;
  char* Pw = dOt + 32 * KK * TRS;               // [wave][16 keys][32 queries] P^T (dropped)
  char* Sw = Pw + 4 * 16 * TRS;                 // ... dS^T
  float* lse_s = reinterpret_cast<float*>(Sw + 4 * 16 * TRS);
  float* del_s = lse_s + MK;
  const int ntiles = (a.L + MQ - 1) / MQ;
  int tile, h, b;
  decode_block(ntiles, a.heads, ntiles * a.heads * a.B, tile, h, b);
  const FullDoc doc = full_doc(a, b);
  const int k0 = tile * MQ;
  if (k0 >= doc.nrows) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int hd = a.hd, ld = 3 * a.D;
  const bf16_t* qbase = reinterpret_cast<const bf16_t*>(a.qkv) + (size_t)doc.base * ld + h * hd;
  const bf16_t* dobase = reinterpret_cast<const bf16_t*>(a.dctx) + (size_t)doc.base * a.D + h * hd;
  f32x4 dk[NT], dv[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) dk[n] = dv[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (k0 < doc.len) {                           // padded keys (padded layout only): gradient 0
    attn_mstage(Ks, a.rs, nullptr, qbase + a.D, ld, k0, MQ, doc.len, hd);
    attn_mstage(Vs, a.rs, nullptr, qbase + 2 * a.D, ld, k0, MQ, doc.len, hd);
    char* PW = Pw + w * 16 * TRS;
    char* SW = Sw + w * 16 * TRS;
    const int nqt = (doc.nrows + MK - 1) / MK;
    for (int qt = 0; qt < nqt; ++qt) {
      const int i0 = qt * MK;
      __syncthreads();
      attn_mstage(Qs, a.rs, Qt, qbase, ld, i0, MK, doc.nrows, hd);
      attn_mstage(dOs, a.rs, dOt, dobase, a.D, i0, MK, doc.nrows, hd);
      if (threadIdx.x < MK) {
        const int i = i0 + threadIdx.x;
        const bool ok = i < doc.nrows;
        lse_s[threadIdx.x] = ok ? a.lse[(size_t)(doc.base + i) * a.heads + h] : INFINITY;
        del_s[threadIdx.x] = ok ? a.delta[(size_t)(doc.base + i) * a.heads + h] : 0.f;
      }
      __syncthreads();
      f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      f32x4 dp[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      attn_mm_xyt<2>(Ks, a.rs, 16 * w, Qs, a.rs, KK, lane, s);      // S^T: rows = keys, columns = queries
      attn_mm_xyt<2>(Vs, a.rs, 16 * w, dOs, a.rs, KK, lane, dp);    // dP^T
      float pt[2][4], st[2][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = k0 + 16 * w + 4 * g + r;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int ci = 16 * ct + l15, i = i0 + ci;
          const float p = (j < doc.len) ? __expf(s[ct][r] - lse_s[ci]) : 0.f;
          float keep = 1.f;
          if (a.drop_thr) keep = (i < doc.nrows && full_keep(a, doc.base + i, h, j)) ? a.drop_scale : 0.f;
          pt[ct][r] = p * keep;
          st[ct][r] = p * (dp[ct][r] * keep - del_s[ci]);
        }
      }
      attn_put_coef(PW, lane, pt);
      attn_put_coef(SW, lane, st);
      __syncthreads();
      attn_mm_xyt<NT>(PW, TRS, 0, dOt, TRS, 1, lane, dv);
      attn_mm_xyt<NT>(SW, TRS, 0, Qt, TRS, 1, lane, dk);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = k0 + 16 * w + 4 * g + r;
    if (j < doc.nrows) {
      bf16_t* o = reinterpret_cast<bf16_t*>(a.dqkv) + (size_t)(doc.base + j) * ld + h * hd;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        o[a.D + 16 * n + l15] = (bf16_t)dk[n][r];
        o[2 * a.D + 16 * n + l15] = (bf16_t)dv[n][r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static size_t full_generic_lds(int rs);

static int full_fill(FullArgs& a, int dtype, int B, int L, int D, int heads, const char* who) {
  MTS_CHECK_ARG(B > 0 && L > 0 && D > 0 && heads > 0, "%s: bad shape", who);
  MTS_CHECK_ARG(D % heads == 0, "%s: D=%d not divisible by heads=%d", who, D, heads);
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "%s: bad dtype %d", who, dtype);
  const int hd = D / heads;
  const int vec = dtype == MTS_F32 ? 4 : 8;
  MTS_UNSUPPORTED(hd % vec == 0 && hd <= 512, "%s: head dim %d must be a multiple of %d and <= 512", who, hd, vec);
  MTS_UNSUPPORTED((long)B * L * heads < (1L << 31) && (long)B * L * 3 * D < (1L << 31), "%s: problem too large for 32-bit row indexing", who);
  memset(&a, 0, sizeof(a));
  a.B = B; a.L = L; a.D = D; a.heads = heads; a.hd = hd;
  a.rs = attn_row_stride(hd, dtype == MTS_F32 ? 4 : 2);
  MTS_UNSUPPORTED(full_generic_lds(a.rs) <= 160 * 1024, "%s: head dim %d in %s needs %zu bytes of LDS (> 160 KiB)", who, hd,
                  dtype == MTS_F32 ? "fp32" : "bf16", full_generic_lds(a.rs));
  a.q_scale = 1.f;
  a.drop_scale = 1.f;
  return MTS_OK;
}

// LDS of the generic kernels (the backward's two are the largest) and of the matrix-core kernels
static size_t full_generic_lds(int rs) { return (size_t)4 * FT * rs + (size_t)(2 * FT * PS + 2 * FT) * sizeof(float); }
static size_t full_mfma_lds(int which, int rs, int hd) {
  const size_t t = (size_t)hd * TRS, w = (size_t)4 * 16 * TRS;
  if (which == 0) return (size_t)(MQ + MK) * rs + t + w;
  if (which == 1) return (size_t)2 * (MQ + MK) * rs + t + w + 2 * MQ * sizeof(float);
  return (size_t)2 * (MQ + MK) * rs + 2 * t + 2 * w + 2 * MK * sizeof(float);
}

static thread_local int g_full_mfma = 1;     // mts_set_option("full_mfma", 0) sends bf16 to the generic kernels (A/B testing)
void mts_full_set_mfma(int on) { g_full_mfma = on; }
static bool full_use_mfma(const FullArgs& a, int dtype) { return dtype == MTS_BF16 && g_full_mfma && a.hd % 32 == 0 && a.hd <= 256; }

#define FULL_KK_SWITCH(KK_, CALL)                                                        \
  switch (KK_) {                                                                         \
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break;              \
    case 4: CALL(4); break; case 5: CALL(5); break; case 6: CALL(6); break;              \
    case 7: CALL(7); break; default: CALL(8); break;                                     \
  }

static int full_mfma_fwd_launch(const FullArgs& a, hipStream_t st) {
  const size_t lds = full_mfma_lds(0, a.rs, a.hd);
  const int nblocks = ceil_div(a.L, MQ) * a.heads * a.B;
  int rc = MTS_OK;
#define FWD_CALL(K)                                                                                   \
  rc = mts_dyn_lds(full_mfma_fwd_kernel<K>, lds, "mts_full_attn_fwd");                                  \
  if (!rc) hipLaunchKernelGGL(full_mfma_fwd_kernel<K>, dim3(nblocks), dim3(256), lds, st, a);
  FULL_KK_SWITCH(a.hd / 32, FWD_CALL)
#undef FWD_CALL
  if (rc) return rc;
  MTS_LAUNCH_CHECK("mts_full_attn_fwd");
  return MTS_OK;
}

static int full_mfma_bwd_launch(const FullArgs& a, hipStream_t st) {
  const size_t lq = full_mfma_lds(1, a.rs, a.hd), lkv = full_mfma_lds(2, a.rs, a.hd);
  const int nblocks = ceil_div(a.L, MQ) * a.heads * a.B;
  int rc = MTS_OK;
#define BWD_CALL(K)                                                                                   \
  rc = mts_dyn_lds(full_mfma_bwd_q_kernel<K>, lq, "mts_full_attn_bwd(q)");                              \
  if (!rc) rc = mts_dyn_lds(full_mfma_bwd_kv_kernel<K>, lkv, "mts_full_attn_bwd(kv)");                  \
  if (!rc) {                                                                                          \
    hipLaunchKernelGGL(full_mfma_bwd_q_kernel<K>, dim3(nblocks), dim3(256), lq, st, a);              \
    hipLaunchKernelGGL(full_mfma_bwd_kv_kernel<K>, dim3(nblocks), dim3(256), lkv, st, a);            \
  }
  FULL_KK_SWITCH(a.hd / 32, BWD_CALL)
#undef BWD_CALL
  if (rc) return rc;
  MTS_LAUNCH_CHECK("mts_full_attn_bwd");
  return MTS_OK;
}

template <typename T>
static int full_fwd_launch(const FullArgs& a, hipStream_t st) {
  const size_t lds = (size_t)2 * FT * a.rs + (size_t)FT * PS * sizeof(float);
  const int nblocks = ceil_div(a.L, FT) * a.heads * a.B;
  auto k = a.hd > 256 ? full_fwd_kernel<T, 16> : full_fwd_kernel<T, 8>;     // 8 lanes x MAXU chunks of 4 cover the head dim
  int rc = mts_dyn_lds(k, lds, "mts_full_attn_fwd");
  if (rc) return rc;
  hipLaunchKernelGGL(k, dim3(nblocks), dim3(256), lds, st, a);
  MTS_LAUNCH_CHECK("mts_full_attn_fwd");
  return MTS_OK;
}

template <typename T>
static int full_bwd_launch(const FullArgs& a, hipStream_t st) {
  const int nblocks = ceil_div(a.L, FT) * a.heads * a.B;
  const size_t lds_q = (size_t)4 * FT * a.rs + (size_t)FT * PS * sizeof(float);
  const size_t lds_kv = (size_t)4 * FT * a.rs + (size_t)(2 * FT * PS + 2 * FT) * sizeof(float);
  auto kq = a.hd > 256 ? full_bwd_q_kernel<T, 16> : full_bwd_q_kernel<T, 8>;
  auto kkv = a.hd > 256 ? full_bwd_kv_kernel<T, 16> : full_bwd_kv_kernel<T, 8>;
  int rc = mts_dyn_lds(kq, lds_q, "mts_full_attn_bwd(q)");
  if (!rc) rc = mts_dyn_lds(kkv, lds_kv, "mts_full_attn_bwd(kv)");
  if (rc) return rc;
  hipLaunchKernelGGL(kq, dim3(nblocks), dim3(256), lds_q, st, a);
  hipLaunchKernelGGL(kkv, dim3(nblocks), dim3(256), lds_kv, st, a);
  MTS_LAUNCH_CHECK("mts_full_attn_bwd");
  return MTS_OK;
}

extern "C" int mts_full_attn_fwd(void* stream, int dtype, int B, int L, int D, int heads, const void* qkv, const int32_t* lengths,
                                 void* ctx, float* lse, const int32_t* row0, float drop_p, uint64_t drop_seed) {
  FullArgs a;
  int rc = full_fill(a, dtype, B, L, D, heads, "mts_full_attn_fwd");
  if (rc) return rc;
  MTS_CHECK_ARG(qkv && ctx && lse, "mts_full_attn_fwd: null pointer");
  MTS_CHECK_ARG(!row0 || lengths, "mts_full_attn_fwd: packed rows (row0) need lengths");
  rc = attn_set_dropout(a, drop_p, drop_seed, "mts_full_attn_fwd");
  if (rc) return rc;
  a.qkv = qkv; a.lengths = lengths; a.ctx = ctx; a.lse = lse; a.row0 = row0;
  if (full_use_mfma(a, dtype)) return full_mfma_fwd_launch(a, (hipStream_t)stream);
  return dtype == MTS_F32 ? full_fwd_launch<float>(a, (hipStream_t)stream) : full_fwd_launch<bf16_t>(a, (hipStream_t)stream);
}

extern "C" size_t mts_full_attn_bwd_workspace(int B, int L, int D, int heads) {
  const size_t delta = align_up((size_t)B * L * (size_t)std::max(heads, 1) * sizeof(float), 256);
  return std::max(delta, mts_colsum_workspace(3 * D));    // delta is dead by the time the bias column sums run
}

extern "C" int mts_full_attn_bwd(void* stream, int dtype, int B, int L, int D, int heads, float q_scale, const void* qkv,
                                 const int32_t* lengths, const float* lse, const void* ctx, const void* dctx, void* dqkv, float* dbias,
                                 void* workspace, const int32_t* row0, int n_rows, float drop_p, uint64_t drop_seed) {
  FullArgs a;
  int rc = full_fill(a, dtype, B, L, D, heads, "mts_full_attn_bwd");
  if (rc) return rc;
  MTS_CHECK_ARG(qkv && lse && ctx && dctx && dqkv && workspace, "mts_full_attn_bwd: null pointer (workspace is required)");
  MTS_CHECK_ARG(!row0 || (lengths && n_rows > 0 && n_rows <= B * L), "mts_full_attn_bwd: packed rows (row0) need lengths and 0 < n_rows <= B*L");
  rc = attn_set_dropout(a, drop_p, drop_seed, "mts_full_attn_bwd");
  if (rc) return rc;
  a.qkv = qkv; a.lengths = lengths; a.lse = const_cast<float*>(lse); a.ctx = const_cast<void*>(ctx); a.dctx = dctx; a.dqkv = dqkv;
  a.delta = (float*)workspace; a.row0 = row0; a.q_scale = q_scale;
  if (full_use_mfma(a, dtype)) rc = full_mfma_bwd_launch(a, (hipStream_t)stream);
  else rc = dtype == MTS_F32 ? full_bwd_launch<float>(a, (hipStream_t)stream) : full_bwd_launch<bf16_t>(a, (hipStream_t)stream);
  if (rc == MTS_OK && dbias) rc = mts_colsum(stream, dtype, row0 ? n_rows : B * L, 3 * D, dqkv, 3 * D, dbias, 0, workspace);
  return rc;
}
