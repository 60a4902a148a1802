// The two pieces of a BERT-family sentence encoder that are not a GEMM, a LayerNorm or document-sized attention (include/mts.h "Text
// sentence features"): the embedding stage and self-attention over packed SHORT sequences.
//
//   text_embed : one 64-lane wave per token row, ROW_WAVES rows per workgroup, as the LayerNorm kernels of norm.hip.  Lane l owns the
//                16-byte chunks l, l + 64, .. of the row (4 fp32 / 8 bf16 elements each): the three table rows are read once with
//                16-byte accesses and summed in fp32, the statistics are wave reductions over registers (mean, then the variance about
//                it), and every element is stored once.  No LDS, no atomics.
//   sent_attn  : one wave per (sentence, head), four pairs per workgroup, v_mfma_f32_16x16x32_bf16 in the fragment layout of
//                attn_tile.h.  Both operands of S = Q K^T run along the head dim, so the rows of q and k are read straight from global
//                memory into fragments: K once per wave, Q once per 16-query tile.  All keys of the sentence are present, so the softmax
//                on the C fragments is exact over the whole row (no online rescaling).  P (bf16) and the transposed V cross LDS once, in
//                images private to the wave: the waves of a workgroup never wait for each other.
#include <algorithm>
#include "common.h"
#include "attn_tile.h"

#define ROW_WAVES 4            // token rows (text_embed) / (sentence, head) pairs (sent_attn) per workgroup

// ------------------------------------------------------------------------------------------------
// embedding stage
// ------------------------------------------------------------------------------------------------
template <typename T> struct Chunk16;        // 16 bytes of T as fp32 values
template <> struct Chunk16<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float (&o)[4]) { load4<float>(p, o); }
  static __device__ __forceinline__ void store(float* p, const float (&o)[4]) { store4<float>(p, o); }
};
template <> struct Chunk16<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float (&o)[8]) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    o[0] = bf16_lo(v.x); o[1] = bf16_hi(v.x); o[2] = bf16_lo(v.y); o[3] = bf16_hi(v.y);
    o[4] = bf16_lo(v.z); o[5] = bf16_hi(v.z); o[6] = bf16_lo(v.w); o[7] = bf16_hi(v.w);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&o)[8]) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
  }
};

// NV: 16-byte chunks per lane (H <= 64 NV N); FULL (H == 64 NV N): no bounds checks around the loads (norm.hip: ln_fwd_kernel)
template <typename T, int NV, bool FULL>
__global__ __launch_bounds__(64 * ROW_WAVES) void text_embed_kernel(int n_tokens, int H, const int32_t* __restrict__ ids, const int32_t* __restrict__ pos,
                                                                    const T* __restrict__ word, const T* __restrict__ position,
                                                                    const T* __restrict__ type_row, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float eps, T* __restrict__ out, int ldo) {
  constexpr int N = Chunk16<T>::N;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
  if (row >= n_tokens) return;
  const T* wr = word + (size_t)ids[row] * H;
  const T* pr = position + (size_t)pos[row] * H;
  float x[NV][N], gv[NV][N / 4][4], bv[NV][N / 4][4];
  // every load is issued before the first reduction and the first store (norm.hip: the vector-memory counter retires in order)
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int e = N * (lane + 64 * i);
    if (FULL || e < H) {
      float a[N], b[N], c[N];
      Chunk16<T>::load(wr + e, a); Chunk16<T>::load(pr + e, b); Chunk16<T>::load(type_row + e, c);
#pragma unroll
      for (int j = 0; j < N; ++j) x[i][j] = (a[j] + b[j]) + c[j];
#pragma unroll
      for (int j = 0; j < N; j += 4) {
        load4<float>(gamma + e + j, gv[i][j / 4]);
        load4<float>(beta + e + j, bv[i][j / 4]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) x[i][j] = 0.f;
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < N; j += 4) s += (x[i][j] + x[i][j + 1]) + (x[i][j + 2] + x[i][j + 3]);
  const float mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (FULL || N * (lane + 64 * i) < H) {
#pragma unroll
      for (int j = 0; j < N; ++j) { const float d = x[i][j] - mean; q += d * d; }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
  T* o = out + (size_t)row * ldo;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int e = N * (lane + 64 * i);
    if (FULL || e < H) {
#pragma unroll
      for (int j = 0; j < N; ++j) x[i][j] = (x[i][j] - mean) * rstd * gv[i][j / 4][j % 4] + bv[i][j / 4][j % 4];
      Chunk16<T>::store(o + e, x[i]);
    }
  }
}

template <typename T>
static int text_embed_launch(hipStream_t st, int n_tokens, int H, const int32_t* ids, const int32_t* pos, const void* word, const void* position,
                             const void* type_row, const float* gamma, const float* beta, float eps, void* out, int ldo) {
  constexpr int N = Chunk16<T>::N;
  const int need = ceil_div(H, 64 * N);
  const dim3 grid(ceil_div(n_tokens, ROW_WAVES)), block(64 * ROW_WAVES);
#define EMBED_CALL(NV_)                                                                                                                 \
  do {                                                                                                                                  \
    if (H == 64 * N * NV_)                                                                                                              \
      hipLaunchKernelGGL((text_embed_kernel<T, NV_, true>), grid, block, 0, st, n_tokens, H, ids, pos, (const T*)word, (const T*)position, \
                         (const T*)type_row, gamma, beta, eps, (T*)out, ldo);                                                           \
    else                                                                                                                                \
      hipLaunchKernelGGL((text_embed_kernel<T, NV_, false>), grid, block, 0, st, n_tokens, H, ids, pos, (const T*)word, (const T*)position, \
                         (const T*)type_row, gamma, beta, eps, (T*)out, ldo);                                                           \
  } while (0)
  if (need <= 1) EMBED_CALL(1);
  else if (need <= 2) EMBED_CALL(2);
  else if (need == 3) EMBED_CALL(3);           // H = 768 in fp32: no idle chunk
  else if (need <= 4) EMBED_CALL(4);
  else EMBED_CALL(8);
#undef EMBED_CALL
  MTS_LAUNCH_CHECK("mts_text_embed");
  return MTS_OK;
}

extern "C" int mts_text_embed(void* stream, int dtype, int n_tokens, int H, const int32_t* ids, const int32_t* pos, const void* word, int vocab,
                              const void* position, int n_pos, const void* type_row, const float* gamma, const float* beta, float eps, void* out,
                              int ldo) {
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "mts_text_embed: bad dtype %d", dtype);
  MTS_CHECK_ARG(n_tokens > 0 && H > 0 && vocab > 0 && n_pos > 0, "mts_text_embed: bad shape (n_tokens=%d, H=%d, vocab=%d, n_pos=%d)", n_tokens, H,
                vocab, n_pos);
  MTS_CHECK_ARG(ids && pos && word && position && type_row && gamma && beta && out, "mts_text_embed: null pointer");
  MTS_CHECK_ARG(eps >= 0.f, "mts_text_embed: eps has to be non-negative, but got %f", (double)eps);
  const int vec = dtype == MTS_F32 ? 4 : 8;
  MTS_UNSUPPORTED(H % vec == 0 && H <= 512 * vec, "mts_text_embed: H=%d must be a multiple of %d and <= %d in %s", H, vec, 512 * vec,
                  dtype == MTS_F32 ? "fp32" : "bf16");
  MTS_CHECK_ARG(ldo >= H && ldo % vec == 0, "mts_text_embed: ldo=%d must be >= H and a multiple of %d", ldo, vec);
  MTS_CHECK_ARG(aligned_to(word, 16) && aligned_to(position, 16) && aligned_to(type_row, 16) && aligned_to(gamma, 16) && aligned_to(beta, 16) &&
                    aligned_to(out, 16),
                "mts_text_embed: the tables, gamma, beta and out must be 16-byte aligned");
  if (dtype == MTS_F32)
    return text_embed_launch<float>((hipStream_t)stream, n_tokens, H, ids, pos, word, position, type_row, gamma, beta, eps, out, ldo);
  return text_embed_launch<bf16_t>((hipStream_t)stream, n_tokens, H, ids, pos, word, position, type_row, gamma, beta, eps, out, ldo);
}

// ------------------------------------------------------------------------------------------------
// self-attention over packed short sequences (bf16)
// ------------------------------------------------------------------------------------------------
struct SentArgs {
  const bf16_t* qkv;
  bf16_t* ctx;
  const int32_t* row0;
  const int32_t* lengths;
  int n_pairs, D, heads, hd, rs;
};

// KK: 32-wide k-steps of the head dim; KS: 32-key steps the kernel covers (sentences up to 32 KS tokens).  LDS per wave: the transposed
// V image Vt[hd][32 KS] and the coefficient image W[16][32 KS], both with row stride rs = 64 KS + 16 bytes (16 B x odd)
template <int KK, int KS>
__global__ __launch_bounds__(64 * ROW_WAVES) void sent_attn_kernel(const SentArgs a) {
  constexpr int NT = 2 * KK;          // 16-wide tiles of the head dim
  constexpr int NCT = 2 * KS;         // 16-key tiles
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int pair = blockIdx.x * ROW_WAVES + w;
  if (pair >= a.n_pairs) return;                      // no workgroup barrier below: a wave may leave alone
  const int s = pair / a.heads, h = pair % a.heads;
  const int len = min(a.lengths[s], 32 * KS);         // the caller's contract is 1 <= len <= max_len; nothing past the cover is touched
  const int hd = a.hd, ld = 3 * a.D;
  const size_t base = (size_t)a.row0[s];
  const bf16_t* qbase = a.qkv + base * ld + h * hd;
  char* Vt = smem + (size_t)w * (hd + 16) * a.rs;
  char* W = Vt + (size_t)hd * a.rs;
  const int nks = (len + 31) / 32;                    // 32-key steps of this sentence
  // K: every row once, as the B fragments of S = Q K^T; key tiles past the sentence stay 0 and are masked below
  bf16x8 kf[NCT][KK];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int k = 0; k < KK; ++k) kf[ct][k] = attn_gfrag(qbase + a.D, ld, 16 * ct + l15, len, k, lane);
  attn_wave_tstage(Vt, a.rs, qbase + 2 * a.D, ld, 32 * nks, len, hd, lane);
  const int nmt = (len + 15) / 16;
  for (int mt = 0; mt < nmt; ++mt) {
    bf16x8 qf[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) qf[k] = attn_gfrag(qbase, ld, 16 * mt + l15, len, k, lane);
    f32x4 sc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      sc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (16 * ct < len) {
#pragma unroll
        for (int k = 0; k < KK; ++k) sc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[k], kf[ct][k], sc[ct], 0, 0, 0);
      }
    }
    float p[NCT][4], inv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -INFINITY;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        if (16 * ct + l15 >= len) sc[ct][r] = -INFINITY;
        mx = fmaxf(mx, sc[ct][r]);
      }
      mx = lanes16_max(mx);                            // finite: key 0 is in every sentence
      float ps = 0.f;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) { p[ct][r] = __expf(sc[ct][r] - mx); ps += p[ct][r]; }
      inv[r] = 1.0f / lanes16_sum(ps);
    }
    attn_put_coef_n<NCT>(W, a.rs, lane, p);
    attn_wave_sync();                                  // W (and, the first time, Vt) written by the wave's other lanes
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    attn_mm_xyt<NT>(W, a.rs, 0, Vt, a.rs, nks, lane, acc);
    attn_wave_sync();                                  // W is rewritten by the next query tile
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * mt + 4 * g + r;
      if (i < len) {
        bf16_t* o = a.ctx + (base + i) * a.D + h * hd;
#pragma unroll
        for (int n = 0; n < NT; ++n) o[16 * n + l15] = (bf16_t)(acc[n][r] * inv[r]);
      }
    }
  }
}

#define SENT_MAX_LEN 64

extern "C" int mts_sent_attn_fwd(void* stream, int dtype, int n_sent, int D, int heads, const void* qkv, const int32_t* row0, const int32_t* lengths,
                                 int max_len, void* ctx) {
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "mts_sent_attn_fwd: bad dtype %d", dtype);
  MTS_CHECK_ARG(n_sent > 0 && D > 0 && heads > 0 && max_len > 0, "mts_sent_attn_fwd: bad shape (n_sent=%d, D=%d, heads=%d, max_len=%d)", n_sent, D,
                heads, max_len);
  MTS_CHECK_ARG(D % heads == 0, "mts_sent_attn_fwd: D=%d not divisible by heads=%d", D, heads);
  MTS_CHECK_ARG(qkv && row0 && lengths && ctx, "mts_sent_attn_fwd: null pointer");
  MTS_UNSUPPORTED(dtype == MTS_BF16, "mts_sent_attn_fwd: bf16 only (fp32 runs on mts_full_attn_fwd)");
  const int hd = D / heads;
  MTS_UNSUPPORTED(hd % 32 == 0 && hd <= 128, "mts_sent_attn_fwd: head dim %d must be a multiple of 32 and <= 128", hd);
  MTS_UNSUPPORTED(max_len <= SENT_MAX_LEN, "mts_sent_attn_fwd: max_len=%d above the %d tokens one wave covers (mts_full_attn_fwd serves it)", max_len,
                  SENT_MAX_LEN);
  MTS_UNSUPPORTED((long)n_sent * heads < (1L << 31) - ROW_WAVES, "mts_sent_attn_fwd: too many (sentence, head) pairs for one launch");
  MTS_CHECK_ARG(aligned_to(qkv, 16) && D % 8 == 0, "mts_sent_attn_fwd: qkv must be 16-byte aligned");
  SentArgs a;
  a.qkv = (const bf16_t*)qkv; a.ctx = (bf16_t*)ctx; a.row0 = row0; a.lengths = lengths;
  a.n_pairs = n_sent * heads; a.D = D; a.heads = heads; a.hd = hd;
  const int ks = max_len <= 32 ? 1 : 2;
  a.rs = 64 * ks + 16;
  const size_t lds = (size_t)ROW_WAVES * (hd + 16) * a.rs;
  const dim3 grid(ceil_div(a.n_pairs, ROW_WAVES)), block(64 * ROW_WAVES);
  hipStream_t st = (hipStream_t)stream;
  int rc = MTS_OK;
#define SENT_CALL(KK_, KS_)                                                          \
  do {                                                                               \
    rc = mts_dyn_lds(sent_attn_kernel<KK_, KS_>, lds, "mts_sent_attn_fwd");          \
    if (!rc) hipLaunchKernelGGL((sent_attn_kernel<KK_, KS_>), grid, block, lds, st, a); \
  } while (0)
#define SENT_KS(KK_) do { if (ks == 1) SENT_CALL(KK_, 1); else SENT_CALL(KK_, 2); } while (0)
  switch (hd / 32) {
    case 1: SENT_KS(1); break;
    case 2: SENT_KS(2); break;
    case 3: SENT_KS(3); break;
    default: SENT_KS(4); break;
  }
#undef SENT_KS
#undef SENT_CALL
  if (rc) return rc;
  MTS_LAUNCH_CHECK("mts_sent_attn_fwd");
  return MTS_OK;
}
