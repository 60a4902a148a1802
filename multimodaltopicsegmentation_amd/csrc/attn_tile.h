// Tile helpers shared by the attention translation units (band_attn.hip, full_attn.hip, t5_local_attn.hip, text_encoder.hip): the
// kernels of the first three have one lane layout, 256 threads = (row t = tid/8, group g = tid%8) over 32-row tiles staged in LDS,
// and the bf16 matrix-core kernels of the last three have one fragment layout.  Everything is inlined; literal arguments (tile sizes,
// a fixed head dim) fold.
#pragma once
#include <algorithm>
#include "band_common.h"

// ---- generic (VALU) kernels ----------------------------------------------------------------------
// rows [first, first + nrows) of one head's slice of a row-major [., ld] matrix into LDS (row stride rs bytes); rows outside
// [0, limit) -> 0
template <typename T>
__device__ __forceinline__ void attn_stage_rows(char* dst, int rs, const T* __restrict__ base, int ld, int first, int nrows, int limit, int hd) {
  constexpr int VEC = 16 / sizeof(T);
  const int cpr = hd / VEC;                      // 16-byte chunks per row
  for (int idx = threadIdx.x; idx < nrows * cpr; idx += 256) {
    const int r = idx / cpr, ch = idx % cpr;
    const int j = first + r;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (j >= 0 && j < limit) v = *reinterpret_cast<const uint4*>(base + (size_t)j * ld + ch * VEC);
    *reinterpret_cast<uint4*>(dst + r * rs + ch * 16) = v;
  }
}

__device__ __forceinline__ float attn_dot16(const uint4& a, const uint4& b, float acc, float) {   // 4 fp32 pairs
  acc = fmaf(__uint_as_float(a.x), __uint_as_float(b.x), acc);
  acc = fmaf(__uint_as_float(a.y), __uint_as_float(b.y), acc);
  acc = fmaf(__uint_as_float(a.z), __uint_as_float(b.z), acc);
  acc = fmaf(__uint_as_float(a.w), __uint_as_float(b.w), acc);
  return acc;
}
__device__ __forceinline__ float attn_dot16(const uint4& a, const uint4& b, float acc, bf16_t) {  // 8 bf16 pairs
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a.x), __builtin_bit_cast(bf16x2, b.x), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a.y), __builtin_bit_cast(bf16x2, b.y), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a.z), __builtin_bit_cast(bf16x2, b.z), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a.w), __builtin_bit_cast(bf16x2, b.w), acc, false);
  return acc;
}

// s[c] = <a_row, b_rows[8c, :]>, c = 0..3 (the caller has offset a_row to its row and b_rows to its first row)
template <typename T>
__device__ __forceinline__ void attn_scores(const char* a_row, const char* b_rows, int rs, int hd, float (&s)[4]) {
  constexpr int VEC = 16 / sizeof(T);
  const int cpr = hd / VEC;
  s[0] = s[1] = s[2] = s[3] = 0.f;
  for (int ch = 0; ch < cpr; ++ch) {
    const uint4 av = *reinterpret_cast<const uint4*>(a_row + ch * 16);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint4 bv = *reinterpret_cast<const uint4*>(b_rows + (8 * c) * rs + ch * 16);
      s[c] = attn_dot16(av, bv, s[c], T());
    }
  }
}

// acc[u][0..3] += sum_{c < ncc} coef[c * coef_stride] * rows[c][4 (g + 8u) ..]: 8 lanes x MAXU chunks of 4 cover the head dim
template <typename T, int MAXU>
__device__ __forceinline__ void attn_accum(const float* coef, int coef_stride, const char* rows, int rs, int hd, int g, int ncc,
                                           float (&acc)[MAXU][4]) {
  const int nch = hd / 4;
  for (int c = 0; c < ncc; ++c) {
    const float p = coef[c * coef_stride];
    const T* row = reinterpret_cast<const T*>(rows + c * rs);
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
      const int ch = g + 8 * u;
      if (ch < nch) {
        float v[4];
        load4<T>(row + 4 * ch, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u][e] = fmaf(p, v[e], acc[u][e]);
      }
    }
  }
}

__device__ __forceinline__ float lanes8_max(float v) {    // over the 8 lanes that share a row
  v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64));
  return v;
}
__device__ __forceinline__ float lanes8_sum(float v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
  return v;
}

#define PS 33   // LDS row stride (floats) of a 32 x 32 coefficient tile

// ---- bf16 matrix-core kernels: v_mfma_f32_16x16x32_bf16, 4 waves x 16 rows per workgroup -----------
// Every product is X . Y^T with X and Y row-major LDS images whose rows run along the summed index: lane l takes
// X[row l&15][8(l>>4) .. +7] as the A fragment and Y[row l&15][8(l>>4) .. +7] as the B fragment of one 32-wide k-step, and the
// 16 x 16 result sits at C[row 4(l>>4) + r][col l&15], r = 0..3.
#define MQ 64                 // rows per workgroup
#define MK 32                 // columns per step
#define TRS (MK * 2 + 16)     // bytes per row of a transposed [dim][32] image (16-byte aligned, padded)

__device__ __forceinline__ bf16x8 attn_frag(const char* img, int rs, int row, int col_elem) {
  return *reinterpret_cast<const bf16x8*>(img + row * rs + col_elem * 2);
}

// rows [first, first + n) of one head's slice into a row-major image `img` (if any) and / or its transpose timg[d][r] (if any;
// row stride TRS, so n <= 32 with it); rows outside [0, limit) -> 0
__device__ __forceinline__ void attn_mstage(char* img, int rs, char* timg, const bf16_t* __restrict__ base, int ld, int first, int n, int limit,
                                            int hd) {
  const int cpr = hd / 8;
  for (int idx = threadIdx.x; idx < n * cpr; idx += 256) {
    const int r = idx / cpr, ch = idx % cpr;
    const int j = first + r;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (j >= 0 && j < limit) v = *reinterpret_cast<const uint4*>(base + (size_t)j * ld + ch * 8);
    if (img) *reinterpret_cast<uint4*>(img + r * rs + ch * 16) = v;
    if (timg) {
      const bf16_t* e = reinterpret_cast<const bf16_t*>(&v);
#pragma unroll
      for (int t = 0; t < 8; ++t) *reinterpret_cast<bf16_t*>(timg + (ch * 8 + t) * TRS + r * 2) = e[t];
    }
  }
}

// acc[ct] += X[x0 + 0..15] . Y[16 ct + 0..15]^T over kk k-steps of 32
template <int NCT>
__device__ __forceinline__ void attn_mm_xyt(const char* X, int xrs, int x0, const char* Y, int yrs, int kk, int lane, f32x4 (&acc)[NCT]) {
  const int l15 = lane & 15, g = lane >> 4;
  for (int k = 0; k < kk; ++k) {
    const bf16x8 a = attn_frag(X, xrs, x0 + l15, 32 * k + 8 * g);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
      acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, attn_frag(Y, yrs, 16 * ct + l15, 32 * k + 8 * g), acc[ct], 0, 0, 0);
  }
}

// 16 x 16 NCT coefficient tile (C layout, NCT 16-column parts) -> bf16 image W[16][16 NCT] of this wave (row stride rs bytes)
template <int NCT>
__device__ __forceinline__ void attn_put_coef_n(char* W, int rs, int lane, const float (&c)[NCT][4]) {
  const int l15 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<bf16_t*>(W + (4 * g + r) * rs + (16 * ct + l15) * 2) = (bf16_t)c[ct][r];
}
// 16 x 32 coefficient tile (two 16-column halves) -> bf16 image W[16][32] of this wave (row stride TRS)
__device__ __forceinline__ void attn_put_coef(char* W, int lane, const float (&c)[2][4]) { attn_put_coef_n<2>(W, TRS, lane, c); }

// ---- one wave per sequence (text_encoder.hip): operands straight from global memory, images private to the wave --------
// the fragment of k-step k for row `row` of one head's slice (both operands of X . Y^T run along the head dim, so a row of q or k IS
// the fragment: 16 bytes per lane, no staging); rows outside [0, limit) -> 0 and are never read
__device__ __forceinline__ bf16x8 attn_gfrag(const bf16_t* __restrict__ base, int ld, int row, int limit, int k, int lane) {
  bf16x8 f = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < limit) f = *reinterpret_cast<const bf16x8*>(base + (size_t)row * ld + 32 * k + 8 * (lane >> 4));
  return f;
}

// rows [0, n) of one head's slice -> the transpose timg[d][r] (row stride rs bytes) by ONE wave; rows in [limit, n) -> 0
__device__ __forceinline__ void attn_wave_tstage(char* timg, int rs, const bf16_t* __restrict__ base, int ld, int n, int limit, int hd, int lane) {
  const int cpr = hd / 8;
  for (int idx = lane; idx < n * cpr; idx += 64) {
    const int r = idx / cpr, ch = idx % cpr;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < limit) v = *reinterpret_cast<const uint4*>(base + (size_t)r * ld + ch * 8);
    const bf16_t* e = reinterpret_cast<const bf16_t*>(&v);
#pragma unroll
    for (int t = 0; t < 8; ++t) *reinterpret_cast<bf16_t*>(timg + (ch * 8 + t) * rs + r * 2) = e[t];
  }
}

// what one wave wrote to its LDS images is visible to its other lanes behind this (no workgroup barrier: the waves are independent)
__device__ __forceinline__ void attn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float lanes16_max(float v) {   // over the 16 lanes that hold one row of a C fragment
  v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64)); v = fmaxf(v, __shfl_xor(v, 8, 64));
  return v;
}
__device__ __forceinline__ float lanes16_sum(float v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
  return v;
}

// ---- host side -----------------------------------------------------------------------------------
// LDS row stride = 16 B x odd: 16 rows at one column hit 16 distinct 16-byte bank slots
static inline int attn_row_stride(int hd, int esize) {
  int bytes = ((hd * esize + 15) / 16) * 16;
  if (((bytes / 16) & 1) == 0) bytes += 16;
  return bytes;
}

// dropout on the attention probabilities (p = 0: the struct's "off" state, drop_thr = 0, stays)
template <class Args> static int attn_set_dropout(Args& a, float p, uint64_t seed, const char* who) {
  MTS_CHECK_ARG(p >= 0.f && p < 1.f, "%s: dropout probability has to be between 0 and 1, but got %f", who, (double)p);
  if (p > 0.f) {
    a.drop_thr = (uint32_t)std::max<double>(1.0, std::min<double>(4294967295.0, (double)p * 4294967296.0));
    a.drop_scale = 1.0f / (1.0f - p);
    a.drop_seed = seed;
  }
  return MTS_OK;
}
