// Pieces shared by the 256x224 bf16 GEMM family: gemm224.hip (eight waves) and the four-wave kernels of gemm224r.hip (NT, one tile per
// workgroup), gemm224p.hip (NT, persistent), gemm224n.hip (NN) and gemm224t.hip (TN).  What differs between those files is the K-loop schedule;
// everything a schedule is built from -- tile order, lane offsets of the LDS-DMA copies, fragment addresses, the K-major fragment reads and MFMA
// block, the residual tile through the LDS, the bf16 store pass, the launchers' "does this kernel take the call" terms -- lives here.  (Two kernels
// keep a piece written out, each with a note why: gemm_bf16_224p_kernel and the eight-wave kernel came out with other register or spill counts
// with their fragment offsets and store passes routed through the helpers.)
#pragma once
#include "gemm_common.h"

#define G224_BN 224                           // tile: 256 rows x 224 columns
#define G224_HN 112                           // columns of a wave (half a tile)

typedef __attribute__((address_space(3))) void dlptr_t;        // destination of a buffer-load LDS-DMA

// buffer resource over "everything from p on": raw 32-bit offsets, no bounds worth the name (the launchers keep every offset below 0x7ff00000)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, 0x7ffffff0, 0x00020000);
}

// ---- tile order: tile id (after xcd_remap) -> origin.  order != 0: bands of four tile rows, column-major inside a band (the 32 tiles an XCD works
// on at a time form a 4 x 8 block: 4 A panels + 8 B panels per K-step); order == 0: row-major
__device__ __forceinline__ void tile_origin(int id, int ntn, int ntm, int order, int& bm0, int& bn0) {
  if (order == 0) { bm0 = (id / ntn) * 256; bn0 = (id % ntn) * G224_BN; return; }
  const int band = id / (4 * ntn), within = id - band * 4 * ntn;
  const int rows = min(4, ntm - band * 4);
  bm0 = (band * 4 + within % rows) * 256;
  bn0 = (within / rows) * G224_BN;
}

// ---- lane offsets (bytes) of the LDS-DMA copies.  A copy moves a 1-KiB piece that is lane-contiguous in the LDS (16 B per lane); the swizzle is
// applied on the SOURCE side, and of a copy's address only this lane part is a vector: the rest (resource, piece rows + K offset) is scalar.
// K-major operand, piece = 8 rows x 128 B: lane (row8 = lane >> 3, pos = lane & 7) fetches chunk pos ^ ((row >> 1) & 7) of its row, row = 8 piece +
// row8 -- one of two offsets by the parity of the piece.
__device__ __forceinline__ void kmajor_copy_offsets(int lane, int ld, unsigned (&vo)[2]) {
  const int row8 = lane >> 3, pos = lane & 7;
  const unsigned keyE = (unsigned)((row8 >> 1) & 7), keyO = (unsigned)(((row8 >> 1) + 4) & 7);
  vo[0] = (unsigned)(row8 * ld + (int)((pos ^ keyE) * 8)) * 2u;
  vo[1] = (unsigned)(row8 * ld + (int)((pos ^ keyO) * 8)) * 2u;
}
// k-strided operand, piece = 4 k-rows x 256 B of one half image: lane (lr = lane >> 4, c16 = lane & 15) fills k-row lr, 32-B slot c16 >> 1, half
// c16 & 1; slot s of k-row r holds source column block s ^ key(r), key(r) = (r & 3) | (((r >> 3) & 1) << 2) (gemm_common.h strided_off) -- r = 4 piece
// + lr, so the key is lr | (bit 1 of the piece number << 2): two offsets.  clip = 112: the half image holds 112 used columns of 128 and the lanes of
// the unused 16 fetch 16 columns further left (nobody reads what they bring); clip = 0: all 128 columns are used.
__device__ __forceinline__ void strided_copy_offsets(int lane, int ld, int clip, unsigned (&vo)[2]) {
  const int lr = lane >> 4, c16 = lane & 15;
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int key = lr | (par << 2);
    const int col = (((c16 >> 1) ^ key) << 4) + ((c16 & 1) << 3);
    vo[par] = (unsigned)(lr * ld + (clip && col >= clip ? col - 16 : col)) * 2u;
  }
}

// ---- fragment addresses = lane part (below) + image base + instruction immediate.  Everywhere in this header (r16, g) = (lane & 15, lane >> 4), the
// lane's row and column group in a 16x16 MFMA block; the helpers take them from the kernel, which has them in registers anyway.
// K-major: kmajor_off(16 t + r16, ks * 4 + g) = t * 2048 + lk[ks]
__device__ __forceinline__ void kmajor_frag_offsets(int r16, int g, unsigned (&lk)[2], unsigned base = 0) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) lk[ks] = base + r16 * 128 + (((ks * 4 + g) ^ ((r16 >> 1) & 7)) << 4);
}
// strided: strided_off(ks * 32 + 8 g + q, 16 c + 4 p) = ks * 8192 + (sx ^ (c << 5)): X[k = 8 g + q (+ 4), column block c, columns 4 p ..] through two
// transposing reads (gemm_common.h frag_strided)
__device__ __forceinline__ unsigned strided_frag_offset(int r16, int g) {
  const int q = r16 >> 2, p = r16 & 3;
  return (unsigned)((8 * g + q) * 256 + 8 * p + ((q | ((g & 1) << 2)) << 5));
}
template <int NC>
__device__ __forceinline__ void strided_frag_offsets(int r16, int g, unsigned base, unsigned (&ax)[NC]) {
  const unsigned sx = strided_frag_offset(r16, g);
#pragma unroll
  for (int c = 0; c < NC; ++c) ax[c] = base + (sx ^ (unsigned)(c << 5));
}

// ---- K-major fragment reads and the MFMA block of the four-wave NT kernels (gemm224r.hip, gemm224p.hip): a wave owns 128 x 112 of the tile, per
// k-step 8 A fragments x 7 B fragments, one ds_read_b128 each.
// (free function templates, not generic lambdas: clang rejects inline-asm operands that name variables captured by a generic lambda)
// request R (0..14) of k-step KS: 0..6 = B fragment R, 7..14 = A fragment R - 7 (fA / fB: the wave's image bases incl. the stage)
template <int KS, int R>
__device__ __forceinline__ void kmajor_rd(s16x8 (&fa)[2][8], s16x8 (&fb)[2][7], unsigned fA, unsigned fB, const unsigned (&lk)[2]) {
  if constexpr (R < 7) {
    const unsigned ad = fB + lk[KS];
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[KS][R]) : "v"(ad), "n"(R * 2048));
  } else {
    const unsigned ad = fA + lk[KS];
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fa[KS][R - 7]) : "v"(ad), "n"((R - 7) * 2048));
  }
}
// block N = 8 ks + i: A fragment i of k-step ks x the 7 B fragments.  ZERO: the accumulators of row block i start here (C = 0)
template <int N, bool ZERO>
__device__ __forceinline__ void kmajor_block(f32x4 (&acc)[8][7], s16x8 (&fa)[2][8], s16x8 (&fb)[2][7]) {
  constexpr int ks = N >> 3, i = N & 7;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" : "+v"(fa[ks][i]));
  const bf16x8 va = __builtin_bit_cast(bf16x8, fa[ks][i]);
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    asm volatile("" : "+v"(fb[ks][j]));
    if constexpr (ZERO) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fb[ks][j]), va, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fb[ks][j]), va, acc[i][j], 0, 0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
}
// block N (0..7) of a K-tile, the part both NT schedules share: the wait that covers the block's fragments (on entry the 15 reads of k-step 0 are
// in flight, B first; LDS returns in order), the block, and behind it two of the 15 reads of k-step 1 (fA / fB: the wave's image bases in stage 0,
// st: the K-tile's stage of STAGE bytes)
template <int N, bool ZERO, int STAGE>
__device__ __forceinline__ void kmajor_step0(f32x4 (&acc)[8][7], s16x8 (&fa)[2][8], s16x8 (&fb)[2][7], unsigned fA, unsigned fB, int st,
                                             const unsigned (&lk)[2]) {
  lgkm_wait<(7 - N) + 2 * N>();
  kmajor_block<N, ZERO>(acc, fa, fb);
  if constexpr (2 * N < 15) kmajor_rd<1, (2 * N < 15 ? 2 * N : 0)>(fa, fb, fA + st * STAGE, fB + st * STAGE, lk);
  if constexpr (2 * N + 1 < 15) kmajor_rd<1, (2 * N + 1 < 15 ? 2 * N + 1 : 0)>(fa, fb, fA + st * STAGE, fB + st * STAGE, lk);
}

// ---- the residual tile of a wave (128 rows x 112 columns) through the LDS (gemm224r.hip, gemm224n.hip: one tile per workgroup, so nothing hides
// the memory round trip of 56 loads per lane in the epilogue).  A copy moves four rows x 14 chunks of 16 B by 56 of the 64 lanes into 1 KiB; copy c
// (0..15) of half h (rows 64 h ..) lands at base + c * 1024 of the 16 KiB the caller gives the wave and half.
struct ResidualViaLds {
  __amdgpu_buffer_rsrc_t rs; unsigned vo; int row4;
  __device__ __forceinline__ void init(const GemmArgs& a, bool has_res, int m0, int n0, int lane) {
    rs = make_rsrc(has_res ? (const void*)(reinterpret_cast<const bf16_t*>(a.residual) + (size_t)m0 * a.ldr + n0) : a.A);
    vo = (unsigned)((lane / 14) * a.ldr + (lane % 14) * 8) * 2u;
    row4 = 8 * a.ldr;                                              // bytes per 4 rows of the residual
  }
  __device__ __forceinline__ void copy(int c, int h, char* dst16k, int lane) const {
    if (lane < 56) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (dlptr_t*)(dst16k + c * 1024), 16, vo, (h * 16 + c) * row4, 0, 0);
  }
  // row group i (0..7) of the wave's 128 rows = rows (i & 3) * 16 + r16 of half i >> 2 (src16k: that half's 16 KiB): copy (row >> 2), lane slot
  // (row & 3) * 14 + chunk; 8 bytes per (row, 16-column block)
  static __device__ __forceinline__ void read(int i, const char* src16k, int r16, int g, uint2 (&r)[7]) {
    const int rr = (i & 3) * 16 + r16;
    const char* rp = src16k + (rr >> 2) * 1024 + ((rr & 3) * 14 + (g >> 1)) * 16 + (g & 1) * 8;
#pragma unroll
    for (int j = 0; j < 7; ++j) r[j] = *reinterpret_cast<const uint2*>(rp + j * 32);
  }
};

// ---- the bf16 store pass: 16 rows x 112 columns of a wave.  Lane (r16, g) holds val(j) = the four finished fp32 values of row r16, columns j * 16 +
// 4 g .. + 3; they go as bf16 through a wave-private staging area (240-byte rows: 16 B of padding) so that HBM sees 16-byte pieces of contiguous
// 224-byte row segments, not the 8-byte pieces of the accumulator layout.
template <class Val>
__device__ __forceinline__ void store_pass_224(bf16_t* C, int ldc, int row0, int n0, char* stage, int lane, int r16, int g, Val&& val) {
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const f32x4 v = val(j);
    uint2 pk;
    pk.x = pack_bf16x2(v[0], v[1]);
    pk.y = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<uint2*>(stage + r16 * 240 + (j * 16 + 4 * g) * 2) = pk;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = it * 64 + lane;
    const int row = idx / 14, ch = idx - row * 14;
    if (idx < 16 * 14) {
      const uint4 val16 = *reinterpret_cast<const uint4*>(stage + row * 240 + ch * 16);
      *reinterpret_cast<uint4*>(C + (size_t)(row0 + row) * ldc + n0 + ch * 8) = val16;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ---- the simple epilogue (full tiles, bf16 C, bias / column scale / residual only) of a wave whose tile starts at (m0, n0).  BRANCH-FREE so that
// every vector-memory wait in it can be counted: without a bias / residual the loads still execute, from a few cache lines at the start of A (always
// mapped, >= 4 KiB), and their values are discarded by a select.
struct Epi224 {
  const float* bias_p; const bf16_t* res_p; size_t res_ld; bool has_bias, has_res; float colscale; int ncols_scaled;
  // init = init_loads (what the loads need) + init_scale (what the arithmetic needs): a kernel that fetches its bias ahead of the K loop calls the
  // first there and the second in its epilogue, so that the lane's column count does not occupy a register across the loop
  __device__ __forceinline__ void init_loads(const GemmArgs& a, int m0, int n0, bool first_slice, int r16, int g) {
    has_bias = (a.epi & MTS_EPI_BIAS) && first_slice;
    has_res = (a.epi & MTS_EPI_RESIDUAL) && first_slice;
    bias_p = has_bias ? a.bias + n0 + 4 * g : reinterpret_cast<const float*>(a.A) + 4 * g;
    res_ld = has_res ? (size_t)a.ldr : 0;
    res_p = has_res ? reinterpret_cast<const bf16_t*>(a.residual) + (size_t)(m0 + r16) * a.ldr + n0 + 4 * g
                    : reinterpret_cast<const bf16_t*>(a.A) + 4 * g;
  }
  __device__ __forceinline__ void init_scale(const GemmArgs& a, int n0, int g) {
    colscale = (a.epi & MTS_EPI_COLSCALE) ? a.colscale : 1.0f;
    ncols_scaled = (a.epi & MTS_EPI_COLSCALE) ? a.ncols_scaled - n0 - 4 * g : 0;
  }
  __device__ __forceinline__ void init(const GemmArgs& a, int m0, int n0, bool first_slice, int lane) {
    const int r16 = lane & 15, g = lane >> 4;
    init_loads(a, m0, n0, first_slice, r16, g);
    init_scale(a, n0, g);
  }
  __device__ __forceinline__ void load_bias(float4 (&b)[7]) const {
#pragma unroll
    for (int j = 0; j < 7; ++j) b[j] = *reinterpret_cast<const float4*>(bias_p + j * 16);
  }
  __device__ __forceinline__ void load_res(int i, uint2 (&r)[7]) const {       // rows m0 + i*16 + r16 of the wave's tile
#pragma unroll
    for (int j = 0; j < 7; ++j) r[j] = *reinterpret_cast<const uint2*>(res_p + (size_t)(i * 16) * res_ld + j * 16);
  }
  // acc = (acc + bias) * scale for the whole 64 x 112 wave tile of the eight-wave kernel
  __device__ __forceinline__ void fold_bias(f32x4 (&acc)[4][7], const float4 (&b)[7]) const {
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const float sc = (j * 16 < ncols_scaled) ? colscale : 1.0f;
      const float4 bb = has_bias ? b[j] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[i][j][0] = (acc[i][j][0] + bb.x) * sc;
        acc[i][j][1] = (acc[i][j][1] + bb.y) * sc;
        acc[i][j][2] = (acc[i][j][2] + bb.z) * sc;
        acc[i][j][3] = (acc[i][j][3] + bb.w) * sc;
      }
    }
  }
  // rows i*16 .. i*16+15 of the wave tile: (acc + bias) * scale + residual -> store pass
  __device__ __forceinline__ void pass(const GemmArgs& a, const f32x4 (&acc)[7], const float4 (&b)[7], const uint2 (&r)[7], int i, int m0, int n0, char* stage,
                                       int lane, int r16, int g) const {
    store_pass_224(reinterpret_cast<bf16_t*>(a.C), a.ldc, m0 + i * 16, n0, stage, lane, r16, g, [&](int j) {
      const float sc = (j * 16 < ncols_scaled) ? colscale : 1.0f;
      const float4 bb = has_bias ? b[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      const uint2 rr = has_res ? r[j] : make_uint2(0u, 0u);
      return (f32x4){(acc[j][0] + bb.x) * sc + bf16_lo(rr.x), (acc[j][1] + bb.y) * sc + bf16_hi(rr.x), (acc[j][2] + bb.z) * sc + bf16_lo(rr.y),
                     (acc[j][3] + bb.w) * sc + bf16_hi(rr.y)};
    });
  }
};

// ---- host side: the terms of the launchers' "does this kernel take the call" predicates
// an operand of LDS-DMA copies: 16-byte pieces, and every byte offset of a copy (`span`: the largest one inside a tile's panels) stays below 2^31
inline bool g224_operand_ok(const void* p, int ld, size_t span) { return ld % 8 == 0 && ((uintptr_t)p & 15) == 0 && span < 0x7ff00000u; }
inline size_t g224_kmajor_span(int rows, int ld, int K) { return (size_t)rows * ld * 2 + (size_t)K * 2; }   // `rows` rows of K-major panels
inline size_t g224_strided_span(int kdepth, int ld) { return ((size_t)kdepth + 64) * ld * 2; }                // kdepth k-rows of a k-strided operand
// bf16 C in 16-byte pieces
__host__ __device__ inline bool g224_c_bf16_ok(const GemmArgs& a) { return (a.ldc % 8 == 0) && (((uintptr_t)a.C & 15) == 0); }
// the simple epilogue (Epi224) applies; res_bytes: the pieces the residual is read in (16: through the LDS, ResidualViaLds; 8: into registers)
__host__ __device__ inline bool g224_simple_epi_ok(const GemmArgs& a, int res_bytes) {
  const unsigned simple = MTS_EPI_BIAS | MTS_EPI_COLSCALE | MTS_EPI_RESIDUAL;
  return !a.slab && (a.epi & ~simple) == 0 && (!(a.epi & MTS_EPI_COLSCALE) || a.ncols_scaled % 4 == 0) &&
         (!(a.epi & MTS_EPI_RESIDUAL) || (a.ldr % (res_bytes / 2) == 0 && ((uintptr_t)a.residual & (uintptr_t)(res_bytes - 1)) == 0)) &&
         (!(a.epi & MTS_EPI_BIAS) || ((uintptr_t)a.bias & 15) == 0);
}
