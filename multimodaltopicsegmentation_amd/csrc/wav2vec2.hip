// wav2vec 2.0 feature encoder pieces for gfx950 (include/mts.h "wav2vec 2.0 sentence features"): what the encoder needs besides the GEMM,
// LayerNorm and full-attention entry points it is composed of (multimodaltopicsegmentation_amd/wav2vec2.py).
//
//   wave_stats    per sentence, the mean and 1 / sqrt(var + 1e-7) of its samples (Wav2Vec2FeatureExtractor's utterance normalisation): one
//                 workgroup per sentence, two passes (mean, then squared deviations), fp64 lane chains over samples tid, tid + 256, .. and a
//                 fixed tree, ONE rounding to fp32.
//   conv0_stats   layer 0 of the feature extractor (Conv1d(1, C, kernel, stride), no bias) on the normalised samples, summed per (sentence,
//                 channel) for GroupNorm(C, C): the conv output is never stored.  One workgroup per (sentence, 64 channels); wave q takes the
//                 frames q, q + 4, .. of every 128-frame tile, whose sample window is staged through LDS once; fp64 sums, fixed order.
//   conv0         the recompute: the same conv value (the same fmaf chain), normalised, affine, erf-GELU, stored time-major into the
//                 sentence's row block.  One workgroup per 64 block rows; threads map to channels (contiguous stores); rows of the block
//                 past the sentence's frames are written as zeros, so every row of the chunk is written exactly once.
//   regroup       [rows, H] -> group-major [G][rows_p, H / G] with pad_front zero rows in front of every sentence: what turns the grouped
//                 positional convolution into overlapping-row NT GEMMs.  Every row of the padded buffer is written (data or zeros).
//   pos_conv      the positional convolution on the matrix cores (bf16): y = x + gelu(conv(x) + b), one workgroup per (64-frame tile of a
//                 sentence, group).  The tile's 64 + K_p - 1 input frames x H / G channels live in LDS; in that image A[t][j * cg + c] is the
//                 element (t + j) * cg + c, so the fragment of v_mfma_f32_16x16x32_bf16 is one 16-byte LDS read.  The four waves split K,
//                 each streams its quarter of the group's weights ONCE for all 64 frames; the partial tiles meet in LDS and are added in
//                 wave order.  No atomics, every output written once.
//   rows          dst[dst_start[s] + t] = src[src_row0[s] + t] (+ res[res_row0[s] + t]): the compaction of a padded layout, the residual
//                 of the GEMM form of the positional convolution and the cast of the result, in one pass.
#include <algorithm>
#include "common.h"

#define W2V_TILE 64     // block rows / frames per workgroup (conv0, pos_conv)
#define W2V_STAT_TILE 128
#define W2V_MAXK 32

// largest s in [0, n) with start[s] <= r (start ascending, start[0] <= r)
__device__ __forceinline__ int w2v_find(const int64_t* __restrict__ start, int n, int64_t r) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct W2vSent { int64_t start, len; };
// the sentence's samples, clamped into the waveform before any address is formed
__device__ __forceinline__ W2vSent w2v_sentence(const int64_t* sent_start, const int64_t* sent_len, int s, int64_t n_wave) {
  W2vSent r;
  r.start = min(max(sent_start[s], (int64_t)0), n_wave - 1);
  r.len = min(max(sent_len[s], (int64_t)0), n_wave - r.start);
  return r;
}

__device__ __forceinline__ double w2v_block_sum(double v, double* red) {   // 256 threads, fixed tree; the result in every thread
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void w2v_wave_stats_kernel(int n_sent, const float* __restrict__ wave, int64_t n_wave,
                                                             const int64_t* __restrict__ sent_start, const int64_t* __restrict__ sent_len,
                                                             float* __restrict__ stats) {
  __shared__ double red[256];
  const int s = blockIdx.x;
  const W2vSent se = w2v_sentence(sent_start, sent_len, s, n_wave);
  const float* x = wave + se.start;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < se.len; i += 256) a += (double)x[i];
  const double n = (double)max(se.len, (int64_t)1);
  const double mean = w2v_block_sum(a, red) / n;
  double q = 0.0;
  for (int64_t i = threadIdx.x; i < se.len; i += 256) {
    const double d = (double)x[i] - mean;
    q += d * d;
  }
  const double var = w2v_block_sum(q, red) / n;
  if (threadIdx.x == 0) {
    stats[2 * (size_t)s] = (float)mean;
    stats[2 * (size_t)s + 1] = (float)(1.0 / sqrt(var + 1e-7));
  }
}

// the normalised samples first .. first + count - 1 of a sentence into LDS (0 past its end: such a sample belongs to no valid frame)
__device__ __forceinline__ void w2v_stage(float* sm, const float* __restrict__ x, int64_t first, int count, int64_t len, float mean, float rstd) {
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    const int64_t at = first + i;
    sm[i] = at < len ? (x[at] - mean) * rstd : 0.f;
  }
}

__device__ __forceinline__ float w2v_conv_at(const float* sm, const float (&w)[W2V_MAXK], int kernel) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < W2V_MAXK; ++k)
    if (k < kernel) acc = fmaf(sm[k], w[k], acc);
  return acc;
}

__device__ __forceinline__ int64_t w2v_frames(int64_t len, int kernel, int stride) { return len >= kernel ? (len - kernel) / stride + 1 : 0; }

__global__ __launch_bounds__(256) void w2v_conv0_stats_kernel(int n_sent, int C, int kernel, int stride, const float* __restrict__ wave, int64_t n_wave,
                                                              const int64_t* __restrict__ sent_start, const int64_t* __restrict__ sent_len,
                                                              const float* __restrict__ wstats, const float* __restrict__ w, float eps,
                                                              float* __restrict__ gmean, float* __restrict__ grstd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = reinterpret_cast<double*>(smem);                 // [4][64][2]
  float* sm = reinterpret_cast<float*>(smem + 4 * 64 * 2 * sizeof(double));
  const int s = blockIdx.x, cl = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int c = min(blockIdx.y * 64 + cl, C - 1);                // a clamped lane repeats channel C - 1 and stores nothing
  const W2vSent se = w2v_sentence(sent_start, sent_len, s, n_wave);
  const int64_t T = w2v_frames(se.len, kernel, stride);
  const float mean = wstats[2 * (size_t)s], rstd = wstats[2 * (size_t)s + 1];
  float wr[W2V_MAXK];
#pragma unroll
  for (int k = 0; k < W2V_MAXK; ++k) wr[k] = k < kernel ? w[(size_t)c * kernel + k] : 0.f;
  const int count = (W2V_STAT_TILE - 1) * stride + kernel;
  double sum = 0.0, sq = 0.0;
  for (int64_t t0 = 0; t0 < T; t0 += W2V_STAT_TILE) {
    __syncthreads();
    w2v_stage(sm, wave + se.start, t0 * stride, count, se.len, mean, rstd);
    __syncthreads();
    const int nf = (int)min((int64_t)W2V_STAT_TILE, T - t0);
    for (int f = q; f < nf; f += 4) {
      const double v = (double)w2v_conv_at(sm + f * stride, wr, kernel);
      sum += v;
      sq += v * v;
    }
  }
  red[(q * 64 + cl) * 2] = sum;
  red[(q * 64 + cl) * 2 + 1] = sq;
  __syncthreads();
  if (q == 0 && blockIdx.y * 64 + cl < C) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < 4; ++i) {
      a += red[(i * 64 + cl) * 2];
      b += red[(i * 64 + cl) * 2 + 1];
    }
    const double n = (double)max(T, (int64_t)1);
    const double m = a / n;
    const double var = fmax(b / n - m * m, 0.0);
    gmean[(size_t)s * C + c] = (float)m;
    grstd[(size_t)s * C + c] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void w2v_conv0_kernel(int n_sent, int C, int kernel, int stride, const float* __restrict__ wave, int64_t n_wave,
                                                        const int64_t* __restrict__ sent_start, const int64_t* __restrict__ sent_len,
                                                        const float* __restrict__ wstats, const float* __restrict__ w,
                                                        const float* __restrict__ gmean, const float* __restrict__ grstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const int64_t* __restrict__ block_start, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm = reinterpret_cast<float*>(smem);
  const int64_t r0 = (int64_t)blockIdx.x * W2V_TILE;
  const int s = w2v_find(block_start, n_sent, r0);
  const W2vSent se = w2v_sentence(sent_start, sent_len, s, n_wave);
  const int64_t Tn = w2v_frames(se.len, kernel, stride);
  const int64_t t0 = r0 - block_start[s];
  const int64_t rows_end = min(block_start[s + 1], r0 + W2V_TILE);   // blocks are whole tiles; the clamp costs nothing
  const int nrows = (int)(rows_end - r0);
  const int nf = (int)max((int64_t)0, min((int64_t)nrows, Tn - t0));
  const float mean = wstats[2 * (size_t)s], rstd = wstats[2 * (size_t)s + 1];
  if (nf > 0) w2v_stage(sm, wave + se.start, t0 * stride, (W2V_TILE - 1) * stride + kernel, se.len, mean, rstd);
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float wr[W2V_MAXK];
#pragma unroll
    for (int k = 0; k < W2V_MAXK; ++k) wr[k] = k < kernel ? w[(size_t)c * kernel + k] : 0.f;
    const float gm = gmean[(size_t)s * C + c], gr = grstd[(size_t)s * C + c], ga = gamma[c], be = beta[c];
    T* o = out + (size_t)r0 * C + c;
    for (int f = 0; f < nf; ++f) {
      const float v = w2v_conv_at(sm + f * stride, wr, kernel);
      o[(size_t)f * C] = from_f32<T>(gelu_erf_f((v - gm) * gr * ga + be));
    }
    for (int f = nf; f < nrows; ++f) o[(size_t)f * C] = from_f32<T>(0.f);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void w2v_regroup_kernel(int n_sent, int H, int G, int pad_front, const T* __restrict__ x,
                                                          const int64_t* __restrict__ src_row0, const int64_t* __restrict__ pad_start,
                                                          int64_t rows_p, T* __restrict__ out) {
  const int hv = H / 4, cg = H / G;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows_p * hv) return;
  const int64_t row = idx / hv;
  const int col = (int)(idx % hv) * 4;
  const int g = col / cg, cc = col % cg;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (row < pad_start[n_sent]) {
    const int s = w2v_find(pad_start, n_sent, row);
    const int64_t t = row - pad_start[s] - pad_front;
    if (t >= 0) load4<T>(x + (size_t)(src_row0[s] + t) * H + col, v);   // t < the sentence's frames: row < pad_start[s + 1]
  }
  store4<T>(out + ((size_t)g * rows_p + row) * cg + cc, v);
}

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void w2v_rows_kernel(int n_sent, int D, const TS* __restrict__ src, const int64_t* __restrict__ src_row0,
                                                       const TS* __restrict__ res, const int64_t* __restrict__ res_row0,
                                                       const int64_t* __restrict__ dst_start, int64_t total_rows, TD* __restrict__ dst) {
  const int dv = D / 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total_rows * dv) return;
  const int64_t row = idx / dv;
  const int col = (int)(idx % dv) * 4;
  const int s = w2v_find(dst_start, n_sent, row);
  const int64_t t = row - dst_start[s];
  float v[4];
  load4<TS>(src + (size_t)(src_row0[s] + t) * D + col, v);
  if (res) {
    float r[4];
    load4<TS>(res + (size_t)(res_row0[s] + t) * D + col, r);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += r[i];
  }
  store4<TD>(dst + (size_t)row * D + col, v);
}

// ------------------------------------------------------------------------------------------------
// positional convolution on the matrix cores
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256) void w2v_pos_conv_kernel(int n_sent, int H, int G, int Kp, const bf16_t* __restrict__ x,
                                                           const int64_t* __restrict__ src_row0, const int64_t* __restrict__ dst_start,
                                                           const int32_t* __restrict__ tile_start, const bf16_t* __restrict__ w,
                                                           const float* __restrict__ bias, bf16_t* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);                  // [W2V_TILE + Kp - 1][cg], dead once the K loop is over
  float* red = reinterpret_cast<float*>(smem);                   // [4][W2V_TILE][cg] after it
  const int cg = H / G, g = blockIdx.y, K = Kp * cg;
  int s = 0;
  {
    int lo = 0, hi = n_sent - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tile_start[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    s = lo;
  }
  const int64_t Tn = dst_start[s + 1] - dst_start[s];
  const int64_t t0 = (int64_t)((int)blockIdx.x - tile_start[s]) * W2V_TILE;
  const bf16_t* xg = x + (size_t)src_row0[s] * H + g * cg;
  const int cv = cg / 8, nstage = (W2V_TILE + Kp - 1) * cv;
  for (int i = threadIdx.x; i < nstage; i += 256) {
    const int r = i / cv, c8 = (i % cv) * 8;
    const int64_t t = t0 + r - Kp / 2;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (t >= 0 && t < Tn) v = *reinterpret_cast<const uint4*>(xg + (size_t)t * H + c8);
    *reinterpret_cast<uint4*>(xs + r * cg + c8) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
  f32x4 acc[4][NT];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nkc = K / 32;
  const int kc0 = wv * nkc / 4, kc1 = (wv + 1) * nkc / 4;
  const bf16_t* wrow[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) wrow[n] = w + ((size_t)g * cg + min(n * 16 + l15, cg - 1)) * K + 8 * l4;
  for (int kc = kc0; kc < kc1; ++kc) {
    bf16x8 b[NT], a[4];
#pragma unroll
    for (int n = 0; n < NT; ++n) b[n] = *reinterpret_cast<const bf16x8*>(wrow[n] + kc * 32);
#pragma unroll
    for (int m = 0; m < 4; ++m) a[m] = *reinterpret_cast<const bf16x8*>(xs + (m * 16 + l15) * cg + kc * 32 + 8 * l4);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], b[n], acc[m][n], 0, 0, 0);
  }
  __syncthreads();                                               // every wave is done reading xs
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int col = n * 16 + l15;
      if (col < cg) {
#pragma unroll
        for (int i = 0; i < 4; ++i) red[((size_t)wv * W2V_TILE + m * 16 + l4 * 4 + i) * cg + col] = acc[m][n][i];
      }
    }
  __syncthreads();
  const int nf = (int)min((int64_t)W2V_TILE, Tn - t0);
  const int c4n = cg / 4;
  for (int e = threadIdx.x; e < nf * c4n; e += 256) {
    const int r = e / c4n, c4 = (e % c4n) * 4;
    float v[4], xr[4];
    load4<bf16_t>(xg + (size_t)(t0 + r) * H + c4, xr);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a = red[(size_t)r * cg + c4 + i];
      a += red[((size_t)W2V_TILE + r) * cg + c4 + i];
      a += red[((size_t)2 * W2V_TILE + r) * cg + c4 + i];
      a += red[((size_t)3 * W2V_TILE + r) * cg + c4 + i];
      v[i] = xr[i] + gelu_erf_f(a + bias[g * cg + c4 + i]);
    }
    store4<bf16_t>(y + (size_t)(dst_start[s] + t0 + r) * H + g * cg + c4, v);
  }
}

// ------------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------------
extern "C" int mts_w2v_wave_stats(void* stream, int n_sent, const float* wave, int64_t total_samples, const int64_t* sent_start,
                                  const int64_t* sent_len, float* stats) {
  MTS_CHECK_ARG(n_sent >= 1 && total_samples >= 1, "mts_w2v_wave_stats: n_sent=%d, total_samples=%lld: sizes must be >= 1", n_sent, (long long)total_samples);
  MTS_CHECK_ARG(wave && sent_start && sent_len && stats, "mts_w2v_wave_stats: null pointer");
  hipLaunchKernelGGL(w2v_wave_stats_kernel, dim3(n_sent), dim3(256), 0, (hipStream_t)stream, n_sent, wave, total_samples, sent_start, sent_len, stats);
  MTS_LAUNCH_CHECK("mts_w2v_wave_stats");
  return MTS_OK;
}

static int w2v_conv0_check(const char* who, int n_sent, int C, int kernel, int stride, int64_t total_samples, int tile, size_t extra, size_t* lds) {
  MTS_CHECK_ARG(n_sent >= 1 && C >= 1 && kernel >= 1 && stride >= 1 && total_samples >= 1,
                "%s: n_sent=%d C=%d kernel=%d stride=%d total_samples=%lld: sizes must be >= 1", who, n_sent, C, kernel, stride, (long long)total_samples);
  MTS_UNSUPPORTED(C % 8 == 0, "%s: C=%d must be a multiple of 8", who, C);
  MTS_UNSUPPORTED(kernel <= W2V_MAXK, "%s: kernel=%d is wider than %d", who, kernel, W2V_MAXK);
  *lds = extra + ((size_t)(tile - 1) * stride + kernel) * sizeof(float);
  MTS_UNSUPPORTED(*lds <= 64 * 1024, "%s: stride=%d stages %zu bytes of samples per tile (> 64 KiB of LDS)", who, stride, *lds);
  return MTS_OK;
}

extern "C" int mts_w2v_conv0_stats(void* stream, int n_sent, int C, int kernel, int stride, const float* wave, int64_t total_samples,
                                   const int64_t* sent_start, const int64_t* sent_len, const float* wave_stats, const float* w, float eps,
                                   float* gmean, float* grstd) {
  size_t lds = 0;
  int rc = w2v_conv0_check("mts_w2v_conv0_stats", n_sent, C, kernel, stride, total_samples, W2V_STAT_TILE, 4 * 64 * 2 * sizeof(double), &lds);
  if (rc) return rc;
  MTS_CHECK_ARG(wave && sent_start && sent_len && wave_stats && w && gmean && grstd, "mts_w2v_conv0_stats: null pointer");
  MTS_CHECK_ARG(eps >= 0.f, "mts_w2v_conv0_stats: eps must not be negative");
  hipLaunchKernelGGL(w2v_conv0_stats_kernel, dim3(n_sent, ceil_div(C, 64)), dim3(256), lds, (hipStream_t)stream, n_sent, C, kernel, stride, wave,
                     total_samples, sent_start, sent_len, wave_stats, w, eps, gmean, grstd);
  MTS_LAUNCH_CHECK("mts_w2v_conv0_stats");
  return MTS_OK;
}

extern "C" int mts_w2v_conv0(void* stream, int out_dtype, int n_sent, int C, int kernel, int stride, const float* wave, int64_t total_samples,
                             const int64_t* sent_start, const int64_t* sent_len, const float* wave_stats, const float* w, const float* gmean,
                             const float* grstd, const float* gamma, const float* beta, const int64_t* block_start, int64_t total_rows, void* out) {
  size_t lds = 0;
  int rc = w2v_conv0_check("mts_w2v_conv0", n_sent, C, kernel, stride, total_samples, W2V_TILE, 0, &lds);
  if (rc) return rc;
  MTS_CHECK_ARG(out_dtype == MTS_F32 || out_dtype == MTS_BF16, "mts_w2v_conv0: bad out_dtype %d", out_dtype);
  MTS_CHECK_ARG(wave && sent_start && sent_len && wave_stats && w && gmean && grstd && gamma && beta && block_start && out, "mts_w2v_conv0: null pointer");
  MTS_CHECK_ARG(total_rows >= W2V_TILE && total_rows % W2V_TILE == 0, "mts_w2v_conv0: total_rows=%lld must be a positive multiple of %d", (long long)total_rows, W2V_TILE);
  MTS_UNSUPPORTED(total_rows / W2V_TILE < (1LL << 31), "mts_w2v_conv0: more rows than one launch covers");
  const dim3 grid((unsigned)(total_rows / W2V_TILE));
  if (out_dtype == MTS_F32)
    hipLaunchKernelGGL(w2v_conv0_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, n_sent, C, kernel, stride, wave, total_samples, sent_start,
                       sent_len, wave_stats, w, gmean, grstd, gamma, beta, block_start, (float*)out);
  else
    hipLaunchKernelGGL(w2v_conv0_kernel<bf16_t>, grid, dim3(256), lds, (hipStream_t)stream, n_sent, C, kernel, stride, wave, total_samples, sent_start,
                       sent_len, wave_stats, w, gmean, grstd, gamma, beta, block_start, (bf16_t*)out);
  MTS_LAUNCH_CHECK("mts_w2v_conv0");
  return MTS_OK;
}

static int w2v_pos_check(const char* who, int n_sent, int H, int G, int Kp) {
  MTS_CHECK_ARG(n_sent >= 1 && H >= 1 && G >= 1 && Kp >= 1, "%s: n_sent=%d H=%d G=%d K_p=%d: sizes must be >= 1", who, n_sent, H, G, Kp);
  MTS_CHECK_ARG(H % G == 0, "%s: H=%d is not divisible by G=%d", who, H, G);
  MTS_UNSUPPORTED((H / G) % 8 == 0, "%s: H / G = %d must be a multiple of 8", who, H / G);
  MTS_UNSUPPORTED(Kp % 2 == 0 && Kp <= 128, "%s: K_p=%d must be even and at most 128", who, Kp);
  return MTS_OK;
}

extern "C" int mts_w2v_regroup(void* stream, int dtype, int n_sent, int H, int G, int Kp, const void* x, const int64_t* src_row0,
                               const int64_t* pad_start, int64_t rows_p, void* out) {
  int rc = w2v_pos_check("mts_w2v_regroup", n_sent, H, G, Kp);
  if (rc) return rc;
  MTS_CHECK_ARG(dtype == MTS_F32 || dtype == MTS_BF16, "mts_w2v_regroup: bad dtype %d", dtype);
  MTS_CHECK_ARG(x && src_row0 && pad_start && out && rows_p >= 1, "mts_w2v_regroup: null pointer or rows_p < 1");
  MTS_CHECK_ARG(aligned_to(x, 16) && aligned_to(out, 16), "mts_w2v_regroup: x and out must be 16-byte aligned");
  const int64_t nblk = (rows_p * (H / 4) + 255) / 256;
  MTS_UNSUPPORTED(nblk < (1LL << 31), "mts_w2v_regroup: more rows than one launch covers");
  if (dtype == MTS_F32)
    hipLaunchKernelGGL(w2v_regroup_kernel<float>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, n_sent, H, G, Kp / 2, (const float*)x, src_row0,
                       pad_start, rows_p, (float*)out);
  else
    hipLaunchKernelGGL(w2v_regroup_kernel<bf16_t>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, n_sent, H, G, Kp / 2, (const bf16_t*)x, src_row0,
                       pad_start, rows_p, (bf16_t*)out);
  MTS_LAUNCH_CHECK("mts_w2v_regroup");
  return MTS_OK;
}

extern "C" int mts_w2v_rows(void* stream, int src_dtype, int dst_dtype, int n_sent, int D, const void* src, const int64_t* src_row0, const void* res,
                            const int64_t* res_row0, const int64_t* dst_start, int64_t total_rows, void* dst) {
  MTS_CHECK_ARG(n_sent >= 1 && D >= 1 && total_rows >= 1, "mts_w2v_rows: n_sent=%d D=%d total_rows=%lld: sizes must be >= 1", n_sent, D, (long long)total_rows);
  MTS_CHECK_ARG((src_dtype == MTS_F32 || src_dtype == MTS_BF16) && (dst_dtype == MTS_F32 || dst_dtype == MTS_BF16), "mts_w2v_rows: bad dtype");
  MTS_CHECK_ARG(src && src_row0 && dst_start && dst && (!res || res_row0), "mts_w2v_rows: null pointer");
  MTS_CHECK_ARG(D % 4 == 0 && aligned_to(src, 16) && aligned_to(res, 16) && aligned_to(dst, 16), "mts_w2v_rows: D %% 4 and 16-byte aligned matrices are expected");
  const int64_t nblk = (total_rows * (D / 4) + 255) / 256;
  MTS_UNSUPPORTED(nblk < (1LL << 31), "mts_w2v_rows: more rows than one launch covers");
#define W2V_ROWS(TS, TD)                                                                                                                  \
  hipLaunchKernelGGL((w2v_rows_kernel<TS, TD>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, n_sent, D, (const TS*)src, src_row0, \
                     (const TS*)res, res_row0, dst_start, total_rows, (TD*)dst)
  if (src_dtype == MTS_F32 && dst_dtype == MTS_F32) W2V_ROWS(float, float);
  else if (src_dtype == MTS_F32) W2V_ROWS(float, bf16_t);
  else if (dst_dtype == MTS_F32) W2V_ROWS(bf16_t, float);
  else W2V_ROWS(bf16_t, bf16_t);
#undef W2V_ROWS
  MTS_LAUNCH_CHECK("mts_w2v_rows");
  return MTS_OK;
}

extern "C" int mts_w2v_pos_conv(void* stream, int n_sent, int H, int G, int Kp, const void* x, const int64_t* src_row0, const int64_t* dst_start,
                                const int32_t* tile_start, int n_tiles, const void* w, const float* bias, void* y) {
  int rc = w2v_pos_check("mts_w2v_pos_conv", n_sent, H, G, Kp);
  if (rc) return rc;
  MTS_CHECK_ARG(x && src_row0 && dst_start && tile_start && w && bias && y && n_tiles >= 1, "mts_w2v_pos_conv: null pointer or n_tiles < 1");
  MTS_CHECK_ARG(aligned_to(x, 16) && aligned_to(w, 16) && aligned_to(y, 16), "mts_w2v_pos_conv: x, w and y must be 16-byte aligned");
  const int cg = H / G;
  MTS_UNSUPPORTED(cg <= 64 && (Kp * cg) % 128 == 0 && G <= 65535, "mts_w2v_pos_conv: H / G = %d (at most 64), K_p * H / G = %d (a multiple of 128) or G=%d is not covered: use the GEMM form",
                  cg, Kp * cg, G);
  const size_t lds = std::max((size_t)(W2V_TILE + Kp - 1) * cg * sizeof(bf16_t), (size_t)4 * W2V_TILE * cg * sizeof(float));
  const dim3 grid((unsigned)n_tiles, (unsigned)G);
#define W2V_POS(NT_)                                                                                                                              \
  hipLaunchKernelGGL(w2v_pos_conv_kernel<NT_>, grid, dim3(256), lds, (hipStream_t)stream, n_sent, H, G, Kp, (const bf16_t*)x, src_row0, dst_start, \
                     tile_start, (const bf16_t*)w, bias, (bf16_t*)y)
  switch (ceil_div(cg, 16)) {
    case 1: W2V_POS(1); break;
    case 2: W2V_POS(2); break;
    case 3: W2V_POS(3); break;
    default: W2V_POS(4); break;
  }
#undef W2V_POS
  MTS_LAUNCH_CHECK("mts_w2v_pos_conv");
  return MTS_OK;
}
