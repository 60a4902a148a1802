// Decision-threshold sweep: for every document x threshold the six integers from which Pk, WindowDiff and boundary-F1 follow exactly
// (include/mts.h).  Replaces the host loop of models/lightning_model.py:435-553 over compute_Pk / compute_window_diff / f1_score.
//
// One 256-thread workgroup per (document, threshold).  A document's two boundary sequences (hypothesis h_i = p_i > th, target t_i) are
// kept in LDS as BIT MASKS, one 64-bit word per 64 sentences -- exactly what __ballot hands a wave -- next to the exclusive prefix count
// of every word, so the segment index of sentence x is   pos(x) = prefix[x / 64] + popcount(mask[x / 64] & below(x % 64)).
// 65 536 sentences are 2 x 8 KiB of masks and 2 x 4 KiB of prefixes: every supported length takes the same path and needs no workspace
// (the window k reaches n / 2, so no halo of positions would bound LDS; the masks do).
//   phase 1  scores, targets -> masks (one ballot per 64 sentences; the probability is decode_prob, the expression greedy decode uses)
//   phase 2  exclusive scan of the words' popcounts (4 words per thread, wave scan by shuffles, wave totals through LDS)
//   phase 3  k from the target's segment count, then the windows i < n - k and the F1 counts word by word; five integer block sums
// Integers only after the compare: results are identical from run to run.  The one lane that owns the result writes it with plain stores.
// Phases 1 and 2 are __device__ functions: winpr_sweep_kernel (the three integers of WinPR, metric 'scaiano') runs them too and differs
// in phase 3 alone -- n + k windows of a fixed width k, each two sweep_pos differences plus one bit of the window before.
#include "common.h"
#include "loss_elems.h"

#define SWEEP_MAX_L 65536
#define SWEEP_WORDS (SWEEP_MAX_L / 64)
#define SWEEP_MAX_T 64
#define WINPR_MAX_K 64

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// number of boundaries strictly before sentence x
__device__ __forceinline__ int sweep_pos(const uint64_t* mask, const int* pre, int x) {
  const int w = x >> 6, bit = x & 63;
  return pre[w] + __popcll(mask[w] & ((1ull << bit) - 1ull));
}

// ---- phase 1: scores, targets -> masks; ends in a barrier.  clear_last: bit n - 1 stays 0 in both masks (WinPR under end_boundary) ------
__device__ __forceinline__ void sweep_masks(int b, int L, int Lt, int n_out, const float* __restrict__ scores,
                                            const float* __restrict__ targets, float th, int n, bool clear_last, uint64_t* mh, uint64_t* mt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nwords = (n + 63) >> 6;
  const int live = clear_last ? n - 1 : n;
  for (int w = wave; w < nwords; w += 4) {
    const int i = w * 64 + lane;
    bool h = false, t = false;
    if (i < live) {
      const float p = decode_prob(scores, (size_t)b * L + i, n_out);
      h = p > th;                                                      // strict, as greedy_decode_kernel
      t = targets[(size_t)b * Lt + i] == 1.f;
    }
    const uint64_t bh = __ballot(h), bt = __ballot(t);
    if (lane == 0) { mh[w] = bh; mt[w] = bt; }
  }
  __syncthreads();
}

// ---- phase 2: exclusive prefix of the words' popcounts (4 words per thread); ends in a barrier ----------------------------------------
__device__ __forceinline__ void sweep_prefixes(int nwords, const uint64_t* mh, const uint64_t* mt, int* ph, int* pt, int (*wtot)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ch[4], ct[4], sh = 0, st = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int w = tid * 4 + u;
    ch[u] = w < nwords ? __popcll(mh[w]) : 0;
    ct[u] = w < nwords ? __popcll(mt[w]) : 0;
    sh += ch[u];
    st += ct[u];
  }
  int ih = sh, it = st;                                                // inclusive scan over the wave's lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int uh = __shfl_up(ih, off, 64), ut = __shfl_up(it, off, 64);
    if (lane >= off) { ih += uh; it += ut; }
  }
  if (lane == 63) { wtot[0][wave] = ih; wtot[1][wave] = it; }
  __syncthreads();
  int eh = ih - sh, et = it - st;                                      // exclusive, then the waves in front
  for (int v = 0; v < wave; ++v) { eh += wtot[0][v]; et += wtot[1][v]; }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int w = tid * 4 + u;
    if (w < nwords) { ph[w] = eh; pt[w] = et; }
    eh += ch[u];
    et += ct[u];
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void threshold_sweep_kernel(int B, int L, int Lt, int n_out, const float* __restrict__ scores,
                                                               const float* __restrict__ targets, const int32_t* __restrict__ lengths, int T,
                                                               const float* __restrict__ thresholds, int end_boundary,
                                                               int32_t* __restrict__ counts_out) {
  __shared__ uint64_t mh[SWEEP_WORDS], mt[SWEEP_WORDS];
  __shared__ int ph[SWEEP_WORDS], pt[SWEEP_WORDS];
  __shared__ int wtot[2][4];
  __shared__ int red[5][4];
  const int b = blockIdx.x / T, j = blockIdx.x % T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* out = counts_out + (size_t)blockIdx.x * 6;
  const int n = lengths ? min(max(lengths[b], 0), L) : L;
  if (n == 0) {                                                        // uniform over the workgroup
    if (tid < 6) out[tid] = 0;
    return;
  }
  const int nwords = (n + 63) >> 6;
  sweep_masks(b, L, Lt, n_out, scores, targets, thresholds[j], n, false, mh, mt);
  sweep_prefixes(nwords, mh, mt, ph, pt, wtot);

  // ---- phase 3: window and counts ------------------------------------------------------------------------------------------
  // k = max(round_half_even(n / (2 nseg)), 2) in integers; nseg = 1 + the target's boundaries before its last sentence
  const int nseg2 = 2 * (1 + sweep_pos(mt, pt, n - 1));
  const int q = n / nseg2, r2 = 2 * (n % nseg2);
  int k = r2 > nseg2 ? q + 1 : (r2 == nseg2 ? q + (q & 1) : q);
  k = max(k, 2);
  const int W = max(n - k, 0);
  int pk = 0, wd = 0, tp = 0, fp = 0, fn = 0;
  for (int i = tid; i < W; i += 256) {                                 // i + k <= n - 1
    const int dh = sweep_pos(mh, ph, i + k) - sweep_pos(mh, ph, i);
    const int dt = sweep_pos(mt, pt, i + k) - sweep_pos(mt, pt, i);
    pk += ((dh == 0) != (dt == 0)) ? 1 : 0;
    wd += (dh != dt) ? 1 : 0;
  }
  // F1 as test_step leaves its operands: the target's last sentence is 0 (compute_Pk restored it so), the hypothesis' too under end_boundary
  const int lw = (n - 1) >> 6;
  const uint64_t lbit = 1ull << ((n - 1) & 63);
  for (int w = tid; w < nwords; w += 256) {
    uint64_t h = mh[w], t = mt[w];
    if (w == lw) {
      t &= ~lbit;
      if (end_boundary) h &= ~lbit;
    }
    tp += __popcll(h & t);
    fp += __popcll(h & ~t);
    fn += __popcll(t & ~h);
  }
  pk = wave_sum_i(pk); wd = wave_sum_i(wd); tp = wave_sum_i(tp); fp = wave_sum_i(fp); fn = wave_sum_i(fn);
  if (lane == 0) { red[0][wave] = pk; red[1][wave] = wd; red[2][wave] = tp; red[3][wave] = fp; red[4][wave] = fn; }
  __syncthreads();
  if (tid == 0) {
    int s[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) s[c] = red[c][0] + red[c][1] + red[c][2] + red[c][3];
    out[0] = s[0]; out[1] = s[1]; out[2] = W; out[3] = s[2]; out[4] = s[3]; out[5] = s[4];
  }
}

// WinPR (Scaiano & Inkpen 2012) of upstream's call WinPR(reference = tags, hypothesis = target): {TP, FP, FN} over the n + k windows
// i = 1 - k .. n (include/mts.h).  The masks carry one word more than the document, all zeros with the document's total as its prefix,
// so that sweep_pos(n) is the count of the whole document also when n is a multiple of 64.
__global__ __launch_bounds__(256) void winpr_sweep_kernel(int B, int L, int Lt, int n_out, const float* __restrict__ scores,
                                                           const float* __restrict__ targets, const int32_t* __restrict__ lengths, int T,
                                                           const float* __restrict__ thresholds, int end_boundary, int k,
                                                           int32_t* __restrict__ counts_out) {
  __shared__ uint64_t mh[SWEEP_WORDS + 1], mt[SWEEP_WORDS + 1];
  __shared__ int ph[SWEEP_WORDS + 1], pt[SWEEP_WORDS + 1];
  __shared__ int wtot[2][4];
  __shared__ int red[3][4];
  const int b = blockIdx.x / T, j = blockIdx.x % T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* out = counts_out + (size_t)blockIdx.x * 3;
  const int n = lengths ? min(max(lengths[b], 0), L) : L;
  if (n == 0) {                                                        // uniform over the workgroup
    if (tid < 3) out[tid] = 0;
    return;
  }
  const int nwords = (n + 63) >> 6;
  sweep_masks(b, L, Lt, n_out, scores, targets, thresholds[j], n, end_boundary != 0, mh, mt);
  sweep_prefixes(nwords, mh, mt, ph, pt, wtot);
  if (tid == 0) {
    mh[nwords] = 0; mt[nwords] = 0;
    ph[nwords] = ph[nwords - 1] + __popcll(mh[nwords - 1]);
    pt[nwords] = pt[nwords - 1] + __popcll(mt[nwords - 1]);
  }
  __syncthreads();

  int tp = 0, fp = 0, fn = 0;
  for (int idx = tid; idx < n + k; idx += 256) {
    const int i = idx + 1 - k;                                         // 1 - k .. n
    const int lo = max(i, 0), hi = min(i + k, n);                      // 0 <= lo <= hi <= n
    int R = sweep_pos(mh, ph, hi) - sweep_pos(mh, ph, lo);
    int C = sweep_pos(mt, pt, hi) - sweep_pos(mt, pt, lo);
    // the first element of the previous window's slice [i-1 : i-1+k]; for a negative start python wraps around (non-empty only for n < k)
    int p = -1;
    if (i >= 1) {
      p = i - 1;
    } else if (i >= 2 - k) {
      const int plo = max(n + i - 1, 0), phi = min(i - 1 + k, n);
      if (plo < phi) p = plo;
    }
    if (p >= 0) {
      R += (int)((mh[p >> 6] >> (p & 63)) & 1ull);
      C += (int)((mt[p >> 6] >> (p & 63)) & 1ull);
    }
    tp += min(R, C);
    fp += max(0, C - R);
    fn += max(0, R - C);
  }
  tp = wave_sum_i(tp); fp = wave_sum_i(fp); fn = wave_sum_i(fn);
  if (lane == 0) { red[0][wave] = tp; red[1][wave] = fp; red[2][wave] = fn; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = red[c][0] + red[c][1] + red[c][2] + red[c][3];
  }
}

extern "C" int mts_threshold_sweep(void* stream, int B, int L, int Lt, int n_out, const float* scores, const float* targets,
                                   const int32_t* lengths, int T, const float* thresholds, int end_boundary, int32_t* counts_out) {
  MTS_CHECK_ARG(B > 0 && L > 0 && Lt >= L && scores && targets && thresholds && counts_out, "mts_threshold_sweep: bad arguments");
  MTS_CHECK_ARG(n_out >= 1 && n_out <= 4, "mts_threshold_sweep: n_out=%d is outside 1..4", n_out);
  MTS_CHECK_ARG(T >= 1 && T <= SWEEP_MAX_T, "mts_threshold_sweep: T=%d thresholds, 1..%d are covered", T, SWEEP_MAX_T);
  MTS_UNSUPPORTED(L <= SWEEP_MAX_L, "mts_threshold_sweep: L=%d sentences, documents up to %d are covered", L, SWEEP_MAX_L);
  MTS_UNSUPPORTED((long long)B * T <= 0x7fffffffLL / 6, "mts_threshold_sweep: B * T = %lld workgroups", (long long)B * T);
  hipLaunchKernelGGL(threshold_sweep_kernel, dim3(B * T), dim3(256), 0, (hipStream_t)stream, B, L, Lt, n_out, scores, targets, lengths, T,
                     thresholds, end_boundary, counts_out);
  MTS_LAUNCH_CHECK("mts_threshold_sweep");
  return MTS_OK;
}

extern "C" int mts_winpr_sweep(void* stream, int B, int L, int Lt, int n_out, const float* scores, const float* targets,
                               const int32_t* lengths, int T, const float* thresholds, int end_boundary, int k, int32_t* counts_out) {
  MTS_CHECK_ARG(B > 0 && L > 0 && Lt >= L && scores && targets && thresholds && counts_out, "mts_winpr_sweep: bad arguments");
  MTS_CHECK_ARG(n_out >= 1 && n_out <= 4, "mts_winpr_sweep: n_out=%d is outside 1..4", n_out);
  MTS_CHECK_ARG(T >= 1 && T <= SWEEP_MAX_T, "mts_winpr_sweep: T=%d thresholds, 1..%d are covered", T, SWEEP_MAX_T);
  MTS_CHECK_ARG(k >= 1 && k <= WINPR_MAX_K, "mts_winpr_sweep: k=%d, windows of 1..%d sentences are covered", k, WINPR_MAX_K);
  MTS_UNSUPPORTED(L <= SWEEP_MAX_L, "mts_winpr_sweep: L=%d sentences, documents up to %d are covered", L, SWEEP_MAX_L);
  MTS_UNSUPPORTED((long long)B * T <= 0x7fffffffLL / 3, "mts_winpr_sweep: B * T = %lld workgroups", (long long)B * T);
  hipLaunchKernelGGL(winpr_sweep_kernel, dim3(B * T), dim3(256), 0, (hipStream_t)stream, B, L, Lt, n_out, scores, targets, lengths, T,
                     thresholds, end_boundary, k, counts_out);
  MTS_LAUNCH_CHECK("mts_winpr_sweep");
  return MTS_OK;
}
