// Bootstrap resampling sums (train_fit.py:540-562 / compute_accuracy_metrics_sentence.py:63-260: 10 000 x `df.sample(frac=1, replace=True)`
// followed by a mean, per metric).  Resample s draws n documents with replacement; the M metric rows share the draw, so a resampled
// document keeps its metrics paired, as a resampled DataFrame row does.  The draw is a counter-based hash of (seed, s * n + j), the one of
// the dropout kernels (common.h: mts_hash32): no RNG state, any rank or host regenerates the same indices.
//   i_j        = (uint32)(((uint64)mts_hash32(seed, (uint64)s * n + j) * (uint64)n) >> 32)           j = 0 .. n-1
//   sums[m, s] = ((0 + values[m, i_0]) + values[m, i_1]) + ... + values[m, i_{n-1}]                  float64, one add after the other
// The multiply-shift maps 2^32 hash values onto n indices: every index gets floor(2^32 / n) or one more of them, a relative bias below
// n / 2^32 (2.5e-4 at the largest n, 1.3e-8 at n = 55).
// Mapping: one thread per (resample, metric), a block = 256 resamples of ONE metric (blockIdx.y), so a single scalar accumulator per thread
// and nothing indexed at run time.  The block stages its metric's row in LDS (dynamic, n * 8 bytes: a short row leaves the CU its
// occupancy) while n <= 8192 = 64 KiB; longer rows are read from global memory (a row is 8 MiB at most: the caches serve it).  The hash is recomputed per
// metric: 16 x at most, against M accumulators in registers and a kernel per M.  No atomics, no workspace; every element of `sums` is written.
#include "common.h"

#define BOOT_BLOCK 256
#define BOOT_LDS_MAX_N 8192          /* 8192 doubles = 64 KiB, what a kernel may use without an opt-in */

template <bool STAGE>
__global__ __launch_bounds__(BOOT_BLOCK) void bootstrap_sums_kernel(int n, int S, const double* __restrict__ values, uint64_t seed,
                                                                     double* __restrict__ sums) {
  extern __shared__ double boot_row[];
  const int m = blockIdx.y;
  const double* __restrict__ row = values + (size_t)m * n;
  if (STAGE) {
    for (int i = threadIdx.x; i < n; i += BOOT_BLOCK) boot_row[i] = row[i];
    __syncthreads();
  }
  const int s = blockIdx.x * BOOT_BLOCK + threadIdx.x;
  if (s >= S) return;                                     // behind the barrier
  const double* src = STAGE ? boot_row : row;
  const uint64_t ctr = (uint64_t)s * (uint64_t)n;
  double acc = 0.0;
#pragma unroll 4
  for (int j = 0; j < n; ++j) {
    const uint32_t i = (uint32_t)(((uint64_t)mts_hash32(seed, ctr + (uint64_t)j) * (uint64_t)n) >> 32);      // < n by construction
    acc = acc + src[i];
  }
  sums[(size_t)m * S + s] = acc;
}

extern "C" int mts_bootstrap_sums(void* stream, int n, int M, int S, const double* values, uint64_t seed, double* sums) {
  MTS_CHECK_ARG(n >= 1 && n <= (1 << 20), "mts_bootstrap_sums: n=%d, 1 .. 2^20 documents are covered", n);
  MTS_CHECK_ARG(M >= 1 && M <= 16, "mts_bootstrap_sums: M=%d, 1 .. 16 metric rows are covered", M);
  MTS_CHECK_ARG(S >= 1 && S <= (1 << 22), "mts_bootstrap_sums: S=%d, 1 .. 2^22 resamples are covered", S);
  MTS_CHECK_ARG(values && sums, "mts_bootstrap_sums: null pointer");
  const dim3 grid(ceil_div(S, BOOT_BLOCK), M);
  hipStream_t st = (hipStream_t)stream;
  if (n <= BOOT_LDS_MAX_N)
    hipLaunchKernelGGL(bootstrap_sums_kernel<true>, grid, dim3(BOOT_BLOCK), (size_t)n * sizeof(double), st, n, S, values, seed, sums);
  else
    hipLaunchKernelGGL(bootstrap_sums_kernel<false>, grid, dim3(BOOT_BLOCK), 0, st, n, S, values, seed, sums);
  MTS_LAUNCH_CHECK("mts_bootstrap_sums");
  return MTS_OK;
}
