// What the kernels over resident waveforms share (mfcc.hip, prosody.hip): the sentence table and librosa's centred framing.
#pragma once
#include "common.h"

__device__ __forceinline__ int64_t mf_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int mf_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the sentence of frame f: the largest s in 0 .. n_sent - 1 with frame_start[s] <= f (0 when there is none)
__device__ __forceinline__ int mf_sentence_of(const int64_t* __restrict__ frame_start, int n_sent, int64_t f) {
  int lo = 0, hi = n_sent - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (frame_start[mid] <= f)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// np.pad(y, ., 'reflect') as an index: period 2 (n - 1), the end samples not repeated; n >= 1
__device__ __forceinline__ int64_t mf_fold(int64_t pos, int64_t n) {
  if (pos >= 0 && pos < n) return pos;
  if (n == 1) return 0;
  const int64_t p = 2 * (n - 1);
  int64_t m = pos % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

__device__ __forceinline__ void mf_store(void* out, int out_dtype, int64_t at, float v) {
  if (out_dtype == MTS_F32)
    reinterpret_cast<float*>(out)[at] = v;
  else
    reinterpret_cast<bf16_t*>(out)[at] = from_f32<bf16_t>(v);
}
