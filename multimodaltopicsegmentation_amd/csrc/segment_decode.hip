// Prediction pass: scores -> boundary tags, probabilities and the per-document SEGMENT TABLE, in one launch (include/mts.h
// mts_segment_decode; predict.py).  Replaces the host loop a caller of the taggers runs today -- tag lists per document, then
// get_boundaries per list -- and adds a decode the per-sentence threshold cannot express: the best boundary set under a MINIMUM SEGMENT
// LENGTH m (an extension; at m = 1 it is the greedy rule of greedy_decode_kernel, bit for bit).
//
// One 256-thread workgroup per document of n sentences.  Boundary bits and the recurrence's take bits live in LDS as 64-bit masks, one
// word per 64 sentences, next to the exclusive prefix popcount of every tag word (the idiom of threshold_sweep.hip phases 1-2), so the
// place of a boundary in the segment table is   pre[i / 64] + popcount(mask[i / 64] & below(i % 64))   (mask_plan.hip's compaction).
//   phase 1  p_i = decode_prob (the ONE expression greedy decode and the sweeps share) -> prob; at m = 1 also the tag masks, a ballot per
//            64 sentences, and phase 2 is skipped
//   phase 2  m >= 2: the recurrence over t = m-1 .. n-1-m in exact integers, q_t = rint(p_t 2^32) - rint(th 2^32):
//              cand_t = q_t + best(t - m);  take_t = cand_t > best(t - 1);  best(t) = max(best(t - 1), cand_t);  best(u < m - 1) = 0
//            The weights q are staged in LDS a tile of DEC_TILE at a time by all four waves; wave 0 walks the tile in runs of
//            W = min(m, 64) positions, a lane per position: every cand of a run reads best() of an EARLIER run (W <= m), so a run is one
//            add per lane and a prefix maximum over the lanes (shuffles), carried from run to run in a register.  best() is kept as a
//            ring of m values in LDS, slot t mod m, read and then written by the lane that owns t -- never an [n] array.  Then one lane
//            walks back from t = n-1-m: the highest take bit at or below t becomes a tag, t continues m below it.
//   phase 3  exclusive scan of the tag words' popcounts (4 words per thread, wave scan by shuffles, wave totals through LDS)
//   phase 4  tags, the segment table (one entry per tag bit, the tail entry, -1 behind) and n_seg
// Integers after decode_prob; every element of every output is written exactly once by a plain vector store: no atomics, no workspace,
// no memset, the same bits on every call.
#include "common.h"
#include "loss_elems.h"

#define DEC_MAX_L 65536
#define DEC_WORDS (DEC_MAX_L / 64)
#define DEC_MAX_M 1024
#define DEC_TILE 2048

namespace {

constexpr long long DEC_NEG = (long long)0x8000000000000000ull;  // below every cand: |cand| < 2^49

__device__ __forceinline__ long long dec_max(long long a, long long b) { return a > b ? a : b; }
__device__ __forceinline__ long long dec_fixed(float p) { return __double2ll_rn((double)p * 4294967296.0); }  // rint, half to even

__global__ __launch_bounds__(256) void segment_decode_kernel(int L, int n_out, const float* __restrict__ scores,
                                                              const int32_t* __restrict__ lengths, float threshold, long long T, int m,
                                                              int close_last, int Smax, uint8_t* __restrict__ tags, float* __restrict__ prob,
                                                              int32_t* __restrict__ seg_end, int32_t* __restrict__ n_seg) {
  __shared__ uint64_t mtag[DEC_WORDS], mtake[DEC_WORDS];
  __shared__ int pre[DEC_WORDS];
  __shared__ long long ring[DEC_MAX_M];
  __shared__ long long stage[DEC_TILE];
  __shared__ int wtot[4];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lengths ? min(max(lengths[b], 0), L) : L;
  const size_t row = (size_t)b * L;
  const int nwords = (n + 63) >> 6;

  // ---- phase 1 -------------------------------------------------------------------------------------------------------------
  if (m == 1) {
    for (int w = wave; w < nwords; w += 4) {
      const int i = w * 64 + lane;
      bool h = false;
      if (i < n) {
        const float p = decode_prob(scores, row + i, n_out);
        h = p > threshold;                                             // strict, as greedy_decode_kernel
        if (prob) prob[row + i] = p;
      }
      const uint64_t bh = __ballot(h);
      if (lane == 0) mtag[w] = bh;
    }
    if (prob)
      for (int i = n + tid; i < L; i += 256) prob[row + i] = 0.f;
  } else {
    if (prob)
      for (int i = tid; i < L; i += 256) prob[row + i] = i < n ? decode_prob(scores, row + i, n_out) : 0.f;
    for (int w = tid; w < nwords; w += 256) { mtag[w] = 0; mtake[w] = 0; }
  }
  __syncthreads();

  // ---- phase 2: the recurrence and the walk back (m >= 2) --------------------------------------------------------------------
  if (m >= 2 && n > 0) {
    const int lo = m - 1, hi = n - 1 - m;                               // the eligible interior boundaries; none when n < 2m
    const int W = min(m, 64);
    long long carry = 0;                                                // best(first position of the run - 1), wave 0
    for (int g0 = lo; g0 <= hi; g0 += DEC_TILE) {                       // uniform over the workgroup: every barrier is reached by all
      const int cnt = min(DEC_TILE, hi + 1 - g0);
      for (int i = tid; i < cnt; i += 256) stage[i] = dec_fixed(decode_prob(scores, row + g0 + i, n_out)) - T;
      __syncthreads();
      if (wave == 0) {
        for (int c0 = 0; c0 < cnt; c0 += W) {
          const int nact = min(W, cnt - c0);                            // a run never crosses the tile: shorter runs are as good
          const int t = g0 + c0 + lane;
          const bool act = lane < nact;
          const int slot = t % m;
          long long cand = DEC_NEG;
          if (act) cand = stage[c0 + lane] + (t - m >= lo ? ring[slot] : 0ll);
          long long x = cand;                                           // inclusive prefix maximum over the run's lanes
          for (int off = 1; off < nact; off <<= 1) {
            const long long y = __shfl_up(x, off, 64);
            if (lane >= off) x = dec_max(x, y);
          }
          long long before = __shfl_up(x, 1, 64);
          before = lane == 0 ? carry : dec_max(carry, before);          // best(t - 1)
          const long long best = dec_max(carry, x);
          if (act) ring[slot] = best;
          const uint64_t votes = __ballot(act && cand > before);        // strict
          carry = __shfl(best, nact - 1, 64);
          if (lane == 0 && votes) {
            const int p0 = g0 + c0, w = p0 >> 6, s = p0 & 63;
            mtake[w] |= votes << s;
            if (s + nact > 64) mtake[w + 1] |= votes >> (64 - s);       // s > 0 here; w + 1 < nwords since the run ends below n
          }
          __builtin_amdgcn_wave_barrier();                              // the ring and the masks are this wave's own: program order
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      int t = hi;
      while (t >= lo) {
        int w = t >> 6;
        uint64_t bits = mtake[w] & (~0ull >> (63 - (t & 63)));
        while (bits == 0 && w > 0) bits = mtake[--w];
        if (bits == 0) break;
        const int u = w * 64 + 63 - __clzll((long long)bits);
        mtag[u >> 6] |= 1ull << (u & 63);
        t = u - m;
      }
      if (decode_prob(scores, row + n - 1, n_out) > threshold) mtag[(n - 1) >> 6] |= 1ull << ((n - 1) & 63);   // the last sentence: greedy
    }
    __syncthreads();
  }

  // ---- phase 3: exclusive prefix of the tag words' popcounts --------------------------------------------------------------------
  int cw[4], sw = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int w = tid * 4 + u;
    cw[u] = w < nwords ? __popcll(mtag[w]) : 0;
    sw += cw[u];
  }
  int iw = sw;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(iw, off, 64);
    if (lane >= off) iw += up;
  }
  if (lane == 63) wtot[wave] = iw;
  __syncthreads();
  int ew = iw - sw;
  for (int v = 0; v < wave; ++v) ew += wtot[v];
  const int total = wtot[0] + wtot[1] + wtot[2] + wtot[3];               // boundaries of the document
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int w = tid * 4 + u;
    if (w < nwords) pre[w] = ew;
    ew += cw[u];
  }
  __syncthreads();

  // ---- phase 4: the outputs ----------------------------------------------------------------------------------------------------
  int32_t* __restrict__ ends = seg_end + (size_t)b * Smax;
  for (int i = tid; i < L; i += 256) {
    bool h = false;
    if (i < n) {
      const int w = i >> 6, bit = i & 63;
      const uint64_t word = mtag[w];
      h = (word >> bit) & 1ull;
      if (h) {
        const int j = pre[w] + __popcll(word & ((1ull << bit) - 1ull));
        if (j < Smax) ends[j] = i + 1;                                  // an exclusive end
      }
    }
    if (tags) tags[row + i] = h ? 1 : 0;
  }
  const bool tail = close_last && n > 0 && !((mtag[(n - 1) >> 6] >> ((n - 1) & 63)) & 1ull);
  const int count = total + (tail ? 1 : 0);
  if (tid == 0) {
    if (tail && total < Smax) ends[total] = n;
    n_seg[b] = count;                                                   // not clipped to Smax (mts_mask_plan's rule)
  }
  for (int j = min(count, Smax) + tid; j < Smax; j += 256) ends[j] = -1;
}

}  // namespace

extern "C" int mts_segment_decode(void* stream, int B, int L, int n_out, const float* scores, const int32_t* lengths, float threshold,
                                  int min_segment, int close_last, int Smax, uint8_t* tags, float* prob, int32_t* seg_end, int32_t* n_seg) {
  MTS_CHECK_ARG(B >= 0 && L >= 1 && Smax >= 1, "mts_segment_decode: bad shape (B %d, L %d, Smax %d)", B, L, Smax);
  MTS_CHECK_ARG(n_out >= 1 && n_out <= 4, "mts_segment_decode: n_out=%d is outside 1..4", n_out);
  MTS_UNSUPPORTED(L <= DEC_MAX_L, "mts_segment_decode: L=%d sentences, documents up to %d are covered", L, DEC_MAX_L);
  MTS_UNSUPPORTED(min_segment >= 1 && min_segment <= DEC_MAX_M, "mts_segment_decode: min_segment=%d, 1..%d are covered", min_segment, DEC_MAX_M);
  // the fixed-point threshold of the constrained decode must fit: a NaN fails both comparisons
  MTS_CHECK_ARG(min_segment == 1 || (threshold >= -1024.f && threshold <= 1024.f),
                "mts_segment_decode: threshold %g is outside [-1024, 1024] (min_segment >= 2 decodes in 32.32 fixed point)", (double)threshold);
  if (B == 0) return MTS_OK;
  MTS_CHECK_ARG(scores && seg_end && n_seg, "mts_segment_decode: null pointer");
  const long long T = min_segment == 1 ? 0ll : (long long)__builtin_rint((double)threshold * 4294967296.0);   // half to even
  hipLaunchKernelGGL(segment_decode_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, L, n_out, scores, lengths, threshold, T,
                     min_segment, close_last, Smax, tags, prob, seg_end, n_seg);
  MTS_LAUNCH_CHECK("mts_segment_decode");
  return MTS_OK;
}
