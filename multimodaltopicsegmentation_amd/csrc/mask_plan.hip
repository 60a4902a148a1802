// Negative-sentence masking (reference: --mask_inner_sentences / --mask_probability, utils/load_datasets_precomputed.py:174-185: a random
// share of a training document's non-boundary sentences is dropped), moved from load time onto the device: the PLAN of a masked batch.
// For batch row b, document d = doc_index[b] with rows r = 0 .. n-1, row r is KEPT when its label is not 0 or when
//   (uint64) mts_hash32(doc_seed[b], r) < T,   T = clamp((uint64)(keep_probability * 2^32), 0, 2^32)
// (the counter hash of common.h: no RNG state, any rank and the host regenerate the same draw); a non-empty document none of whose rows
// is kept keeps row 0.  The kept rows move up in order (a stream compaction): src_row[b, t] = the document-relative index of the t-th
// kept row, -1 behind the last one, kept[b] = their number (not clipped to Lmax).  mts_gather_rows (gather.hip) then builds every tensor
// of the batch from that table.
//
// Mapping: one workgroup of MASK_CHUNK threads per batch row walks its document MASK_CHUNK rows at a time, a thread per row.  The keep
// flag is one label load and one hash; a row's place among the kept ones is
//   (kept in earlier chunks: a register) + (kept in the waves below: four counts through LDS) + (kept in the lanes below: popcount of
//   the wave's 64-bit ballot under the lane's mask).
// The waves' counts are double-buffered, so a chunk costs one barrier.  Every element of src_row and kept is written exactly once by a
// plain vector store: the kept rows' places in the walk, the places behind them in a tail loop, row 0 of the empty-draw rule by the
// thread that would have written it.  No memset, no atomics, no workspace; integers, so bitwise reproducible.
#include "common.h"

namespace {

constexpr int MASK_CHUNK = 256;                      // rows per trip of the workgroup = its threads
constexpr int MASK_WAVES = MASK_CHUNK / MTS_WAVE;

__global__ __launch_bounds__(MASK_CHUNK) void mask_plan_kernel(const float* __restrict__ targets, const int64_t* __restrict__ row_start, int n_docs,
                                                               const int32_t* __restrict__ doc_index, const uint64_t* __restrict__ doc_seed,
                                                               uint64_t threshold, int Lmax, int32_t* __restrict__ src_row,
                                                               int32_t* __restrict__ kept) {
  __shared__ int wave_kept[2][MASK_WAVES];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (MTS_WAVE - 1), wave = tid >> 6;
  const int d = doc_index[b];
  int64_t first = 0;
  int n = 0;
  if ((unsigned)d < (unsigned)n_docs) {
    first = row_start[d];
    n = (int)min(row_start[d + 1] - first, (int64_t)0x7fffffff);  // table entries are int32
  }
  const uint64_t seed = doc_seed[b];
  int32_t* __restrict__ out = src_row + (int64_t)b * Lmax;
  int base = 0;  // rows kept in the chunks walked so far
  int buf = 0;
  for (int64_t c0 = 0; c0 < n; c0 += MASK_CHUNK) {  // n, and so the trip count, is uniform over the workgroup: the barrier is reached by all
    const int64_t r = c0 + tid;
    const bool keep = r < n && (targets[first + r] != 0.0f || (uint64_t)mts_hash32(seed, (uint64_t)r) < threshold);
    const unsigned long long votes = __ballot(keep);
    const int below = __popcll(votes & ((1ull << lane) - 1ull));
    if (lane == 0) wave_kept[buf][wave] = __popcll(votes);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < MASK_WAVES; ++w) {
      const int k = wave_kept[buf][w];
      before += w < wave ? k : 0;
      all += k;
    }
    const int t = base + before + below;
    if (keep && t < Lmax) out[t] = (int32_t)r;
    base += all;
    buf ^= 1;  // the next chunk's counts go to the other half: nobody still reads this one behind the next barrier
  }
  if (base == 0 && n > 0) {  // the empty-draw rule: row 0 stays
    base = 1;
    if (tid == 0) out[0] = 0;
  }
  for (int t = min(base, Lmax) + tid; t < Lmax; t += MASK_CHUNK) out[t] = -1;
  if (tid == 0) kept[b] = base;
}

}  // namespace

extern "C" int mts_mask_plan(void* stream, int B, int Lmax, const float* targets, const int64_t* row_start, int n_docs, const int32_t* doc_index,
                             const uint64_t* doc_seed, double keep_probability, int32_t* src_row, int32_t* kept) {
  MTS_CHECK_ARG(B >= 0 && Lmax >= 1 && n_docs >= 1, "mts_mask_plan: bad shape (B %d, Lmax %d, n_docs %d)", B, Lmax, n_docs);
  MTS_CHECK_ARG(keep_probability >= 0.0 && keep_probability <= 1.0, "mts_mask_plan: keep_probability %g is outside [0, 1]", keep_probability);
  if (B == 0) return MTS_OK;
  MTS_CHECK_ARG(targets && row_start && doc_index && doc_seed && src_row && kept, "mts_mask_plan: null pointer");
  const double scaled = keep_probability * 4294967296.0;  // in [0, 2^32] by the check above; exact at both ends
  const uint64_t threshold = scaled >= 4294967296.0 ? 4294967296ull : (uint64_t)scaled;
  hipLaunchKernelGGL(mask_plan_kernel, dim3((unsigned)B), dim3(MASK_CHUNK), 0, (hipStream_t)stream, targets, row_start, n_docs, doc_index, doc_seed,
                     threshold, Lmax, src_row, kept);
  MTS_LAUNCH_CHECK("mts_mask_plan");
  return MTS_OK;
}
