// Prosodic sentence features from resident waveforms (audio.ResidentAudio.pitch / yin / prosodic; reference:
// extract_acoustic_features.py:20-55 and :74-108, the `prosodic` encoder: per sentence librosa.pyin(y, fmin=70, fmax=500), the pause and
// voiced-segment statistics of its voicing probability, mean and std of a 40-band mel power spectrogram and of its delta, and the pitch jump
// against the previous sentence's plain-YIN track).  The definition is librosa 0.8.1's, restated in include/mts.h; what is computed here:
//
//   mts_yin_frames      wave -> cmnd, shift [total_frames, n_lags]: the cumulative-mean-normalised difference function and its parabolic
//                       shifts.  One workgroup of 256 threads per frame.  The frame's samples x[1 .. W + max_period] lie in LDS; a thread
//                       owns one lag tau and walks j: x[j] is the same address for every lane (a broadcast, read as one 16-byte access per
//                       four j), x[j + tau] is consecutive dwords over consecutive lanes (32 lanes on 32 banks: conflict-free).  7.5 KiB of
//                       LDS per workgroup, so the waves per CU are set by registers, not LDS.  DIRECT form: no FFT autocorrelation.
//   mts_pyin_observe    cmnd, shift -> voiced_prob [total_frames] and the fp64 log-observations [total_frames, 2 n_bins].  One wave per
//                       frame; troughs are compacted by ballots and prefix counts, the 100 thresholds are walked with one ballot each.
//   mts_pyin_viterbi    log-observations -> state, f0, voiced flag.  One workgroup per sentence, a thread per state, the frames in sequence,
//                       all fp64: per candidate one rounded add and an exact compare.
//   mts_yin_pick        cmnd, shift -> the plain-YIN f0.  One wave per frame.
//   mts_frame_delta     the Savitzky-Golay slope of mts_mfcc_frames over any fp32 [total_frames, D].
//   mts_prosodic_stats  f0, voiced_prob, previous plain-YIN f0 -> the six scalar columns and pitch_jump.  One wave per sentence; runs of
//                       pause frames are measured with ballots and prefix masks, every sum is a lane chain and a shuffle tree in fp64.
//
// No atomics, no workgroup depends on another inside a launch, every output element is written exactly once by a vector store.
#include <float.h>

#include "frame_common.h"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_FB = 16;            // frames per workgroup of the delta launch
constexpr int PR_MAX_FRAME = 4096;
constexpr int PR_MAX_STATES = 1024;  // one thread per state
constexpr int PR_MAX_WAVES = PR_MAX_STATES / MTS_WAVE;

__device__ __forceinline__ uint64_t pr_lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

__device__ __forceinline__ double pr_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int pr_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------------- yin frames
__global__ __launch_bounds__(PR_THREADS) void yin_frames_kernel(const float* __restrict__ wave, int64_t total_samples,
                                                                const int64_t* __restrict__ sent_start, const int64_t* __restrict__ sent_len,
                                                                const int64_t* __restrict__ frame_start, int64_t total_frames, int n_sent,
                                                                int frame_length, int win, int hop, int min_period, int max_period,
                                                                float* __restrict__ cmnd, float* __restrict__ shift) {
  extern __shared__ __attribute__((aligned(16))) float pr_lds[];
  const int tid = threadIdx.x;
  const int n_lags = max_period - min_period + 1;
  const int need = win + max_period;  // xs[i] = x[1 + i], i < need
  const int NX = (need + 3) & ~3;
  float* xs = pr_lds;
  float* d = xs + NX;              // d[tau], tau = 1 .. max_period (d[0] unused)
  float* cs = d + max_period + 1;  // cs[tau] = d[1] + .. + d[tau]
  float* cm = cs + max_period + 1; // cm[i] = cmnd of lag i

  const int64_t f = blockIdx.x;
  const int s = mf_sentence_of(frame_start, n_sent, f);
  const int64_t t = f - mf_clamp(frame_start[s], total_frames);
  const int64_t s0 = mf_clamp(sent_start[s], total_samples);
  const int64_t n = mf_clamp(sent_len[s], total_samples - s0);
  float* __restrict__ crow = cmnd + f * n_lags;
  float* __restrict__ srow = shift + f * n_lags;
  if (n <= 0) {  // uniform over the workgroup
    for (int i = tid; i < n_lags; i += PR_THREADS) {
      crow[i] = 0.0f;
      srow[i] = 0.0f;
    }
    return;
  }
  const float* __restrict__ y = wave + s0;
  const int64_t p0 = t * hop - (frame_length >> 1) + 1;
  const bool interior = p0 >= 0 && p0 + need <= n;
  for (int i = tid; i < NX; i += PR_THREADS) xs[i] = i < need ? y[interior ? p0 + i : mf_fold(p0 + i, n)] : 0.0f;
  __syncthreads();
  // ---- d(tau) = sum_{j=1..W} (x[j] - x[j + tau])^2: eight chains (chain u takes j = 1 + u, 9 + u, ..), added as a tree
  for (int tau = 1 + tid; tau <= max_period; tau += PR_THREADS) {
    float acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.0f;
    const float* __restrict__ b = xs + tau;
    for (int j = 0; j < win; j += 8) {
      const float4 a0 = *reinterpret_cast<const float4*>(xs + j);
      const float4 a1 = *reinterpret_cast<const float4*>(xs + j + 4);
      const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float e = __fsub_rn(a[u], b[j + u]);
        acc[u] = __fadd_rn(acc[u], __fmul_rn(e, e));
      }
    }
    d[tau] = __fadd_rn(__fadd_rn(__fadd_rn(acc[0], acc[1]), __fadd_rn(acc[2], acc[3])),
                       __fadd_rn(__fadd_rn(acc[4], acc[5]), __fadd_rn(acc[6], acc[7])));
  }
  __syncthreads();
  // ---- running sums: lane l of wave 0 owns the lags l * chunk + 1 .. (l + 1) * chunk; a chain inside, a scan of the chunk totals over the lanes
  if (tid < MTS_WAVE) {
    const int chunk = (max_period + MTS_WAVE - 1) / MTS_WAVE;
    const int a = tid * chunk + 1, e = min(a + chunk - 1, max_period);
    float run = 0.0f;
    for (int tau = a; tau <= e; ++tau) run = __fadd_rn(run, d[tau]);
    float incl = run;
#pragma unroll
    for (int off = 1; off < MTS_WAVE; off <<= 1) {
      const float o = __shfl_up(incl, off, 64);
      if (tid >= off) incl = __fadd_rn(incl, o);
    }
    float before = __shfl_up(incl, 1, 64);
    if (tid == 0) before = 0.0f;
    run = 0.0f;
    for (int tau = a; tau <= e; ++tau) {
      run = __fadd_rn(run, d[tau]);
      cs[tau] = __fadd_rn(before, run);
    }
  }
  __syncthreads();
  for (int i = tid; i < n_lags; i += PR_THREADS) {
    const int tau = min_period + i;
    const float v = d[tau] / __fadd_rn(cs[tau] / (float)tau, FLT_MIN);
    cm[i] = v;
    crow[i] = v;
  }
  __syncthreads();
  for (int i = tid; i < n_lags; i += PR_THREADS) {
    float sh = 0.0f;
    if (i > 0 && i < n_lags - 1) {
      const float l = cm[i - 1], c = cm[i], r = cm[i + 1];
      const float pa = __fmul_rn(0.5f, __fsub_rn(__fadd_rn(l, r), __fmul_rn(2.0f, c)));
      const float pb = __fmul_rn(0.5f, __fsub_rn(r, l));
      sh = -pb / __fadd_rn(__fmul_rn(2.0f, pa), FLT_MIN);
      if (!(fabsf(sh) <= 1.0f)) sh = 0.0f;
    }
    srow[i] = sh;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------- troughs
// is lag i of c[0 .. L) a trough: below its left neighbour, not above its right one; lag 0: c[0] < c[1]; the last lag: c[L-1] < c[L-2]
__device__ __forceinline__ bool pr_is_trough(const float* c, int i, int L) {
  if (i >= L) return false;
  if (i == 0) return c[0] < c[1];
  return c[i] < c[i - 1] && (i == L - 1 || c[i] <= c[i + 1]);
}

// ---------------------------------------------------------------------------------------------------------------------------- observe
__global__ __launch_bounds__(MTS_WAVE) void pyin_observe_kernel(int n_lags, int min_period, int n_bins, double sr, double fmin,
                                                                double bins_per_octave, const float* __restrict__ cmnd,
                                                                const float* __restrict__ shift, const double* __restrict__ thresholds,
                                                                const double* __restrict__ beta, const double* __restrict__ beta_head,
                                                                int n_thr, const double* __restrict__ boltz_fact,
                                                                const double* __restrict__ boltz_exp, int n_boltz, double no_trough_prob,
                                                                double log_floor, float* __restrict__ voiced_prob,
                                                                double* __restrict__ logobs) {
  extern __shared__ __attribute__((aligned(16))) double po_lds[];
  const int lane = threadIdx.x;
  const int max_t = n_lags / 2 + 1;
  const int n_chunks = (max_t + MTS_WAVE - 1) / MTS_WAVE;
  double* obs = po_lds;                                  // [n_bins]
  double* prob = obs + n_bins;                           // [max_t]
  float* c = reinterpret_cast<float*>(prob + max_t);     // [n_lags]
  int* tl = reinterpret_cast<int*>(c + n_lags);          // [max_t] lag of trough t
  int* tb = tl + max_t;                                  // [max_t] its bin
  int* cnt = tb + max_t;                                 // [n_chunks][n_thr] troughs of the chunk below the threshold
  const int64_t f = blockIdx.x;
  const float* __restrict__ crow = cmnd + f * n_lags;
  const float* __restrict__ srow = shift + f * n_lags;
  for (int i = lane; i < n_lags; i += MTS_WAVE) c[i] = crow[i];
  for (int b = lane; b < n_bins; b += MTS_WAVE) obs[b] = 0.0;
  __syncthreads();
  // ---- the troughs in lag order
  int n_t = 0;
  for (int i0 = 0; i0 < n_lags; i0 += MTS_WAVE) {
    const bool tr = pr_is_trough(c, i0 + lane, n_lags);
    const uint64_t m = __ballot(tr);
    if (tr) tl[n_t + __popcll(m & pr_lanes_below(lane))] = i0 + lane;
    n_t += __popcll(m);
  }
  __syncthreads();
  double vp = 0.0;
  if (n_t > 0) {  // uniform
    const int chunks = (n_t + MTS_WAVE - 1) / MTS_WAVE;
    for (int ch = 0; ch < chunks; ++ch) {
      const int t = ch * MTS_WAVE + lane;
      const double ct = t < n_t ? (double)c[tl[t]] : INFINITY;
      for (int k = 0; k < n_thr; ++k) {
        const uint64_t m = __ballot(ct < thresholds[k]);
        if (lane == 0) cnt[ch * n_thr + k] = __popcll(m);
      }
    }
    __syncthreads();
    // ---- the prior of every trough: sum over the thresholds it is below, ascending, of boltzmann(position, count) * beta
    float best_c = INFINITY;
    int best_t = 0x7fffffff;
    for (int ch = 0; ch < chunks; ++ch) {
      const int t = ch * MTS_WAVE + lane;
      const bool ok = t < n_t;
      const float cf = ok ? c[tl[t]] : INFINITY;
      const double ct = cf;
      double p = 0.0;
      for (int k = 0; k < n_thr; ++k) {
        const bool below = ct < thresholds[k];
        const uint64_t m = __ballot(below);
        int before = 0, total = 0;
        for (int o = 0; o < chunks; ++o) {
          const int v = cnt[o * n_thr + k];
          before += o < ch ? v : 0;
          total += v;
        }
        if (below) {
          const int pos = min(before + __popcll(m & pr_lanes_below(lane)), n_boltz - 1);
          p = p + (boltz_fact[min(total, n_boltz - 1)] * boltz_exp[pos]) * beta[k];
        }
      }
      if (ok) prob[t] = p;
      if (ok && cf < best_c) {  // a lane's troughs come in ascending order: strict keeps the first
        best_c = cf;
        best_t = t;
      }
    }
    // the lowest trough (the first of equals) takes the thresholds nothing is below
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float oc = __shfl_xor(best_c, off, 64);
      const int ot = __shfl_xor(best_t, off, 64);
      if (oc < best_c || (oc == best_c && ot < best_t)) {
        best_c = oc;
        best_t = ot;
      }
    }
    __syncthreads();
    if (lane == 0 && best_t < n_t) {
      int not_below = 0;
      for (int k = 0; k < n_thr; ++k) not_below += !((double)best_c < thresholds[k]);
      prob[best_t] = prob[best_t] + no_trough_prob * beta_head[not_below];
    }
    // ---- bins; on a collision the last trough in lag order wins
    for (int t = lane; t < n_t; t += MTS_WAVE) {
      const int lag = tl[t];
      const double period = (double)(min_period + lag) + (double)srow[lag];
      const double bin = rint(bins_per_octave * log2((sr / period) / fmin));
      tb[t] = bin >= (double)n_bins ? n_bins : (bin > 0.0 ? (int)bin : 0);  // NaN -> 0, as the clip of an undefined cast never is
    }
    __syncthreads();
    for (int t = lane; t < n_t; t += MTS_WAVE) {
      const int b = tb[t];
      bool wins = b < n_bins;  // bin n_bins is the first unvoiced state upstream and is overwritten there: dropped
      for (int o = t + 1; o < n_t && wins; ++o) wins = tb[o] != b;
      if (wins) obs[b] = prob[t];
    }
    __syncthreads();
    for (int b = lane; b < n_bins; b += MTS_WAVE) vp = vp + obs[b];
    vp = pr_wave_sum(vp);
    vp = vp < 0.0 ? 0.0 : (vp > 1.0 ? 1.0 : vp);
  }
  if (lane == 0) voiced_prob[f] = (float)vp;
  double* __restrict__ row = logobs + f * (2 * (int64_t)n_bins);
  const double unvoiced = log((1.0 - vp) / (double)n_bins + DBL_MIN);
  for (int b = lane; b < n_bins; b += MTS_WAVE) {
    const double o = obs[b];
    row[b] = o == 0.0 ? log_floor : log(o + DBL_MIN);
    row[n_bins + b] = unvoiced;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------- viterbi
struct PrBest {
  double v;
  int i;
};
// the larger value, the smaller index among equals
__device__ __forceinline__ PrBest pr_better(PrBest a, PrBest b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

__device__ __forceinline__ PrBest pr_wave_best(PrBest a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    PrBest o;
    o.v = __shfl_xor(a.v, off, 64);
    o.i = __shfl_xor(a.i, off, 64);
    a = pr_better(a, o);
  }
  return a;
}

__global__ __launch_bounds__(PR_MAX_STATES) void pyin_viterbi_kernel(int n_bins, int width, const double* __restrict__ logobs,
                                                                     int64_t total_frames, const int64_t* __restrict__ frame_start,
                                                                     const double* __restrict__ ltri, const double* __restrict__ lsrc,
                                                                     const double* __restrict__ linit, double log_floor,
                                                                     const float* __restrict__ freqs, int16_t* __restrict__ backptr,
                                                                     int32_t* __restrict__ state, float* __restrict__ f0,
                                                                     uint8_t* __restrict__ voiced) {
  extern __shared__ __attribute__((aligned(16))) double pv_lds[];
  __shared__ double red_v[2][PR_MAX_WAVES];
  __shared__ int red_i[2][PR_MAX_WAVES];
  const int S = 2 * n_bins, half = width >> 1;
  double* u = pv_lds;                   // [2][4][n_bins]: u[buf][2 v + v'][j] = value[v n_bins + j] + lsrc[2 v + v'][j]
  double* tri = u + 8 * n_bins;         // [width]
  double* vals = tri + width;           // [S]: the values of a frame, for the dense walk only
  const int tid = threadIdx.x;
  const int n_waves = blockDim.x >> 6;
  const int s = tid, wave = tid >> 6;
  const bool active = s < S;
  const int v = (active && s >= n_bins) ? 1 : 0;
  const int b = active ? s - v * n_bins : 0;
  const int sent = blockIdx.x;
  const int64_t fa = mf_clamp(frame_start[sent], total_frames);
  const int64_t T = mf_clamp(frame_start[sent + 1], total_frames) - fa;
  if (T <= 0) return;  // uniform
  for (int i = tid; i < width; i += blockDim.x) tri[i] = ltri[i];
  const double src0 = active ? lsrc[(2 * v + 0) * n_bins + b] : 0.0;
  const double src1 = active ? lsrc[(2 * v + 1) * n_bins + b] : 0.0;
  const int jlo = max(0, b - half), jhi = min(n_bins - 1, b + half);
  double val = active ? logobs[fa * S + s] + linit[s] : -INFINITY;
  for (int64_t t = 1; t < T; ++t) {
    const int buf = (int)(t & 1);
    const double lo = active ? logobs[(fa + t) * S + s] : 0.0;
    double* ub = u + buf * 4 * n_bins;
    if (active) {
      ub[(2 * v + 0) * n_bins + b] = val + src0;
      ub[(2 * v + 1) * n_bins + b] = val + src1;
    }
    PrBest g = pr_wave_best(PrBest{val, active ? s : 0x7fffffff});
    if ((tid & 63) == 0) {
      red_v[buf][wave] = g.v;
      red_i[buf][wave] = g.i;
    }
    __syncthreads();
    g = PrBest{red_v[buf][0], red_i[buf][0]};
    for (int w = 1; w < n_waves; ++w) g = pr_better(g, PrBest{red_v[buf][w], red_i[buf][w]});
    bool dense = false;
    PrBest best{-INFINITY, 0};
    if (active) {
      // sources in ascending state index, a strict compare: the first of equals stays
      for (int vs = 0; vs < 2; ++vs) {
        const double* __restrict__ us = ub + (2 * vs + v) * n_bins;
        for (int j = jlo; j <= jhi; ++j) {
          const double cand = us[j] + tri[j - b + half];
          if (cand > best.v) best = PrBest{cand, vs * n_bins + j};
        }
      }
      // outside the band upstream's dense matrix holds log(0 + tiny): the best such source is the largest value of all -- unless a
      // rounding makes a smaller one equal, so a frame where the floor reaches the band's best is walked densely
      const int gj = g.i >= n_bins ? g.i - n_bins : g.i;
      dense = (gj < jlo || gj > jhi) && g.v + log_floor >= best.v;
    }
    if (__syncthreads_or(dense)) {  // rare: every thread publishes its value, the threads that need it walk all sources in order
      if (active) vals[s] = val;
      __syncthreads();
      if (dense) {
        best = PrBest{-INFINITY, 0};
        for (int j = 0; j < S; ++j) {
          const int vs = j >= n_bins ? 1 : 0, jb = j - vs * n_bins;
          const double cand = (jb >= jlo && jb <= jhi) ? ub[(2 * vs + v) * n_bins + jb] + tri[jb - b + half] : vals[j] + log_floor;
          if (cand > best.v) best = PrBest{cand, j};
        }
      }
      __syncthreads();
    }
    if (active) {
      val = lo + best.v;
      backptr[(fa + t) * S + s] = (int16_t)best.i;
    }
  }
  // ---- the last state (the first of the best), then the pointers backwards
  PrBest g = pr_wave_best(PrBest{val, active ? s : 0x7fffffff});
  __syncthreads();  // the pointers written above are visible to thread 0; red[0] is free again
  if ((tid & 63) == 0) {
    red_v[0][wave] = g.v;
    red_i[0][wave] = g.i;
  }
  __syncthreads();
  if (tid == 0) {
    g = PrBest{red_v[0][0], red_i[0][0]};
    for (int w = 1; w < n_waves; ++w) g = pr_better(g, PrBest{red_v[0][w], red_i[0][w]});
    int cur = g.i;
    for (int64_t t = T - 1; t >= 0; --t) {
      const bool vo = cur < n_bins;
      state[fa + t] = cur;
      voiced[fa + t] = vo ? 1 : 0;
      f0[fa + t] = vo ? freqs[cur] : __builtin_nanf("");
      if (t > 0) cur = mf_clampi((int)backptr[(fa + t) * S + cur], 0, S - 1);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------- yin pick
__global__ __launch_bounds__(MTS_WAVE) void yin_pick_kernel(int n_lags, int min_period, float sr, float threshold,
                                                            const float* __restrict__ cmnd, const float* __restrict__ shift,
                                                            float* __restrict__ f0) {
  extern __shared__ __attribute__((aligned(16))) float yp_lds[];
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  const float* __restrict__ crow = cmnd + f * n_lags;
  for (int i = lane; i < n_lags; i += MTS_WAVE) yp_lds[i] = crow[i];
  __syncthreads();
  int pick = -1;
  float best_c = INFINITY;
  int best_i = 0x7fffffff;
  for (int i0 = 0; i0 < n_lags; i0 += MTS_WAVE) {
    const int i = i0 + lane;
    const float ci = i < n_lags ? yp_lds[i] : INFINITY;
    if (i < n_lags && ci < best_c) {
      best_c = ci;
      best_i = i;
    }
    const uint64_t m = __ballot(pr_is_trough(yp_lds, i, n_lags) && ci < threshold);
    if (pick < 0 && m) pick = i0 + __builtin_ctzll(m);
  }
  if (pick < 0) {  // no trough below the threshold: the global minimum, the first of equals
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float oc = __shfl_xor(best_c, off, 64);
      const int oi = __shfl_xor(best_i, off, 64);
      if (oc < best_c || (oc == best_c && oi < best_i)) {
        best_c = oc;
        best_i = oi;
      }
    }
    pick = mf_clampi(best_i, 0, n_lags - 1);  // a row of NaN has no minimum: lag 0, as np.argmin gives
  }
  if (lane == 0) f0[f] = sr / __fadd_rn((float)(min_period + pick), shift[f * n_lags + pick]);
}

// ---------------------------------------------------------------------------------------------------------------------------- delta
__global__ __launch_bounds__(PR_THREADS) void frame_delta_kernel(const float* __restrict__ x, int64_t total_frames,
                                                                 const int64_t* __restrict__ frame_start, int n_sent, int D,
                                                                 float* __restrict__ out) {
  __shared__ int64_t sent_f0[PR_FB], sent_T[PR_FB];
  const int tid = threadIdx.x;
  const int64_t fa = (int64_t)blockIdx.x * PR_FB;
  const int nf = (int)min((int64_t)PR_FB, total_frames - fa);
  if (tid < nf) {
    const int s = mf_sentence_of(frame_start, n_sent, fa + tid);
    const int64_t f0 = mf_clamp(frame_start[s], total_frames);
    sent_f0[tid] = f0;
    sent_T[tid] = mf_clamp(frame_start[s + 1], total_frames) - f0;
  }
  __syncthreads();
  for (int o = tid; o < nf * D; o += PR_THREADS) {
    const int fr = o / D, c = o - fr * D;
    const int64_t T = sent_T[fr], t = fa + fr - sent_f0[fr];
    float delta = 0.0f;
    if (T >= 9 && t >= 0 && t < T) {
      const int64_t tc = t < 4 ? 4 : (t > T - 5 ? T - 5 : t);
      const float* __restrict__ p = x + (sent_f0[fr] + tc) * D + c;
      float acc = 0.0f;
#pragma unroll
      for (int k = 1; k <= 4; ++k) acc = __fadd_rn(acc, __fmul_rn((float)k, __fsub_rn(p[(int64_t)k * D], p[-(int64_t)k * D])));
      delta = acc / 60.0f;
    }
    out[fa * D + o] = delta;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------- statistics
// One pass over a sentence's voicing probabilities: what a closed pause (a run below 0.5 that a voiced frame ends) contributes.
// mode 0: -> the number of closed pauses and the sum of their lengths; mode 1: -> the sum of (length - mean)^2.
__device__ __forceinline__ void pr_pauses(const float* __restrict__ vp, int64_t T, int lane, int mode, double mean, int& n_closed,
                                          int& len_sum, double& dev_sum) {
  int64_t carry = -1;  // the last voiced frame before the chunk
  int cnt = 0, sum = 0;
  double dev = 0.0;
  for (int64_t c0 = 0; c0 < T; c0 += MTS_WAVE) {
    const int64_t t = c0 + lane;
    const bool voi = t < T && !(vp[t] < 0.5f);
    const uint64_t m = __ballot(voi);
    if (voi && t > 0 && vp[t - 1] < 0.5f) {
      const uint64_t lower = m & pr_lanes_below(lane);
      const int64_t prev = lower ? c0 + 63 - __builtin_clzll(lower) : carry;
      const int len = (int)(t - prev - 1);
      cnt += 1;
      sum += len;
      if (mode) {
        const double e = (double)len - mean;
        dev = dev + e * e;
      }
    }
    if (m) carry = c0 + 63 - __builtin_clzll(m);
  }
  n_closed = pr_wave_sum(cnt);
  len_sum = pr_wave_sum(sum);
  dev_sum = pr_wave_sum(dev);
}

// mean over the non-NaN x[a .. b) / scale, NaN when there is none
__device__ __forceinline__ double pr_ratio_mean(const float* __restrict__ x, int64_t a, int64_t b, double scale, int lane) {
  double sum = 0.0;
  int cnt = 0;
  for (int64_t t = a + lane; t < b; t += MTS_WAVE) {
    const double r = (double)x[t] / scale;
    if (r == r) {
      sum = sum + r;
      cnt += 1;
    }
  }
  sum = pr_wave_sum(sum);
  cnt = pr_wave_sum(cnt);
  return cnt ? sum / (double)cnt : (double)__builtin_nanf("");
}

// (count, sum) and then the squared deviations of the non-NaN x[a .. b)
__device__ __forceinline__ void pr_moments(const float* __restrict__ x, int64_t a, int64_t b, int lane, int& count, double& mean,
                                           double& dev) {
  double sum = 0.0;
  int cnt = 0;
  for (int64_t t = a + lane; t < b; t += MTS_WAVE) {
    const double v = x[t];
    if (v == v) {
      sum = sum + v;
      cnt += 1;
    }
  }
  sum = pr_wave_sum(sum);
  count = pr_wave_sum(cnt);
  mean = count ? sum / (double)count : (double)__builtin_nanf("");
  double sq = 0.0;
  for (int64_t t = a + lane; t < b; t += MTS_WAVE) {
    const double v = x[t];
    if (v == v) {
      const double e = v - mean;
      sq = sq + e * e;
    }
  }
  dev = pr_wave_sum(sq);
}

__global__ __launch_bounds__(MTS_WAVE) void prosodic_stats_kernel(const float* __restrict__ f0, const float* __restrict__ vp,
                                                                  const float* __restrict__ prev_f0, int64_t total_frames,
                                                                  const int64_t* __restrict__ frame_start,
                                                                  const uint8_t* __restrict__ doc_first, void* __restrict__ out,
                                                                  int out_dtype, int64_t ld_out, int jump_col) {
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  const int64_t fa = mf_clamp(frame_start[s], total_frames);
  const int64_t T = mf_clamp(frame_start[s + 1], total_frames) - fa;
  double col[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (T > 0) {  // uniform
    const float* __restrict__ p = vp + fa;
    // ---- f0 over the voiced frames; none: 0 and 0
    int nv;
    double f_mean, f_dev;
    pr_moments(f0, fa, fa + T, lane, nv, f_mean, f_dev);
    if (nv) {
      col[0] = f_mean;
      col[1] = sqrt(f_dev / (double)nv);
    }
    // ---- pauses
    int n_closed, len_sum;
    double dev;
    pr_pauses(p, T, lane, 0, 0.0, n_closed, len_sum, dev);
    int low = 0;
    double v_sum = 0.0;
    for (int64_t t = lane; t < T; t += MTS_WAVE) {
      if (p[t] < 0.5f)
        low += 1;
      else
        v_sum = v_sum + (double)p[t];
    }
    low = pr_wave_sum(low);
    v_sum = pr_wave_sum(v_sum);
    if (n_closed) {
      const double m = (double)len_sum / (double)n_closed;
      pr_pauses(p, T, lane, 1, m, n_closed, len_sum, dev);
      col[2] = m;
      col[3] = sqrt(dev / (double)n_closed);
    } else {
      col[2] = (double)low;  // the one unclosed run, or [0]
    }
    // ---- voiced intensities; without a closed pause but with pause frames upstream appends a 0
    const int extra = (!n_closed && low) ? 1 : 0;
    const int n_v = (int)(T - low) + extra;
    const double v_mean = v_sum / (double)n_v;
    double v_dev = 0.0;
    for (int64_t t = lane; t < T; t += MTS_WAVE) {
      if (!(p[t] < 0.5f)) {
        const double e = (double)p[t] - v_mean;
        v_dev = v_dev + e * e;
      }
    }
    v_dev = pr_wave_sum(v_dev);
    if (extra) v_dev = v_dev + v_mean * v_mean;
    col[4] = v_mean;
    col[5] = sqrt(v_dev / (double)n_v);
    // ---- the pitch jump against the previous sentence of the document
    if (s > 0 && !doc_first[s]) {
      const int64_t pa = mf_clamp(frame_start[s - 1], total_frames);
      const int64_t Tp = fa - pa;
      if (Tp > 0) {
        // no voiced frame: upstream has replaced the NaN track by zeros, 0 / 0 is NaN and the jump 0
        const double head = nv ? pr_ratio_mean(f0, fa, fa + T / 5, f_mean, lane) : (double)__builtin_nanf("");
        int np_;
        double p_mean, p_dev;
        pr_moments(prev_f0, pa, pa + Tp, lane, np_, p_mean, p_dev);
        const double tail = pr_ratio_mean(prev_f0, pa + Tp - (Tp + 4) / 5, pa + Tp, p_mean, lane);
        const double jump = head - tail;
        col[6] = jump == jump ? jump : 0.0;
      }
    }
  }
  if (lane < 7) {
    double v = col[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) v = lane == k ? col[k] : v;
    mf_store(out, out_dtype, (int64_t)s * ld_out + (lane < 6 ? lane : jump_col), (float)v);
  }
}

}  // namespace

extern "C" int mts_yin_frames(void* stream, int n_sent, int frame_length, int win_length, int hop, int min_period, int max_period,
                              const float* wave, int64_t total_samples, const int64_t* sent_start, const int64_t* sent_len,
                              const int64_t* frame_start, int64_t total_frames, float* cmnd, float* shift) {
  MTS_CHECK_ARG(wave && sent_start && sent_len && frame_start && cmnd && shift, "mts_yin_frames: null pointer");
  MTS_CHECK_ARG(n_sent >= 1 && total_samples >= 1 && total_frames >= 1 && hop >= 1,
                "mts_yin_frames: bad shape (n_sent %d, total_samples %lld, total_frames %lld, hop %d)", n_sent, (long long)total_samples,
                (long long)total_frames, hop);
  MTS_CHECK_ARG(frame_length >= 16 && frame_length <= PR_MAX_FRAME && frame_length % 2 == 0 && win_length >= 8 && win_length % 8 == 0,
                "mts_yin_frames: frame_length must be even in 16 .. %d and win_length a positive multiple of 8 (got %d, %d)", PR_MAX_FRAME,
                frame_length, win_length);
  MTS_CHECK_ARG(min_period >= 1 && max_period >= min_period + 2 && max_period <= frame_length - win_length - 1,
                "mts_yin_frames: periods must satisfy 1 <= min_period, min_period + 2 <= max_period <= frame_length - win_length - 1 (got %d, %d)",
                min_period, max_period);
  MTS_CHECK_ARG(aligned_to(wave, 4) && aligned_to(cmnd, 4) && aligned_to(shift, 4), "mts_yin_frames: wave / cmnd / shift not aligned");
  MTS_UNSUPPORTED(total_frames <= 0x7fffffffLL, "mts_yin_frames: %lld frames are more than one launch covers", (long long)total_frames);
  const int n_lags = max_period - min_period + 1;
  const size_t lds = ((size_t)((win_length + max_period + 3) & ~3) + 2 * (size_t)(max_period + 1) + n_lags) * sizeof(float);
  hipLaunchKernelGGL(yin_frames_kernel, dim3((unsigned)total_frames), dim3(PR_THREADS), lds, (hipStream_t)stream, wave, total_samples,
                     sent_start, sent_len, frame_start, total_frames, n_sent, frame_length, win_length, hop, min_period, max_period, cmnd,
                     shift);
  MTS_LAUNCH_CHECK("mts_yin_frames");
  return MTS_OK;
}

extern "C" int mts_pyin_observe(void* stream, int64_t total_frames, int n_lags, int min_period, int n_bins, double sr, double fmin,
                                double bins_per_octave, const float* cmnd, const float* shift, const double* thresholds, const double* beta,
                                const double* beta_head, int n_thresholds, const double* boltz_fact, const double* boltz_exp, int n_boltz,
                                double no_trough_prob, double log_floor, float* voiced_prob, double* logobs) {
  MTS_CHECK_ARG(cmnd && shift && thresholds && beta && beta_head && boltz_fact && boltz_exp && voiced_prob && logobs,
                "mts_pyin_observe: null pointer");
  MTS_CHECK_ARG(total_frames >= 1 && n_lags >= 3 && min_period >= 1 && n_bins >= 1 && n_thresholds >= 1,
                "mts_pyin_observe: bad shape (total_frames %lld, n_lags %d, min_period %d, n_bins %d, n_thresholds %d)", (long long)total_frames,
                n_lags, min_period, n_bins, n_thresholds);
  MTS_CHECK_ARG(n_boltz >= n_lags / 2 + 2, "mts_pyin_observe: the Boltzmann tables hold %d entries, %d lags can have %d troughs", n_boltz, n_lags,
                n_lags / 2 + 1);
  MTS_CHECK_ARG(sr > 0.0 && fmin > 0.0 && bins_per_octave > 0.0 && no_trough_prob >= 0.0 && log_floor < 0.0,
                "mts_pyin_observe: sr, fmin and bins_per_octave must be positive, no_trough_prob >= 0 and log_floor < 0");
  MTS_CHECK_ARG(aligned_to(cmnd, 4) && aligned_to(shift, 4) && aligned_to(voiced_prob, 4) && aligned_to(logobs, 8) && aligned_to(thresholds, 8) &&
                    aligned_to(beta, 8) && aligned_to(beta_head, 8) && aligned_to(boltz_fact, 8) && aligned_to(boltz_exp, 8),
                "mts_pyin_observe: a pointer is not aligned to its element size");
  MTS_UNSUPPORTED(total_frames <= 0x7fffffffLL, "mts_pyin_observe: %lld frames are more than one launch covers", (long long)total_frames);
  const int max_t = n_lags / 2 + 1;
  const size_t lds = ((size_t)n_bins + max_t) * sizeof(double) + (size_t)n_lags * sizeof(float) +
                     ((size_t)2 * max_t + (size_t)ceil_div(max_t, MTS_WAVE) * n_thresholds) * sizeof(int);
  MTS_UNSUPPORTED(lds <= 64 * 1024, "mts_pyin_observe: %d lags, %d bins and %d thresholds do not fit a workgroup's 64 KiB of LDS", n_lags, n_bins,
                  n_thresholds);
  hipLaunchKernelGGL(pyin_observe_kernel, dim3((unsigned)total_frames), dim3(MTS_WAVE), lds, (hipStream_t)stream, n_lags, min_period, n_bins, sr,
                     fmin, bins_per_octave, cmnd, shift, thresholds, beta, beta_head, n_thresholds, boltz_fact, boltz_exp, n_boltz,
                     no_trough_prob, log_floor, voiced_prob, logobs);
  MTS_LAUNCH_CHECK("mts_pyin_observe");
  return MTS_OK;
}

extern "C" int mts_pyin_viterbi(void* stream, int n_sent, int n_bins, int width, const double* logobs, int64_t total_frames,
                                const int64_t* frame_start, const double* ltri, const double* lsrc, const double* linit, double log_floor,
                                const float* freqs, int16_t* backptr, int32_t* state, float* f0, uint8_t* voiced) {
  MTS_CHECK_ARG(logobs && frame_start && ltri && lsrc && linit && freqs && backptr && state && f0 && voiced, "mts_pyin_viterbi: null pointer");
  MTS_CHECK_ARG(n_sent >= 1 && n_bins >= 1 && total_frames >= 1 && width >= 1 && width % 2 == 1,
                "mts_pyin_viterbi: bad shape (n_sent %d, n_bins %d, total_frames %lld, width %d: odd and positive)", n_sent, n_bins,
                (long long)total_frames, width);
  MTS_CHECK_ARG(log_floor < 0.0, "mts_pyin_viterbi: log_floor must be negative");
  MTS_CHECK_ARG(aligned_to(logobs, 8) && aligned_to(ltri, 8) && aligned_to(lsrc, 8) && aligned_to(linit, 8) && aligned_to(freqs, 4) &&
                    aligned_to(backptr, 2) && aligned_to(state, 4) && aligned_to(f0, 4),
                "mts_pyin_viterbi: a pointer is not aligned to its element size");
  MTS_UNSUPPORTED(2 * n_bins <= PR_MAX_STATES, "mts_pyin_viterbi: %d states are more than the %d a workgroup holds", 2 * n_bins, PR_MAX_STATES);
  const size_t lds = ((size_t)10 * n_bins + width) * sizeof(double);
  MTS_UNSUPPORTED(lds <= 64 * 1024, "mts_pyin_viterbi: %d bins and a band of %d do not fit a workgroup's 64 KiB of LDS", n_bins, width);
  const unsigned threads = (unsigned)align_up((size_t)2 * n_bins, MTS_WAVE);
  hipLaunchKernelGGL(pyin_viterbi_kernel, dim3((unsigned)n_sent), dim3(threads), lds, (hipStream_t)stream, n_bins, width, logobs, total_frames,
                     frame_start, ltri, lsrc, linit, log_floor, freqs, backptr, state, f0, voiced);
  MTS_LAUNCH_CHECK("mts_pyin_viterbi");
  return MTS_OK;
}

extern "C" int mts_yin_pick(void* stream, int64_t total_frames, int n_lags, int min_period, float sr, float trough_threshold,
                            const float* cmnd, const float* shift, float* f0) {
  MTS_CHECK_ARG(cmnd && shift && f0, "mts_yin_pick: null pointer");
  MTS_CHECK_ARG(total_frames >= 1 && n_lags >= 3 && n_lags <= PR_MAX_FRAME && min_period >= 1 && sr > 0.0f,
                "mts_yin_pick: bad shape (total_frames %lld, n_lags %d, min_period %d, sr %g)", (long long)total_frames, n_lags, min_period,
                (double)sr);
  MTS_CHECK_ARG(aligned_to(cmnd, 4) && aligned_to(shift, 4) && aligned_to(f0, 4), "mts_yin_pick: a pointer is not aligned to its element size");
  MTS_UNSUPPORTED(total_frames <= 0x7fffffffLL, "mts_yin_pick: %lld frames are more than one launch covers", (long long)total_frames);
  hipLaunchKernelGGL(yin_pick_kernel, dim3((unsigned)total_frames), dim3(MTS_WAVE), (size_t)n_lags * sizeof(float), (hipStream_t)stream, n_lags,
                     min_period, sr, trough_threshold, cmnd, shift, f0);
  MTS_LAUNCH_CHECK("mts_yin_pick");
  return MTS_OK;
}

extern "C" int mts_frame_delta(void* stream, int n_sent, int D, const float* x, int64_t total_frames, const int64_t* frame_start,
                               float* out) {
  MTS_CHECK_ARG(x && frame_start && out, "mts_frame_delta: null pointer");
  MTS_CHECK_ARG(n_sent >= 1 && D >= 1 && total_frames >= 1, "mts_frame_delta: bad shape (n_sent %d, D %d, total_frames %lld)", n_sent, D,
                (long long)total_frames);
  MTS_CHECK_ARG(aligned_to(x, 4) && aligned_to(out, 4), "mts_frame_delta: x / out not aligned to their element size");
  const int64_t groups = (total_frames + PR_FB - 1) / PR_FB;
  MTS_UNSUPPORTED(groups <= 0x7fffffffLL, "mts_frame_delta: %lld frames are more than one launch covers", (long long)total_frames);
  hipLaunchKernelGGL(frame_delta_kernel, dim3((unsigned)groups), dim3(PR_THREADS), 0, (hipStream_t)stream, x, total_frames, frame_start, n_sent,
                     D, out);
  MTS_LAUNCH_CHECK("mts_frame_delta");
  return MTS_OK;
}

extern "C" int mts_prosodic_stats(void* stream, int out_dtype, int n_sent, const float* f0, const float* voiced_prob, const float* prev_f0,
                                  int64_t total_frames, const int64_t* frame_start, const uint8_t* doc_first, void* out, int64_t ld_out,
                                  int jump_col) {
  MTS_CHECK_ARG(out_dtype == MTS_F32 || out_dtype == MTS_BF16, "mts_prosodic_stats: out_dtype must be fp32 or bf16 (got %d)", out_dtype);
  MTS_CHECK_ARG(f0 && voiced_prob && prev_f0 && frame_start && doc_first && out, "mts_prosodic_stats: null pointer");
  MTS_CHECK_ARG(n_sent >= 1 && total_frames >= 1, "mts_prosodic_stats: bad shape (n_sent %d, total_frames %lld)", n_sent, (long long)total_frames);
  MTS_CHECK_ARG(jump_col >= 6 && ld_out > jump_col, "mts_prosodic_stats: jump_col %d must lie behind the six scalar columns and inside ld_out %lld",
                jump_col, (long long)ld_out);
  MTS_CHECK_ARG(aligned_to(f0, 4) && aligned_to(voiced_prob, 4) && aligned_to(prev_f0, 4) && aligned_to(out, out_dtype == MTS_F32 ? 4 : 2),
                "mts_prosodic_stats: a pointer is not aligned to its element size");
  hipLaunchKernelGGL(prosodic_stats_kernel, dim3((unsigned)n_sent), dim3(MTS_WAVE), 0, (hipStream_t)stream, f0, voiced_prob, prev_f0, total_frames,
                     frame_start, doc_first, out, out_dtype, ld_out, jump_col);
  MTS_LAUNCH_CHECK("mts_prosodic_stats");
  return MTS_OK;
}
