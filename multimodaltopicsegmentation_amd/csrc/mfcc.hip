// MFCC + delta frames from resident waveforms (audio.ResidentAudio.mfcc; reference: extract_acoustic_features.py:58-72, the `mfcc` encoder:
// per sentence librosa.feature.mfcc(y, sr, n_mfcc=50), its librosa.feature.delta, then mean and std over the frames of both).  The waveform
// of a whole corpus lies in HBM as one fp32 vector; sentence s is the samples sent_start[s] .. sent_start[s] + sent_len[s] and owns the
// frames frame_start[s] .. frame_start[s + 1] of the outputs.  The definition restated (librosa 0.8.1 at the reference's arguments; every
// number below is a parameter of the ABI or a table the host builds in fp64 and rounds once to fp32):
//   frame t   samples t * hop - n_fft / 2 .. t * hop + n_fft / 2 - 1 of the sentence, an index outside 0 .. n - 1 reflected about the
//             sentence's OWN ends without repeating the end sample (np.pad(y, n_fft / 2, 'reflect'): the fold of period 2 (n - 1); n == 1
//             is constant) -- the neighbouring audio is never read;
//   power     P[k] = |rfft(window . frame)[k]|^2,  k = 0 .. n_fft / 2;
//   mel       M[m] = sum_j w[m][j] P[first[m] + j]: the filter's own bins in ascending order (filter-major, no scatter);
//   dB        d = 10 log10(max(1e-10, M)), then max(d, top - 80) with top the dB of the sentence's largest mel power;
//   MFCC      c[i] = sum_m dct[i][m] d[m];
//   delta     the Savitzky-Golay slope of width 9: D[t] = sum_{k=1..4} k (c[t + k] - c[t - k]) / 60 for 4 <= t <= T - 5, D[0..3] = D[4],
//             D[T-4..T-1] = D[T-5]; 0 for a sentence of fewer than 9 frames (where librosa raises).
//
// mts_mel_frames: one workgroup of 256 threads per frame.  The n_fft real samples are packed as an N = n_fft / 2 point complex sequence
// z[i] = x[2 i] + i x[2 i + 1], transformed in LDS by a Stockham autosort schedule (radix-4 passes, one radix-2 pass last when log2 N is
// odd: no bit reversal, every pass reads one buffer and writes the other), finished by the real-split pass that gives P, and the mel sums
// read P from LDS.  LDS holds re and im apart (so a butterfly's four points are four conflict-free dword accesses) and element i sits at
// i + (i >> 5): the pad breaks the power-of-two strides of the passes' scattered stores.  Twiddles come from the host's table tw[m] =
// exp(-2 pi i m / n_fft), m < n_fft (16 KiB at 2048: L1 / L2 serve it); no sine or cosine is evaluated on the device.  Samples are read from
// global memory through the fold; consecutive frames overlap by 1 - hop / n_fft and L2 serves that.
//
// mts_mfcc_frames: three launches on the caller's stream, the workspace between them.  (1) one workgroup per sentence takes the maximum
// of its mel powers (exact, whatever the order) and stores its dB as the sentence's top; (2) one workgroup per 16 frames forms the clamped
// dB rows and the DCT -- the table transposed in LDS so that consecutive lanes (consecutive coefficients) read consecutive banks -- into
// the fp32 MFCC workspace; (3) one workgroup per 16 frames writes the output block: the MFCC, and the delta from the fp32 MFCC of up to
// four frames on either side INSIDE the sentence.  A bf16 output is one rounding of the fp32 value: the delta never sees a rounded MFCC.
// No atomics, no workgroup depends on another inside a launch, every element of the block written exactly once, nothing outside it touched.
//
// The arithmetic and the order of every sum: include/mts.h.
#include "frame_common.h"

namespace {

constexpr int MF_THREADS = 256;
constexpr int MF_FB = 16;          // frames per workgroup of the DCT and the delta launches
constexpr int MF_MIN_FFT = 64, MF_MAX_FFT = 4096;

__device__ __forceinline__ int mf_pad(int i) { return i + (i >> 5); }
// (a + i b) (c + i d), four products and two sums, each rounded
__device__ __forceinline__ void mf_cmul(float& a, float& b, float2 w) {
  const float r = __fsub_rn(__fmul_rn(a, w.x), __fmul_rn(b, w.y));
  const float i = __fadd_rn(__fmul_rn(a, w.y), __fmul_rn(b, w.x));
  a = r;
  b = i;
}

__device__ __forceinline__ float mf_db(float power) { return __fmul_rn(10.0f, log10f(fmaxf(1e-10f, power))); }

__global__ __launch_bounds__(MF_THREADS) void mel_frames_kernel(const float* __restrict__ wave, int64_t total_samples,
                                                                const int64_t* __restrict__ sent_start, const int64_t* __restrict__ sent_len,
                                                                const int64_t* __restrict__ frame_start, int64_t total_frames, int n_sent,
                                                                int n_fft, int hop, int n_mels, const float* __restrict__ window,
                                                                const float2* __restrict__ tw, const int32_t* __restrict__ mel_first,
                                                                const int32_t* __restrict__ mel_ptr, const float* __restrict__ mel_w, int mel_nnz,
                                                                float* __restrict__ mel) {
  extern __shared__ float mf_lds[];
  const int tid = threadIdx.x;
  const int N = n_fft >> 1;
  const int NP = N + (N >> 5) + 1;
  float* sr = mf_lds;
  float* si = mf_lds + NP;
  float* dr = mf_lds + 2 * NP;
  float* di = mf_lds + 3 * NP;

  const int64_t f = blockIdx.x;
  const int s = mf_sentence_of(frame_start, n_sent, f);
  const int64_t t = f - mf_clamp(frame_start[s], total_frames);
  const int64_t s0 = mf_clamp(sent_start[s], total_samples);
  const int64_t n = mf_clamp(sent_len[s], total_samples - s0);
  float* __restrict__ row = mel + f * n_mels;
  if (n <= 0) {  // uniform over the workgroup: a sentence without samples has no spectrum
    for (int m = tid; m < n_mels; m += MF_THREADS) row[m] = 0.0f;
    return;
  }
  // ---- the windowed frame, packed: z[i] = x[2 i] + i x[2 i + 1]
  const float* __restrict__ y = wave + s0;
  const int64_t p0 = t * hop - N;
  const bool interior = p0 >= 0 && p0 + n_fft <= n;
  for (int i = tid; i < N; i += MF_THREADS) {
    const int64_t pa = p0 + 2 * i;
    const int64_t ia = interior ? pa : mf_fold(pa, n);
    const int64_t ib = interior ? pa + 1 : mf_fold(pa + 1, n);
    sr[mf_pad(i)] = __fmul_rn(y[ia], window[2 * i]);
    si[mf_pad(i)] = __fmul_rn(y[ib], window[2 * i + 1]);
  }
  __syncthreads();
  // ---- Stockham passes: radix 4 while four sub-transforms of length Ns fit, then one radix-2 pass when log2 N is odd
  int Ns = 1;
  const int q = N >> 2;
  for (; Ns * 4 <= N; Ns *= 4) {
    const int tstep = n_fft / (Ns * 4);  // tw index of exp(-2 pi i / (4 Ns))
    for (int j = tid; j < q; j += MF_THREADS) {
      const int k = j & (Ns - 1);
      float ar = sr[mf_pad(j)], ai = si[mf_pad(j)];
      float br = sr[mf_pad(j + q)], bi = si[mf_pad(j + q)];
      float cr = sr[mf_pad(j + 2 * q)], ci = si[mf_pad(j + 2 * q)];
      float er = sr[mf_pad(j + 3 * q)], ei = si[mf_pad(j + 3 * q)];
      if (Ns > 1) {  // the first pass' twiddles are all 1
        mf_cmul(br, bi, tw[k * tstep]);
        mf_cmul(cr, ci, tw[2 * k * tstep]);
        mf_cmul(er, ei, tw[3 * k * tstep]);
      }
      const float a0r = __fadd_rn(ar, cr), a0i = __fadd_rn(ai, ci);
      const float a1r = __fsub_rn(ar, cr), a1i = __fsub_rn(ai, ci);
      const float a2r = __fadd_rn(br, er), a2i = __fadd_rn(bi, ei);
      const float a3r = __fsub_rn(bi, ei), a3i = __fsub_rn(er, br);  // -i (b - e)
      const int j0 = ((j - k) << 2) + k;
      dr[mf_pad(j0)] = __fadd_rn(a0r, a2r);
      di[mf_pad(j0)] = __fadd_rn(a0i, a2i);
      dr[mf_pad(j0 + Ns)] = __fadd_rn(a1r, a3r);
      di[mf_pad(j0 + Ns)] = __fadd_rn(a1i, a3i);
      dr[mf_pad(j0 + 2 * Ns)] = __fsub_rn(a0r, a2r);
      di[mf_pad(j0 + 2 * Ns)] = __fsub_rn(a0i, a2i);
      dr[mf_pad(j0 + 3 * Ns)] = __fsub_rn(a1r, a3r);
      di[mf_pad(j0 + 3 * Ns)] = __fsub_rn(a1i, a3i);
    }
    __syncthreads();
    float* x = sr; sr = dr; dr = x;
    x = si; si = di; di = x;
  }
  if (Ns < N) {  // Ns == N / 2: out[j] = a + w b, out[j + N / 2] = a - w b, w = exp(-2 pi i j / N) = tw[2 j]
    const int h = N >> 1;
    for (int j = tid; j < h; j += MF_THREADS) {
      const float ar = sr[mf_pad(j)], ai = si[mf_pad(j)];
      float br = sr[mf_pad(j + h)], bi = si[mf_pad(j + h)];
      mf_cmul(br, bi, tw[2 * j]);
      dr[mf_pad(j)] = __fadd_rn(ar, br);
      di[mf_pad(j)] = __fadd_rn(ai, bi);
      dr[mf_pad(j + h)] = __fsub_rn(ar, br);
      di[mf_pad(j + h)] = __fsub_rn(ai, bi);
    }
    __syncthreads();
    float* x = sr; sr = dr; dr = x;
    x = si; si = di; di = x;
  }
  // ---- real split: X[k] = E + exp(-2 pi i k / n_fft) O,  E = (Z[k] + conj Z[N - k]) / 2,  O = -i (Z[k] - conj Z[N - k]) / 2;  P = |X|^2.
  // P (N + 1 floats) goes to the buffer the last pass read: dr and di are one contiguous run of 2 NP floats.
  float* P = dr < di ? dr : di;
  for (int k = tid; k <= N; k += MF_THREADS) {
    const int ka = k & (N - 1), kb = (N - k) & (N - 1);
    const float zr = sr[mf_pad(ka)], zi = si[mf_pad(ka)];
    const float nr = sr[mf_pad(kb)], ni = -si[mf_pad(kb)];
    const float Er = __fmul_rn(0.5f, __fadd_rn(zr, nr)), Ei = __fmul_rn(0.5f, __fadd_rn(zi, ni));
    float Or = __fmul_rn(0.5f, __fsub_rn(zi, ni)), Oi = __fmul_rn(-0.5f, __fsub_rn(zr, nr));
    mf_cmul(Or, Oi, tw[k]);
    const float Xr = __fadd_rn(Er, Or), Xi = __fadd_rn(Ei, Oi);
    P[k] = __fadd_rn(__fmul_rn(Xr, Xr), __fmul_rn(Xi, Xi));
  }
  __syncthreads();
  // ---- mel: filter m adds its own bins in ascending order; table entries are clamped before an address is formed
  for (int m = tid; m < n_mels; m += MF_THREADS) {
    const int a = mf_clampi(mel_ptr[m], 0, mel_nnz);
    const int b = mf_clampi(mel_ptr[m + 1], a, mel_nnz);
    const int first = mf_clampi(mel_first[m], 0, N);
    const int cnt = min(b - a, N + 1 - first);
    float acc = 0.0f;
    for (int j = 0; j < cnt; ++j) acc = __fadd_rn(acc, __fmul_rn(mel_w[a + j], P[first + j]));
    row[m] = acc;
  }
}

// (1) top[s] = the dB of the sentence's largest mel power
__global__ __launch_bounds__(MF_THREADS) void mfcc_top_kernel(const float* __restrict__ mel, int64_t total_frames,
                                                              const int64_t* __restrict__ frame_start, int n_mels, float* __restrict__ top) {
  __shared__ float part[MF_THREADS / MTS_WAVE];
  const int s = blockIdx.x;
  const int64_t f0 = mf_clamp(frame_start[s], total_frames);
  const int64_t f1 = mf_clamp(frame_start[s + 1], total_frames);
  const int64_t cnt = f1 > f0 ? (f1 - f0) * n_mels : 0;
  const float* __restrict__ base = mel + f0 * n_mels;
  float m = 0.0f;  // powers are >= 0 and the floor is above 0
  for (int64_t i = threadIdx.x; i < cnt; i += MF_THREADS) m = fmaxf(m, base[i]);
  m = wave_max(m);
  if ((threadIdx.x & (MTS_WAVE - 1)) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < MF_THREADS / MTS_WAVE; ++w) m = fmaxf(m, part[w]);
    top[s] = mf_db(m);
  }
}

// (2) the clamped dB rows and the DCT of MF_FB frames -> the fp32 MFCC workspace [total_frames, n_mfcc]
__global__ __launch_bounds__(MF_THREADS) void mfcc_dct_kernel(const float* __restrict__ mel, int64_t total_frames,
                                                              const int64_t* __restrict__ frame_start, int n_sent, int n_mels, int n_mfcc,
                                                              const float* __restrict__ dct, const float* __restrict__ top,
                                                              float* __restrict__ mfcc) {
  extern __shared__ float mf_lds[];
  float* dctT = mf_lds;                           // [n_mels][n_mfcc]
  float* db = dctT + n_mels * n_mfcc;             // [MF_FB][n_mels + 1]
  float* floor_db = db + MF_FB * (n_mels + 1);    // [MF_FB]
  const int tid = threadIdx.x;
  const int64_t fa = (int64_t)blockIdx.x * MF_FB;
  const int nf = (int)min((int64_t)MF_FB, total_frames - fa);
  for (int i = tid; i < n_mfcc * n_mels; i += MF_THREADS) {
    const int c = i / n_mels, m = i - c * n_mels;
    dctT[m * n_mfcc + c] = dct[i];
  }
  if (tid < nf) floor_db[tid] = __fsub_rn(top[mf_sentence_of(frame_start, n_sent, fa + tid)], 80.0f);
  __syncthreads();
  for (int i = tid; i < nf * n_mels; i += MF_THREADS) {
    const int fr = i / n_mels, m = i - fr * n_mels;
    db[fr * (n_mels + 1) + m] = fmaxf(mf_db(mel[fa * n_mels + i]), floor_db[fr]);
  }
  __syncthreads();
  for (int o = tid; o < nf * n_mfcc; o += MF_THREADS) {
    const int fr = o / n_mfcc, c = o - fr * n_mfcc;
    const float* __restrict__ d = db + fr * (n_mels + 1);
    float acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.0f;
    int m = 0;
    for (; m + 8 <= n_mels; m += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = fmaf(d[m + u], dctT[(m + u) * n_mfcc + c], acc[u]);
    }
    for (int u = 0; m < n_mels; ++m, ++u) acc[u] = fmaf(d[m], dctT[m * n_mfcc + c], acc[u]);
    mfcc[fa * n_mfcc + o] = __fadd_rn(__fadd_rn(__fadd_rn(acc[0], acc[1]), __fadd_rn(acc[2], acc[3])),
                                      __fadd_rn(__fadd_rn(acc[4], acc[5]), __fadd_rn(acc[6], acc[7])));
  }
}

// (3) the output block of MF_FB frames: the MFCC and its delta
__global__ __launch_bounds__(MF_THREADS) void mfcc_delta_kernel(const float* __restrict__ mfcc, int64_t total_frames,
                                                                const int64_t* __restrict__ frame_start, int n_sent, int n_mfcc,
                                                                void* __restrict__ out, int out_dtype, int64_t ld_out) {
  __shared__ int64_t sent_f0[MF_FB], sent_T[MF_FB];
  const int tid = threadIdx.x;
  const int64_t fa = (int64_t)blockIdx.x * MF_FB;
  const int nf = (int)min((int64_t)MF_FB, total_frames - fa);
  if (tid < nf) {
    const int s = mf_sentence_of(frame_start, n_sent, fa + tid);
    const int64_t f0 = mf_clamp(frame_start[s], total_frames);
    sent_f0[tid] = f0;
    sent_T[tid] = mf_clamp(frame_start[s + 1], total_frames) - f0;
  }
  __syncthreads();
  for (int o = tid; o < nf * n_mfcc; o += MF_THREADS) {
    const int fr = o / n_mfcc, c = o - fr * n_mfcc;
    const int64_t f = fa + fr, T = sent_T[fr], t = f - sent_f0[fr];
    float delta = 0.0f;
    if (T >= 9 && t >= 0 && t < T) {
      const int64_t tc = t < 4 ? 4 : (t > T - 5 ? T - 5 : t);  // the edge frames take the nearest interior slope: the same bits
      const float* __restrict__ x = mfcc + (sent_f0[fr] + tc) * n_mfcc + c;
      float acc = 0.0f;
#pragma unroll
      for (int k = 1; k <= 4; ++k) acc = __fadd_rn(acc, __fmul_rn((float)k, __fsub_rn(x[(int64_t)k * n_mfcc], x[-(int64_t)k * n_mfcc])));
      delta = acc / 60.0f;
    }
    mf_store(out, out_dtype, f * ld_out + c, mfcc[fa * n_mfcc + o]);
    mf_store(out, out_dtype, f * ld_out + n_mfcc + c, delta);
  }
}

}  // namespace

extern "C" int mts_mel_frames(void* stream, int n_sent, int n_fft, int hop, int n_mels, const float* wave, int64_t total_samples,
                              const int64_t* sent_start, const int64_t* sent_len, const int64_t* frame_start, int64_t total_frames,
                              const float* window, const float* twiddle, const int32_t* mel_first, const int32_t* mel_ptr, const float* mel_w,
                              int mel_nnz, float* mel) {
  MTS_CHECK_ARG(wave && sent_start && sent_len && frame_start && window && twiddle && mel_first && mel_ptr && mel_w && mel,
                "mts_mel_frames: null pointer");
  MTS_CHECK_ARG(n_sent >= 1 && total_samples >= 1 && total_frames >= 1 && hop >= 1 && n_mels >= 1 && mel_nnz >= 1,
                "mts_mel_frames: bad shape (n_sent %d, total_samples %lld, total_frames %lld, hop %d, n_mels %d, mel_nnz %d)", n_sent,
                (long long)total_samples, (long long)total_frames, hop, n_mels, mel_nnz);
  MTS_CHECK_ARG(n_fft >= MF_MIN_FFT && n_fft <= MF_MAX_FFT && (n_fft & (n_fft - 1)) == 0,
                "mts_mel_frames: n_fft must be a power of two in %d .. %d, not %d", MF_MIN_FFT, MF_MAX_FFT, n_fft);
  MTS_CHECK_ARG(aligned_to(wave, 4) && aligned_to(window, 4) && aligned_to(twiddle, 8) && aligned_to(mel_w, 4) && aligned_to(mel, 4),
                "mts_mel_frames: wave / tables / mel not aligned to their element size");
  MTS_UNSUPPORTED(total_frames <= 0x7fffffffLL, "mts_mel_frames: %lld frames are more than one launch covers", (long long)total_frames);
  const int N = n_fft >> 1;
  const size_t lds = (size_t)4 * (N + (N >> 5) + 1) * sizeof(float);
  hipLaunchKernelGGL(mel_frames_kernel, dim3((unsigned)total_frames), dim3(MF_THREADS), lds, (hipStream_t)stream, wave, total_samples,
                     sent_start, sent_len, frame_start, total_frames, n_sent, n_fft, hop, n_mels, window,
                     reinterpret_cast<const float2*>(twiddle), mel_first, mel_ptr, mel_w, mel_nnz, mel);
  MTS_LAUNCH_CHECK("mts_mel_frames");
  return MTS_OK;
}

extern "C" size_t mts_mfcc_frames_workspace(int n_sent, int64_t total_frames, int n_mfcc) {
  if (n_sent < 1 || total_frames < 1 || n_mfcc < 1) return 0;
  return ((size_t)n_sent + (size_t)total_frames * (size_t)n_mfcc) * sizeof(float);
}

extern "C" int mts_mfcc_frames(void* stream, int out_dtype, int n_sent, int n_mels, int n_mfcc, const float* mel, int64_t total_frames,
                               const int64_t* frame_start, const float* dct, void* workspace, size_t workspace_bytes, void* out,
                               int64_t ld_out) {
  MTS_CHECK_ARG(out_dtype == MTS_F32 || out_dtype == MTS_BF16, "mts_mfcc_frames: out_dtype must be fp32 or bf16 (got %d)", out_dtype);
  MTS_CHECK_ARG(mel && frame_start && dct && workspace && out, "mts_mfcc_frames: null pointer");
  MTS_CHECK_ARG(n_sent >= 1 && n_mels >= 1 && n_mfcc >= 1 && total_frames >= 1,
                "mts_mfcc_frames: bad shape (n_sent %d, n_mels %d, n_mfcc %d, total_frames %lld)", n_sent, n_mels, n_mfcc, (long long)total_frames);
  MTS_CHECK_ARG(n_mfcc <= n_mels, "mts_mfcc_frames: n_mfcc %d exceeds the %d mel bands", n_mfcc, n_mels);
  MTS_CHECK_ARG(ld_out >= 2 * (int64_t)n_mfcc, "mts_mfcc_frames: ld_out %lld is smaller than the %d columns written", (long long)ld_out,
                2 * n_mfcc);
  MTS_CHECK_ARG(workspace_bytes >= mts_mfcc_frames_workspace(n_sent, total_frames, n_mfcc),
                "mts_mfcc_frames: the workspace has %zu bytes, mts_mfcc_frames_workspace asks for %zu", workspace_bytes,
                mts_mfcc_frames_workspace(n_sent, total_frames, n_mfcc));
  MTS_CHECK_ARG(aligned_to(mel, 4) && aligned_to(dct, 4) && aligned_to(workspace, 4) && aligned_to(out, out_dtype == MTS_F32 ? 4 : 2),
                "mts_mfcc_frames: mel / dct / workspace / out not aligned to their element size");
  const size_t lds = ((size_t)n_mels * n_mfcc + (size_t)MF_FB * (n_mels + 1) + MF_FB) * sizeof(float);
  MTS_UNSUPPORTED(lds <= 64 * 1024, "mts_mfcc_frames: a %d x %d DCT table does not fit the 64 KiB of LDS of a workgroup", n_mfcc, n_mels);
  const int64_t groups = (total_frames + MF_FB - 1) / MF_FB;
  MTS_UNSUPPORTED(groups <= 0x7fffffffLL, "mts_mfcc_frames: %lld frames are more than one launch covers", (long long)total_frames);
  hipStream_t st = (hipStream_t)stream;
  float* top = reinterpret_cast<float*>(workspace);
  float* mfcc = top + n_sent;
  hipLaunchKernelGGL(mfcc_top_kernel, dim3((unsigned)n_sent), dim3(MF_THREADS), 0, st, mel, total_frames, frame_start, n_mels, top);
  MTS_LAUNCH_CHECK("mts_mfcc_frames (top)");
  hipLaunchKernelGGL(mfcc_dct_kernel, dim3((unsigned)groups), dim3(MF_THREADS), lds, st, mel, total_frames, frame_start, n_sent, n_mels, n_mfcc,
                     dct, top, mfcc);
  MTS_LAUNCH_CHECK("mts_mfcc_frames (dct)");
  hipLaunchKernelGGL(mfcc_delta_kernel, dim3((unsigned)groups), dim3(MF_THREADS), 0, st, mfcc, total_frames, frame_start, n_sent, n_mfcc, out,
                     out_dtype, ld_out);
  MTS_LAUNCH_CHECK("mts_mfcc_frames (delta)");
  return MTS_OK;
}
