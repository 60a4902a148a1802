// Optimizer steps over the flat fp32 parameter buffer + error plumbing of the C ABI.
// HBM-bound streaming kernels: 16-byte accesses, grid-stride, optional fused bf16 weight copy so the next
// step's GEMMs never re-read the fp32 master weights.
#include <stdarg.h>
#include <algorithm>
#include <math.h>
#include <mutex>
#include "common.h"

static thread_local char g_err[512] = "";
void mts_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* mts_last_error(void) { return g_err; }

// The dynamic-LDS limit is a property of (kernel, device): g_lds remembers the bytes set per kernel and device.  Entries are
// appended under the mutex and published through g_lds_n, so the steady-state path only reads atomics.  A kernel or device
// the table has no room for is opted in on every launch.
enum { LDS_KERNELS = 256, LDS_DEVICES = 16 };
struct LdsEntry { const void* fn; std::atomic<uint32_t> bytes[LDS_DEVICES]; };
static LdsEntry g_lds[LDS_KERNELS];
static std::atomic<int> g_lds_n{0};
static std::mutex g_lds_mu;

static LdsEntry* lds_find(const void* kernel, int n) {
  for (int i = 0; i < n; ++i)
    if (g_lds[i].fn == kernel) return &g_lds[i];
  return nullptr;
}

int mts_dyn_lds(const void* kernel, size_t bytes, const char* who) {
  MTS_UNSUPPORTED(bytes <= 160 * 1024, "%s: needs %zu bytes of LDS (> 160 KiB)", who, bytes);
  if (bytes <= 64 * 1024) return MTS_OK;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) { mts_set_error("%s: hipGetDevice: %s", who, hipGetErrorString(e)); return MTS_ERR_LAUNCH; }
  const bool tracked = dev >= 0 && dev < LDS_DEVICES;
  LdsEntry* x = tracked ? lds_find(kernel, g_lds_n.load(std::memory_order_acquire)) : nullptr;
  if (x && x->bytes[dev].load(std::memory_order_acquire) >= bytes) return MTS_OK;
  std::lock_guard<std::mutex> lk(g_lds_mu);
  if (tracked && !x) {
    const int n = g_lds_n.load(std::memory_order_relaxed);
    x = lds_find(kernel, n);
    if (!x && n < LDS_KERNELS) {
      x = &g_lds[n];
      x->fn = kernel;
      g_lds_n.store(n + 1, std::memory_order_release);
    }
  }
  if (x && x->bytes[dev].load(std::memory_order_relaxed) >= bytes) return MTS_OK;    // another thread got here first
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) { mts_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e)); return MTS_ERR_LAUNCH; }
  if (x) x->bytes[dev].store((uint32_t)bytes, std::memory_order_release);
  return MTS_OK;
}
extern "C" const char* mts_version(void) { return "mts-hip 1 gfx950"; }

// Gradient clipping (Lightning's Trainer(gradient_clip_val, gradient_clip_algorithm) -> torch.nn.utils.clip_grad_norm_ / clip_grad_value_)
// is folded into the optimizer pass: the kernels below are instantiated once without it (mts_adam_step / mts_sgd_step, the
// arithmetic they always had) and once per clipping mode.
enum { CLIP_NONE = 0, CLIP_NORM = 1, CLIP_VALUE = 2 };

// c: the norm mode's coefficient / the value mode's bound.  The library is built with -ffp-contract=off, so a coefficient of
// exactly 1 leaves the bits of the unclipped step (x * 1.0f == x).
template <int CLIP> __device__ __forceinline__ float clip_grad(float gr, float c) {
  if (CLIP == CLIP_NORM) return gr * c;
  if (CLIP == CLIP_VALUE) return gr > c ? c : (gr < -c ? -c : gr);   // a NaN fails both comparisons and stays NaN
  return gr;
}

// clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to at most 1; a NaN norm gives a NaN coefficient
// (torch.clamp keeps NaN, fminf would not)
__device__ __forceinline__ float clip_coef(float total_norm, float max_norm) {
  const float c = max_norm / (total_norm + 1e-6f);
  return c > 1.f ? 1.f : c;
}

// torch.optim.Adam (no amsgrad, no weight decay): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
template <int CLIP>
__device__ __forceinline__ void adam_loop(size_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                          float gscale, bf16_t* __restrict__ copy, float c) {
  const size_t stride = (size_t)gridDim.x * 256 * 4;
  const float step_size = lr / bc1;
  for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      float pv[4], gv[4], mv[4], vv[4];
      load4<float>(p + i, pv); load4<float>(g + i, gv); load4<float>(m + i, mv); load4<float>(v + i, vv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gr = clip_grad<CLIP>(gv[j] * gscale, c);
        mv[j] = mv[j] + (1.f - b1) * (gr - mv[j]);                 // lerp form used by torch
        vv[j] = b2 * vv[j] + (1.f - b2) * gr * gr;
        const float denom = sqrtf(vv[j]) / bc2_sqrt + eps;
        pv[j] = pv[j] - step_size * (mv[j] / denom);
      }
      store4<float>(p + i, pv); store4<float>(m + i, mv); store4<float>(v + i, vv);
      if (copy) store4<bf16_t>(copy + i, pv);
    } else {
      for (size_t k = i; k < n; ++k) {
        const float gr = clip_grad<CLIP>(g[k] * gscale, c);
        const float mm = m[k] + (1.f - b1) * (gr - m[k]);
        const float vv = b2 * v[k] + (1.f - b2) * gr * gr;
        m[k] = mm; v[k] = vv;
        const float pp = p[k] - step_size * (mm / (sqrtf(vv) / bc2_sqrt + eps));
        p[k] = pp;
        if (copy) copy[k] = (bf16_t)pp;
      }
    }
  }
}

__global__ __launch_bounds__(256) void adam_kernel(size_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                   float gscale, bf16_t* __restrict__ copy) {
  adam_loop<CLIP_NONE>(n, p, g, m, v, lr, b1, b2, eps, bc1, bc2_sqrt, gscale, copy, 1.f);
}

// the scale comes from DEVICE memory (total_norm, written by mts_grad_norm earlier on the stream): the host never sees it
template <int CLIP>
__global__ __launch_bounds__(256) void adam_clip_kernel(size_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float lr, float b1, float b2, float eps, float bc1,
                                                        float bc2_sqrt, float gscale, bf16_t* __restrict__ copy,
                                                        const float* __restrict__ total_norm, float max_norm, float clip_value,
                                                        float* __restrict__ coef_out) {
  float c = clip_value;
  if (CLIP == CLIP_NORM) {
    c = clip_coef(*total_norm, max_norm);
    if (coef_out && blockIdx.x == 0 && threadIdx.x == 0) *coef_out = c;
  }
  adam_loop<CLIP>(n, p, g, m, v, lr, b1, b2, eps, bc1, bc2_sqrt, gscale, copy, c);
}

// torch.optim.SGD(momentum, weight_decay, dampening 0, no nesterov); the weight decay is added to the CLIPPED gradient, as when
// torch clips .grad before step()
template <int CLIP>
__device__ __forceinline__ void sgd_loop(size_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, float lr,
                                         float mom, float wd, int first, float gscale, bf16_t* __restrict__ copy, float c) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float gr = clip_grad<CLIP>(g[i] * gscale, c) + wd * p[i];
    float b = first ? gr : mom * buf[i] + gr;
    buf[i] = b;
    const float pp = p[i] - lr * b;
    p[i] = pp;
    if (copy) copy[i] = (bf16_t)pp;
  }
}

__global__ __launch_bounds__(256) void sgd_kernel(size_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, float lr,
                                                  float mom, float wd, int first, float gscale, bf16_t* __restrict__ copy) {
  sgd_loop<CLIP_NONE>(n, p, g, buf, lr, mom, wd, first, gscale, copy, 1.f);
}

template <int CLIP>
__global__ __launch_bounds__(256) void sgd_clip_kernel(size_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                       float lr, float mom, float wd, int first, float gscale, bf16_t* __restrict__ copy,
                                                       const float* __restrict__ total_norm, float max_norm, float clip_value,
                                                       float* __restrict__ coef_out) {
  float c = clip_value;
  if (CLIP == CLIP_NORM) {
    c = clip_coef(*total_norm, max_norm);
    if (coef_out && blockIdx.x == 0 && threadIdx.x == 0) *coef_out = c;
  }
  sgd_loop<CLIP>(n, p, g, buf, lr, mom, wd, first, gscale, copy, c);
}

// the vector accesses of adam_loop: 16 bytes on the fp32 operands, 8 on the bf16 copy (which may be NULL)
static int check_adam_alignment(const char* name, const float* param, const float* grad, const float* exp_avg, const float* exp_avg_sq,
                                const void* bf16_copy) {
  MTS_CHECK_ARG(aligned_to(param, 16) && aligned_to(grad, 16) && aligned_to(exp_avg, 16) && aligned_to(exp_avg_sq, 16) && aligned_to(bf16_copy, 8),
                "%s: param, grad and moments must be 16-byte aligned, bf16_copy 8-byte aligned", name);
  return MTS_OK;
}

// sgd_loop works element by element: every operand on its element size
static int check_sgd_alignment(const char* name, const float* param, const float* grad, const float* momentum_buf, const void* bf16_copy) {
  MTS_CHECK_ARG(aligned_to(param, 4) && aligned_to(grad, 4) && aligned_to(momentum_buf, 4) && aligned_to(bf16_copy, 2),
                "%s: param, grad and momentum_buf must be 4-byte aligned, bf16_copy 2-byte aligned", name);
  return MTS_OK;
}

extern "C" int mts_adam_step(void* stream, size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                             float beta2, float eps, int step, float grad_scale, void* bf16_copy) {
  MTS_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && step >= 1, "mts_adam_step: bad arguments");
  if (int rc = check_adam_alignment("mts_adam_step", param, grad, exp_avg, exp_avg_sq, bf16_copy)) return rc;
  if (n == 0) return MTS_OK;
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const int blocks = (int)std::min<size_t>(2048, (n / 4 + 255) / 256 + 1);
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
                     (float)bc1, (float)sqrt(bc2), grad_scale, (bf16_t*)bf16_copy);
  MTS_LAUNCH_CHECK("mts_adam_step");
  return MTS_OK;
}

extern "C" int mts_sgd_step(void* stream, size_t n, float* param, const float* grad, float* momentum_buf, float lr, float momentum,
                            float weight_decay, int first_step, float grad_scale, void* bf16_copy) {
  MTS_CHECK_ARG(param && grad && momentum_buf, "mts_sgd_step: bad arguments");
  if (int rc = check_sgd_alignment("mts_sgd_step", param, grad, momentum_buf, bf16_copy)) return rc;
  if (n == 0) return MTS_OK;
  const int blocks = (int)std::min<size_t>(2048, (n + 255) / 256);
  hipLaunchKernelGGL(sgd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, param, grad, momentum_buf, lr, momentum, weight_decay,
                     first_step, grad_scale, (bf16_t*)bf16_copy);
  MTS_LAUNCH_CHECK("mts_sgd_step");
  return MTS_OK;
}

// total_norm != NULL selects the norm mode, total_norm == NULL with clip_value > 0 the value mode
static int check_clip_args(const char* name, const float* total_norm, float max_norm, float clip_value) {
  MTS_CHECK_ARG(max_norm >= 0.f, "%s: max_norm must be >= 0 (got %g)", name, (double)max_norm);
  MTS_CHECK_ARG(clip_value >= 0.f, "%s: clip_value must be >= 0 (got %g)", name, (double)clip_value);
  MTS_CHECK_ARG(total_norm ? clip_value == 0.f : clip_value > 0.f,
                "%s: give either total_norm (norm mode, clip_value 0) or clip_value > 0 without total_norm (value mode)", name);
  return MTS_OK;
}

extern "C" int mts_adam_step_clipped(void* stream, size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                                     float beta1, float beta2, float eps, int step, float grad_scale, void* bf16_copy, const float* total_norm,
                                     float max_norm, float clip_value, float* clip_coef_out) {
  MTS_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && step >= 1, "mts_adam_step_clipped: bad arguments");
  if (int rc = check_clip_args("mts_adam_step_clipped", total_norm, max_norm, clip_value)) return rc;
  if (int rc = check_adam_alignment("mts_adam_step_clipped", param, grad, exp_avg, exp_avg_sq, bf16_copy)) return rc;
  MTS_CHECK_ARG(aligned_to(total_norm, 4) && aligned_to(clip_coef_out, 4), "mts_adam_step_clipped: misaligned scalar");
  if (n == 0) return MTS_OK;
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const int blocks = (int)std::min<size_t>(2048, (n / 4 + 255) / 256 + 1);
  auto kernel = total_norm ? adam_clip_kernel<CLIP_NORM> : adam_clip_kernel<CLIP_VALUE>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
                     (float)bc1, (float)sqrt(bc2), grad_scale, (bf16_t*)bf16_copy, total_norm, max_norm, clip_value, clip_coef_out);
  MTS_LAUNCH_CHECK("mts_adam_step_clipped");
  return MTS_OK;
}

extern "C" int mts_sgd_step_clipped(void* stream, size_t n, float* param, const float* grad, float* momentum_buf, float lr, float momentum,
                                    float weight_decay, int first_step, float grad_scale, void* bf16_copy, const float* total_norm,
                                    float max_norm, float clip_value, float* clip_coef_out) {
  MTS_CHECK_ARG(param && grad && momentum_buf, "mts_sgd_step_clipped: bad arguments");
  if (int rc = check_clip_args("mts_sgd_step_clipped", total_norm, max_norm, clip_value)) return rc;
  if (int rc = check_sgd_alignment("mts_sgd_step_clipped", param, grad, momentum_buf, bf16_copy)) return rc;
  MTS_CHECK_ARG(aligned_to(total_norm, 4) && aligned_to(clip_coef_out, 4), "mts_sgd_step_clipped: misaligned scalar");
  if (n == 0) return MTS_OK;
  const int blocks = (int)std::min<size_t>(2048, (n + 255) / 256);
  auto kernel = total_norm ? sgd_clip_kernel<CLIP_NORM> : sgd_clip_kernel<CLIP_VALUE>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, param, grad, momentum_buf, lr, momentum, weight_decay,
                     first_step, grad_scale, (bf16_t*)bf16_copy, total_norm, max_norm, clip_value, clip_coef_out);
  MTS_LAUNCH_CHECK("mts_sgd_step_clipped");
  return MTS_OK;
}

// ---- || grad * grad_scale ||_2 over spans of the flat gradient ------------------------------------------------------------------
// A pure read stream: every lane keeps two 16-byte loads in flight and four running sums, a workgroup adds its lanes through a
// wave butterfly and a four-entry LDS tree and STORES one partial; a one-workgroup kernel adds the partials in a fixed order and
// writes the norm.  No float atomics anywhere: which elements a lane sums and the order of every addition depend on the span
// lengths alone, so the same input gives the same bits on every run and on every rank.
#define NORM_MAX_SPANS 4
#define NORM_MAX_BLOCKS 2048
struct NormSpans {
  const float* p[NORM_MAX_SPANS];
  size_t n[NORM_MAX_SPANS];
};

__device__ __forceinline__ float block_sum_256(float s) {
  __shared__ float wave_part[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
  __syncthreads();
  return (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(NormSpans spans, int n_spans, float gscale, float* __restrict__ partials) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const size_t stride = (size_t)gridDim.x * 256 * 4;
  const size_t first = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
#pragma unroll
  for (int s = 0; s < NORM_MAX_SPANS; ++s) {
    if (s >= n_spans) break;
    const float* __restrict__ g = spans.p[s];
    const size_t n = spans.n[s], nv = n & ~(size_t)3;
    size_t i = first;
    for (; i + stride < nv; i += 2 * stride) {
      float a[4], b[4];
      load4<float>(g + i, a); load4<float>(g + i + stride, b);
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float t = a[j] * gscale; acc[j] += t * t; }
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float t = b[j] * gscale; acc[j] += t * t; }
    }
    if (i < nv) {
      float a[4];
      load4<float>(g + i, a);
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float t = a[j] * gscale; acc[j] += t * t; }
    }
    if (first == 0)                                                // the span's last n % 4 elements: one lane
      for (size_t k = nv; k < n; ++k) { const float t = g[k] * gscale; acc[0] += t * t; }
  }
  const float total = block_sum_256((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const float* __restrict__ partials, int n_partials, float* __restrict__ norm_out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n_partials; i += 256) s += partials[i];
  const float total = block_sum_256(s);
  if (threadIdx.x == 0) *norm_out = sqrtf(total);
}

extern "C" size_t mts_grad_norm_workspace(void) { return NORM_MAX_BLOCKS * sizeof(float); }

extern "C" int mts_grad_norm(void* stream, const float* grad, int n_spans, const size_t* span_begin_host, const size_t* span_end_host,
                             float grad_scale, float* workspace, float* norm_out) {
  MTS_CHECK_ARG(grad && span_begin_host && span_end_host && workspace && norm_out, "mts_grad_norm: null pointer");
  MTS_CHECK_ARG(n_spans >= 1 && n_spans <= NORM_MAX_SPANS, "mts_grad_norm: n_spans must be 1..%d (got %d)", NORM_MAX_SPANS, n_spans);
  MTS_CHECK_ARG(aligned_to(workspace, 4) && aligned_to(norm_out, 4), "mts_grad_norm: misaligned workspace or result");
  NormSpans spans = {};
  size_t longest = 0;
  for (int s = 0; s < n_spans; ++s) {
    MTS_CHECK_ARG(span_end_host[s] >= span_begin_host[s], "mts_grad_norm: span %d ends before it begins", s);
    spans.p[s] = grad + span_begin_host[s];
    spans.n[s] = span_end_host[s] - span_begin_host[s];
    MTS_CHECK_ARG(aligned_to(spans.p[s], 16), "mts_grad_norm: span %d does not begin on a 16-byte boundary", s);
    longest = std::max(longest, spans.n[s]);
  }
  if (longest == 0) return MTS_OK;
  const int blocks = (int)std::min<size_t>(NORM_MAX_BLOCKS, std::max<size_t>(1, (longest / 4 + 255) / 256));
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, spans, n_spans, grad_scale, workspace);
  MTS_LAUNCH_CHECK("mts_grad_norm");
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace, blocks, norm_out);
  MTS_LAUNCH_CHECK("mts_grad_norm");
  return MTS_OK;
}

// x *= scale (fp32, any n): the loss-gradient weight of token-weighted data parallelism (trainer.py: a rank's d loss / d scores
// is multiplied by world * n_r / sum n_r before the SUM all-reduce)
__global__ __launch_bounds__(256) void scale_kernel(size_t n, float* __restrict__ x, float scale) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) x[i] *= scale;
}
extern "C" int mts_scale(void* stream, size_t n, float* x, float scale) {
  MTS_CHECK_ARG(x || n == 0, "mts_scale: null pointer");
  if (n == 0 || scale == 1.0f) return MTS_OK;
  const int blocks = (int)std::min<size_t>(1024, (n + 255) / 256);
  hipLaunchKernelGGL(scale_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, x, scale);
  MTS_LAUNCH_CHECK("mts_scale");
  return MTS_OK;
}
