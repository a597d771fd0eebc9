// Multi-tensor Adam over one parameter arena, its gradient guard (norm, clipping, non-finite skip) and the averaged
// shadow of the parameters.  gfx950.
#include <float.h>

#include "common.h"

namespace xas {

// ------------------------------------------------------------------ gradient guard (xas_hip.h: xas_grad_guard)
// The guard record of the header, as the kernels see it.
struct GuardRecord {
  float norm, scale;
  int skip, t, skipped;
  float step_size, inv_sqrt_bc2;
  int nonfinite;
};
static_assert(sizeof(GuardRecord) == XAS_GUARD_FLOATS * sizeof(float), "guard record layout");

constexpr int kGuardThreads = 256;

// Sum (and OR) over the block in a fixed order: a binary tree over the thread index.  Valid in thread 0.
__device__ __forceinline__ double guard_block_sum(double v, int& flag, double* s_sum) {
  const int t = threadIdx.x;
  flag = __syncthreads_or(flag);
  s_sum[t] = v;
  __syncthreads();
  for (int s = kGuardThreads / 2; s > 0; s >>= 1) {
    if (t < s) s_sum[t] += s_sum[t + s];
    __syncthreads();
  }
  return s_sum[0];
}

// One pass over the gradient arena: block b -> partial[b] = sum of g^2 over its grid-stride share, accumulated in double
// (a thread's elements in index order, then the tree above), and flags[b] = 1 if it met an element that is not finite.
// No atomics: both are pure functions of the arena's contents and the grid.
__global__ __launch_bounds__(kGuardThreads) void grad_sumsq_partial_kernel(const float4* __restrict__ g, long n4,
                                                                           double* __restrict__ partial,
                                                                           int* __restrict__ flags) {
  __shared__ double s_sum[kGuardThreads];
  double acc = 0.0;
  int bad = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 gv = g[i];
#define XAS_SUMSQ1(f)                                  \
    acc = fma((double)gv.f, (double)gv.f, acc);        \
    bad |= !(fabsf(gv.f) <= FLT_MAX);
    XAS_SUMSQ1(x) XAS_SUMSQ1(y) XAS_SUMSQ1(z) XAS_SUMSQ1(w)
#undef XAS_SUMSQ1
  }
  const double r = guard_block_sum(acc, bad, s_sum);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = r;
    flags[blockIdx.x] = bad;
  }
}

// One block: the per-block sums in index order (thread t takes the t-th run of consecutive blocks, then the tree), the
// decision, the step counter and the bias corrections of the step that follows -> the guard record.
__global__ __launch_bounds__(kGuardThreads) void grad_guard_finalize_kernel(const double* __restrict__ partial,
                                                                            const int* __restrict__ flags, int nblk,
                                                                            float max_norm, int skip_nonfinite, float lr,
                                                                            float beta1, float beta2, GuardRecord* rec) {
  __shared__ double s_sum[kGuardThreads];
  const int per = (nblk + kGuardThreads - 1) / kGuardThreads;
  double acc = 0.0;
  int bad = 0;
  for (int k = 0, b = threadIdx.x * per; k < per && b < nblk; ++k, ++b) {
    acc += partial[b];
    bad |= flags[b];
  }
  const double sumsq = guard_block_sum(acc, bad, s_sum);
  if (threadIdx.x != 0) return;
  const double norm = sqrt(sumsq);
  const float normf = (float)norm;
  float scale = 1.0f;
  if (max_norm > 0.f && max_norm <= FLT_MAX) {           // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1)
    const double c = (double)max_norm / (norm + 1e-6);   // (a NaN norm stays a NaN scale, as it does there)
    scale = c > 1.0 ? 1.0f : (float)c;
  }
  const int skip = (skip_nonfinite && (bad || !(normf <= FLT_MAX))) ? 1 : 0;
  const int t = rec->t + (skip ? 0 : 1);
  rec->norm = normf;
  rec->scale = scale;
  rec->skip = skip;
  rec->t = t;
  rec->skipped += skip;
  rec->nonfinite = bad;
  if (t >= 1) {
    rec->step_size = (float)((double)lr / (1.0 - pow((double)beta1, (double)t)));
    rec->inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)t)));
  }
}

// ------------------------------------------------------------------ Adam
// One element of the step.
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, float b1, float b2, float eps,
                                          float step_size, float inv_sqrt_bc2) {
  m = b1 * m + (1.f - b1) * g;
  v = b2 * v + (1.f - b2) * g * g;
  p -= step_size * m / (sqrtf(v) * inv_sqrt_bc2 + eps);
}

// One element of the averaged shadow of the parameters (xas_hip.h: xas_adam_step_ema): the product rounds once, the fused
// multiply-add once.  decay == 0 gives the new parameter itself.
__device__ __forceinline__ float ema_elem(float e, float p, float decay, float omd) { return fmaf(decay, e, omd * p); }

struct AdamArgs {
  float4* p;
  const float4* g;
  float4* m;
  float4* v;
  float4* e;                     // Ema: the shadow arena
  long n4;
  float b1, b2, eps;
  float decay, omd;              // Ema
  const GuardRecord* rec;        // Guarded: scale, the decision and the bias corrections come from the record ...
  float step_size, inv_sqrt_bc2; // ... else the bias corrections of this step come from the host
};

// Guarded: the step runs on g * scale, with scale, the bias corrections and the decision read from the guard record (uniform
// loads); a skipped step stores nothing, so the shadow keeps its bits too.  Ema: the shadow update while p_new is in a
// register: one more arena read, one more arena write.
template <bool Guarded, bool Ema>
__global__ void adam_step_kernel(AdamArgs a) {
  float scale = 1.f, step_size = a.step_size, inv_sqrt_bc2 = a.inv_sqrt_bc2;
  if constexpr (Guarded) {
    if (a.rec->skip != 0) return;
    scale = a.rec->scale; step_size = a.rec->step_size; inv_sqrt_bc2 = a.rec->inv_sqrt_bc2;
  }
  float4* __restrict__ p = a.p;
  const float4* __restrict__ g = a.g;
  float4* __restrict__ m = a.m;
  float4* __restrict__ v = a.v;
  float4* __restrict__ e = a.e;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n4; i += (long)gridDim.x * blockDim.x) {
    float4 gv = g[i];
    float4 mv = m[i], vv = v[i], pv = p[i], ev;
    if constexpr (Ema) ev = e[i];
    if constexpr (Guarded) { gv.x *= scale; gv.y *= scale; gv.z *= scale; gv.w *= scale; }
    adam_elem(pv.x, mv.x, vv.x, gv.x, a.b1, a.b2, a.eps, step_size, inv_sqrt_bc2);
    adam_elem(pv.y, mv.y, vv.y, gv.y, a.b1, a.b2, a.eps, step_size, inv_sqrt_bc2);
    adam_elem(pv.z, mv.z, vv.z, gv.z, a.b1, a.b2, a.eps, step_size, inv_sqrt_bc2);
    adam_elem(pv.w, mv.w, vv.w, gv.w, a.b1, a.b2, a.eps, step_size, inv_sqrt_bc2);
    if constexpr (Ema) {
      ev.x = ema_elem(ev.x, pv.x, a.decay, a.omd); ev.y = ema_elem(ev.y, pv.y, a.decay, a.omd);
      ev.z = ema_elem(ev.z, pv.z, a.decay, a.omd); ev.w = ema_elem(ev.w, pv.w, a.decay, a.omd);
    }
    m[i] = mv; v[i] = vv; p[i] = pv;
    if constexpr (Ema) e[i] = ev;
  }
}

// The launch of all four forms: a guard record selects Guarded, a shadow arena Ema.
static int adam_launch(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1, float beta2, float eps,
                       float step_size, float inv_sqrt_bc2, float decay, float omd, const void* guard, void* stream) {
  const AdamArgs a = {reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(m),
                      reinterpret_cast<float4*>(v), reinterpret_cast<float4*>(ema), n / 4, beta1, beta2, eps, decay, omd,
                      static_cast<const GuardRecord*>(guard), step_size, inv_sqrt_bc2};
  auto* kernel = guard ? (ema ? adam_step_kernel<true, true> : adam_step_kernel<true, false>)
                       : (ema ? adam_step_kernel<false, true> : adam_step_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(ew_grid(n / 4)), dim3(256), 0, as_stream(stream), a);
  XAS_LAUNCH_CHECK();
  return 0;
}

// the bias corrections of step `step`, as the unguarded entry points hand them to the kernel
struct AdamBias { float step_size, inv_sqrt_bc2; };
static AdamBias adam_bias(float lr, float beta1, float beta2, int step) {
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  return {(float)(lr / bc1), (float)(1.0 / sqrt(bc2))};
}

}  // namespace xas

using namespace xas;

// workspace of xas_grad_guard: one double and one flag word per block of the norm pass
extern "C" size_t xas_grad_guard_workspace_bytes(long n) {
  if (n <= 0 || n % 4 != 0) return 0;
  return (size_t)ew_grid(n / 4, kGuardThreads) * (sizeof(double) + sizeof(int));
}

extern "C" int xas_grad_guard(const float* g, long n, float max_norm, int skip_nonfinite, float lr, float beta1,
                              float beta2, void* guard, void* workspace, void* stream) {
  XAS_REQUIRE(g && guard && workspace && n > 0 && n % 4 == 0, "grad_guard: bad arguments (n must be a multiple of 4)");
  XAS_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)guard & 3) == 0 && ((uintptr_t)g & 15) == 0,
              "grad_guard: the arena must be 16-byte, the workspace 8-byte and the guard record 4-byte aligned");
  const unsigned nblk = ew_grid(n / 4, kGuardThreads);
  double* partial = static_cast<double*>(workspace);
  int* flags = reinterpret_cast<int*>(partial + nblk);
  hipLaunchKernelGGL(grad_sumsq_partial_kernel, dim3(nblk), dim3(kGuardThreads), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(g), n / 4, partial, flags);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_guard_finalize_kernel, dim3(1), dim3(kGuardThreads), 0, as_stream(stream), partial, flags,
                     (int)nblk, max_norm, skip_nonfinite, lr, beta1, beta2, static_cast<GuardRecord*>(guard));
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                             float eps, int step, void* stream) {
  XAS_REQUIRE(p && g && m && v && n > 0 && n % 4 == 0 && step >= 1, "adam: bad arguments (n must be a multiple of 4)");
  const AdamBias bc = adam_bias(lr, beta1, beta2, step);
  return adam_launch(p, g, m, v, nullptr, n, beta1, beta2, eps, bc.step_size, bc.inv_sqrt_bc2, 0.f, 0.f, nullptr, stream);
}

extern "C" int xas_adam_step_guarded(float* p, const float* g, float* m, float* v, long n, float beta1, float beta2,
                                     float eps, const void* guard, void* stream) {
  XAS_REQUIRE(p && g && m && v && guard && n > 0 && n % 4 == 0, "adam guarded: bad arguments (n must be a multiple of 4)");
  return adam_launch(p, g, m, v, nullptr, n, beta1, beta2, eps, 0.f, 0.f, 0.f, 0.f, guard, stream);
}

// the two arguments every averaged step checks alike: the shadow arena and its decay
#define XAS_REQUIRE_EMA(name)                                                                                        \
  XAS_REQUIRE(ema, name ": the shadow arena (ema) is null");                                                         \
  XAS_REQUIRE(decay >= 0.f && decay < 1.f, name ": decay must be in [0, 1), got %g", (double)decay)

extern "C" int xas_adam_step_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1,
                                 float beta2, float eps, int step, float decay, float one_minus_decay, void* stream) {
  XAS_REQUIRE(p && g && m && v && n > 0 && n % 4 == 0 && step >= 1, "adam ema: bad arguments (n must be a multiple of 4)");
  XAS_REQUIRE_EMA("adam ema");
  const AdamBias bc = adam_bias(lr, beta1, beta2, step);
  return adam_launch(p, g, m, v, ema, n, beta1, beta2, eps, bc.step_size, bc.inv_sqrt_bc2, decay, one_minus_decay, nullptr,
                     stream);
}

extern "C" int xas_adam_step_guarded_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1,
                                         float beta2, float eps, float decay, float one_minus_decay, const void* guard,
                                         void* stream) {
  XAS_REQUIRE(p && g && m && v && n > 0 && n % 4 == 0, "adam guarded ema: bad arguments (n must be a multiple of 4)");
  XAS_REQUIRE(guard, "adam guarded ema: the guard record is null");
  XAS_REQUIRE_EMA("adam guarded ema");
  return adam_launch(p, g, m, v, ema, n, beta1, beta2, eps, 0.f, 0.f, decay, one_minus_decay, guard, stream);
}
#undef XAS_REQUIRE_EMA
