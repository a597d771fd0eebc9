// What the averaged-weights step costs: at the detector arena's size, HIP-event times of
//   plain     xas_adam_step                                   reads p g m v, writes p m v        7 arena streams
//   fused     xas_adam_step_ema                               + one read and one write of ema    9
//   separate  xas_adam_step, then a stand-alone average pass  + read p, read ema, write ema      10   (what the fusion avoids)
// The three are timed in turn inside every repetition (a window of `inner` back-to-back calls between two events), after a
// warm-up of each; the medians over the repetitions are printed, with the spread and the bytes-over-time rates.
// usage: ema_adam_timing [n floats = 34708516] [repetitions = 41] [inner = 20]
// build: hipcc -O3 --offload-arch=gfx950 -Iinclude tools/micro/ema_adam_timing.hip -o tools/micro/ema_adam_timing \
//        -Lx-as-supervision_amd/xas_amd -lxas_hip -Wl,-rpath,'$ORIGIN/../../x-as-supervision_amd/xas_amd'
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "xas_hip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)
#define XK(x) do { int r_ = (x); if (r_ != 0) { printf("%s:%d xas rc %d: %s\n", __FILE__, __LINE__, r_, xas_last_error()); exit(1); } } while (0)

__global__ void fill(float4* __restrict__ x, long n4, float v) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
    x[i] = make_float4(v, v, v, v);
}

// the average as a pass of its own: the launch shape and the arithmetic of the fused kernels
__global__ void ema_average(const float4* __restrict__ p, float4* __restrict__ e, long n4, float decay, float omd) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 pv = p[i];
    float4 ev = e[i];
    ev.x = fmaf(decay, ev.x, omd * pv.x); ev.y = fmaf(decay, ev.y, omd * pv.y);
    ev.z = fmaf(decay, ev.z, omd * pv.z); ev.w = fmaf(decay, ev.w, omd * pv.w);
    e[i] = ev;
  }
}

static unsigned grid_of(long n4) {
  const long b = (n4 + 255) / 256;
  return (unsigned)(b > 4096 ? 4096 : b);
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 34708516L;
  const int reps = argc > 2 ? atoi(argv[2]) : 41, inner = argc > 3 ? atoi(argv[3]) : 20;
  if (n <= 0 || n % 4 != 0 || reps < 1 || inner < 1) { printf("n must be a positive multiple of 4\n"); return 1; }
  const long n4 = n / 4;
  float *p, *g, *m, *v, *e;
  for (float** a : {&p, &g, &m, &v, &e}) CK(hipMalloc(a, n * sizeof(float)));
  const float init[5] = {0.5f, 0.01f, 0.f, 0.f, 0.5f};
  int k = 0;
  for (float* a : {p, g, m, v, e}) hipLaunchKernelGGL(fill, dim3(grid_of(n4)), dim3(256), 0, 0, reinterpret_cast<float4*>(a), n4, init[k++]);
  CK(hipDeviceSynchronize());
  const float lr = 2e-4f, b1 = 0.5f, b2 = 0.999f, eps = 1e-8f, decay = 0.999f, omd = (float)(1.0 - (double)decay);
  int step = 0;
  auto run = [&](int which) {
    ++step;
    if (which == 1) {
      XK(xas_adam_step_ema(p, g, m, v, e, n, lr, b1, b2, eps, step, decay, omd, nullptr));
    } else {
      XK(xas_adam_step(p, g, m, v, n, lr, b1, b2, eps, step, nullptr));
      if (which == 2) hipLaunchKernelGGL(ema_average, dim3(grid_of(n4)), dim3(256), 0, 0, reinterpret_cast<const float4*>(p), reinterpret_cast<float4*>(e), n4, decay, omd);
    }
  };
  hipEvent_t t0, t1;
  CK(hipEventCreate(&t0));
  CK(hipEventCreate(&t1));
  for (int which = 0; which < 3; ++which)
    for (int i = 0; i < 5; ++i) run(which);
  CK(hipDeviceSynchronize());
  std::vector<float> us[3];
  for (int r = 0; r < reps; ++r)
    for (int which = 0; which < 3; ++which) {
      CK(hipEventRecord(t0, 0));
      for (int i = 0; i < inner; ++i) run(which);
      CK(hipEventRecord(t1, 0));
      CK(hipEventSynchronize(t1));
      float ms = 0.f;
      CK(hipEventElapsedTime(&ms, t0, t1));
      us[which].push_back(ms * 1000.f / inner);
    }
  CK(hipGetLastError());
  const char* name[3] = {"plain     xas_adam_step", "fused     xas_adam_step_ema", "separate  xas_adam_step + average pass"};
  const int streams[3] = {7, 9, 10};
  float med[3];
  printf("n = %ld floats (%.1f MB per arena), %d repetitions of %d calls each, the three in turn\n", n, n * 4 / 1e6, reps, inner);
  for (int w = 0; w < 3; ++w) {
    std::sort(us[w].begin(), us[w].end());
    med[w] = us[w][reps / 2];
    printf("%-40s median %8.1f us  (min %8.1f  max %8.1f)  %2d arena streams  %.2f TB/s\n", name[w], med[w], us[w][0],
           us[w][reps - 1], streams[w], streams[w] * (double)n * 4 / (med[w] * 1e-6) / 1e12);
  }
  printf("fused / plain = %.3f (bytes: 9/7 = 1.286)   fused / separate = %.3f (bytes: 9/10 = 0.900)\n", med[1] / med[0], med[1] / med[2]);
  return 0;
}
