// Layout changes: NCHW <-> NHWC, and the mirrored pair stack of the flip test.  gfx950.
#include "common.h"

namespace xas {

__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, int N, int C, int HW, float* __restrict__ y, int inverse) {
  const long total = (long)N * C * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    // i enumerates NHWC
    const int c = i % C; const long t = i / C; const long p = t % HW; const long n = t / HW;
    const long j = (n * C + c) * HW + p;
    if (inverse) y[j] = x[i]; else y[i] = x[j];
  }
}

// ------------------------------------------------------------------ mirrored pair stack (flip test)
// x [B][C][H][W] -> y [2B][H][W][C]: y[b] = x[b] and y[B + b][h][w] = x[b][h][W - 1 - w], the batch a flip-test pass feeds
// the detector (torch.flip + torch.cat + the layout change in one pass that reads x once).  A thread owns one pixel of x:
// the loads of a wave are contiguous in every channel plane, its stores contiguous in both halves of y.
__global__ void nchw_to_nhwc_mirror_pair_kernel(const float* __restrict__ x, int B, int C, int H, int W, float* __restrict__ y) {
  const long HW = (long)H * W, pixels = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (long)gridDim.x * blockDim.x) {
    const long b = i / HW, p = i - b * HW;
    const int w = (int)(p % W);
    const float* src = x + b * C * HW + p;
    float* same = y + i * C;
    float* mirrored = y + (pixels + i + (W - 1 - 2 * w)) * C;      // pixel (B + b, h, W - 1 - w)
    for (int c = 0; c < C; ++c) {
      const float v = src[c * HW];
      same[c] = v;
      mirrored[c] = v;
    }
  }
}

}  // namespace xas

using namespace xas;

extern "C" int xas_nchw_to_nhwc(const float* x, int N, int C, int H, int W, float* y, void* stream) {
  XAS_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0, "nchw_to_nhwc: bad arguments");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(ew_grid((long)N * C * H * W)), dim3(256), 0, as_stream(stream), x, N, C,
                     H * W, y, 0);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_nhwc_to_nchw(const float* x, int N, int C, int H, int W, float* y, void* stream) {
  XAS_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0, "nhwc_to_nchw: bad arguments");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(ew_grid((long)N * C * H * W)), dim3(256), 0, as_stream(stream), x, N, C,
                     H * W, y, 1);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_nchw_to_nhwc_mirror_pair(const float* x, int B, int C, int H, int W, float* y, void* stream) {
  XAS_REQUIRE(x && y && x != y && B > 0 && C > 0 && H > 0 && W > 0, "nchw_to_nhwc_mirror_pair: bad arguments");
  XAS_REQUIRE((long)2 * B * C * H * W < (1l << 40), "nchw_to_nhwc_mirror_pair: tensor too large");
  hipLaunchKernelGGL(nchw_to_nhwc_mirror_pair_kernel, dim3(ew_grid((long)B * H * W)), dim3(256), 0, as_stream(stream), x, B, C,
                     H, W, y);
  XAS_LAUNCH_CHECK();
  return 0;
}
