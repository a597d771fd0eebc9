// Parameter-free NHWC layers, HBM bound: 3x3-s2 max pool, bilinear x2 upsample and sigmoid, each with its backward.  gfx950.
//
// Replaces max_pool2d (resnet.py:20), upsample_bilinear2d (physique_network.py:31) and sigmoid
// (physique_network.py:57).  The pool and resample kernels move float4 (4 channels) per lane.
#include "common.h"

namespace xas {

// ---------------------------------------------------------------- max pool 3x3 s2 p1
// One block walks whole image ROWS (grid-stride over n * rows): the row decode is scalar and 32-bit, a lane splits only its
// element index into (column, channel quad).  (r04: the flat 64-bit index per thread cost three emulated 64-bit divisions -
// backward 697 us for 1.4 GB = 2.0 TB/s at 256 images.)
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C, int Ho, int Wo,
                                                          float* __restrict__ y, int8_t* __restrict__ idx) {
  const int C4 = C / 4, per_row = Wo * C4;
  for (int row = blockIdx.x; row < N * Ho; row += gridDim.x) {
    const int n = row / Ho, ho = row - n * Ho;
    const float* xn = x + (size_t)n * H * W * C;
    const size_t obase = (size_t)row * per_row;
    for (int e = threadIdx.x; e < per_row; e += blockDim.x) {
      const int wo = e / C4, c = (e - wo * C4) * 4;
      float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      int b0 = 0, b1 = 0, b2 = 0, b3 = 0;
      bool first = true;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int hi = ho * 2 - 1 + r;
        if ((unsigned)hi >= (unsigned)H) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int wi = wo * 2 - 1 + s;
          if ((unsigned)wi >= (unsigned)W) continue;
          const float4 v = *reinterpret_cast<const float4*>(xn + ((size_t)hi * W + wi) * C + c);
          const int tap = r * 3 + s;
          if (first || v.x > best.x) { best.x = v.x; b0 = tap; }
          if (first || v.y > best.y) { best.y = v.y; b1 = tap; }
          if (first || v.z > best.z) { best.z = v.z; b2 = tap; }
          if (first || v.w > best.w) { best.w = v.w; b3 = tap; }
          first = false;
        }
      }
      *reinterpret_cast<float4*>(y + (obase + e) * 4) = best;
      *reinterpret_cast<char4*>(idx + (obase + e) * 4) = make_char4((char)b0, (char)b1, (char)b2, (char)b3);
    }
  }
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy, const int8_t* __restrict__ idx, int N, int H,
                                                          int W, int C, int Ho, int Wo, float* __restrict__ dx) {
  const int C4 = C / 4, per_row = W * C4;
  for (int row = blockIdx.x; row < N * H; row += gridDim.x) {
    const int n = row / H, hi = row - n * H;
    const size_t obase = (size_t)row * per_row;
    for (int e = threadIdx.x; e < per_row; e += blockDim.x) {
      const int wi = e / C4, c = (e - wi * C4) * 4;
      float4 acc = make_float4(0, 0, 0, 0);
      // output windows ho with ho*2-1 <= hi <= ho*2+1
      for (int ho = hi / 2; ho <= (hi + 1) / 2; ++ho) {
        if (ho >= Ho) continue;
        const int r = hi - (ho * 2 - 1);
        if (r < 0 || r > 2) continue;
        for (int wo = wi / 2; wo <= (wi + 1) / 2; ++wo) {
          if (wo >= Wo) continue;
          const int s = wi - (wo * 2 - 1);
          if (s < 0 || s > 2) continue;
          const size_t o = (((size_t)n * Ho + ho) * Wo + wo) * C + c;
          const char4 k = *reinterpret_cast<const char4*>(idx + o);
          const float4 g = *reinterpret_cast<const float4*>(dy + o);
          const int tap = r * 3 + s;
          if (k.x == tap) acc.x += g.x;
          if (k.y == tap) acc.y += g.y;
          if (k.z == tap) acc.z += g.z;
          if (k.w == tap) acc.w += g.w;
        }
      }
      stream_store(reinterpret_cast<float4*>(dx) + obase + e, acc);
    }
  }
}

// ---------------------------------------------------------------- bilinear x2 (align_corners=False)
// Workgroups are dealt round-robin over the 8 XCDs (private L2 each).  Neighbouring image rows share their source rows:
// give every XCD a CONTIGUOUS range of the logical block ids, so the shared rows are found in that XCD's L2.
// Launch with 8 * ceil(nblk / 8) blocks; ids >= nblk are padding.
__device__ __forceinline__ unsigned xcd_contiguous(unsigned b, unsigned nblk) {
  const unsigned per = (nblk + 7u) >> 3;
  return (b & 7u) * per + (b >> 3);
}

// One block = 256 consecutive float4 of ONE output row: the row decode is scalar (block-uniform), a lane only splits its
// element index into (column, channel quad) with 32-bit arithmetic.  (The first version decoded a flat 64-bit index per
// thread - three emulated 64-bit divisions - and ran at 1.2 TB/s.)
__global__ __launch_bounds__(256) void upsample2x_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C,
                                                             float* __restrict__ y, unsigned segs, unsigned nblk) {
  const unsigned C4 = (unsigned)C / 4, Ho = 2u * H, Wo = 2u * W;
  const unsigned bid = xcd_contiguous(blockIdx.x, nblk);
  if (bid >= nblk) return;
  const unsigned row = bid / segs, seg = bid - row * segs;                      // row = n * Ho + ho
  const unsigned n = row / Ho, ho = row - n * Ho;
  const unsigned e = seg * 256u + threadIdx.x;
  if (e >= Wo * C4) return;
  const unsigned wo = e / C4, c = (e - wo * C4) * 4u;
  const float sh = fmaxf(0.f, (ho + 0.5f) * 0.5f - 0.5f), sw = fmaxf(0.f, (wo + 0.5f) * 0.5f - 0.5f);
  const int h0 = (int)sh, w0 = (int)sw;
  const int h1 = min(h0 + 1, H - 1), w1 = min(w0 + 1, W - 1);
  const float lh = sh - h0, lw = sw - w0;
  const float* base = x + (size_t)n * H * W * C + c;
  const float4 a = *reinterpret_cast<const float4*>(base + ((size_t)h0 * W + w0) * C);
  const float4 b = *reinterpret_cast<const float4*>(base + ((size_t)h0 * W + w1) * C);
  const float4 cc = *reinterpret_cast<const float4*>(base + ((size_t)h1 * W + w0) * C);
  const float4 d = *reinterpret_cast<const float4*>(base + ((size_t)h1 * W + w1) * C);
  const float h0l = 1.f - lh, w0l = 1.f - lw;
  float4 o;
  o.x = h0l * (w0l * a.x + lw * b.x) + lh * (w0l * cc.x + lw * d.x);
  o.y = h0l * (w0l * a.y + lw * b.y) + lh * (w0l * cc.y + lw * d.y);
  o.z = h0l * (w0l * a.z + lw * b.z) + lh * (w0l * cc.z + lw * d.z);
  o.w = h0l * (w0l * a.w + lw * b.w) + lh * (w0l * cc.w + lw * d.w);
  stream_store(reinterpret_cast<float4*>(y + ((size_t)row * Wo + wo) * C + c), o);
}

// Adjoint of the x2 bilinear map.  Input i receives from outputs 2i-1 (0.25), 2i (0.75; 1 at i == 0), 2i+1 (0.75; 1 at
// i == last), 2i+2 (0.25): a lane owns one input pixel (4 channels) and gathers its 4 x 4 output taps - sixteen
// independent 16-byte loads from clamped addresses, taps outside the image carry weight 0.  Same block layout as the
// forward kernel (one block = 256 float4 of one input row).
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const float* __restrict__ dy, int N, int H, int W, int C,
                                                             float* __restrict__ dx, unsigned segs, unsigned nblk) {
  const unsigned C4 = (unsigned)C / 4;
  const int Ho = 2 * H, Wo = 2 * W;
  const unsigned bid = xcd_contiguous(blockIdx.x, nblk);
  if (bid >= nblk) return;
  const unsigned row = bid / segs, seg = bid - row * segs;                      // row = n * H + hi
  const unsigned n = row / (unsigned)H;
  const int hi = (int)(row - n * (unsigned)H);
  const unsigned e = seg * 256u + threadIdx.x;
  if (e >= (unsigned)W * C4) return;
  const int wi = (int)(e / C4);
  const unsigned c = (e - (unsigned)wi * C4) * 4u;
  const float wh[4] = {hi >= 1 ? 0.25f : 0.f, hi == 0 ? 1.f : 0.75f, hi == H - 1 ? 1.f : 0.75f, hi <= H - 2 ? 0.25f : 0.f};
  const float ww[4] = {wi >= 1 ? 0.25f : 0.f, wi == 0 ? 1.f : 0.75f, wi == W - 1 ? 1.f : 0.75f, wi <= W - 2 ? 0.25f : 0.f};
  const float* base = dy + (size_t)n * Ho * Wo * C + c;
  float4 g[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = min(max(2 * hi - 1 + k, 0), Ho - 1);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int q = min(max(2 * wi - 1 + l, 0), Wo - 1);
      g[k][l] = *reinterpret_cast<const float4*>(base + ((size_t)r * Wo + q) * C);
    }
  }
  float4 acc = make_float4(0, 0, 0, 0);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float4 tr = make_float4(0, 0, 0, 0);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      tr.x = fmaf(ww[l], g[k][l].x, tr.x); tr.y = fmaf(ww[l], g[k][l].y, tr.y);
      tr.z = fmaf(ww[l], g[k][l].z, tr.z); tr.w = fmaf(ww[l], g[k][l].w, tr.w);
    }
    acc.x = fmaf(wh[k], tr.x, acc.x); acc.y = fmaf(wh[k], tr.y, acc.y);
    acc.z = fmaf(wh[k], tr.z, acc.z); acc.w = fmaf(wh[k], tr.w, acc.w);
  }
  stream_store(reinterpret_cast<float4*>(dx + ((size_t)row * W + wi) * C + c), acc);
}

__global__ void sigmoid_fwd_kernel(const float* __restrict__ x, long n, float* __restrict__ y) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = 1.f / (1.f + __expf(-x[i]));
}
__global__ void sigmoid_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, long n, float* __restrict__ dx) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    dx[i] = dy[i] * y[i] * (1.f - y[i]);
}

}  // namespace xas

using namespace xas;

extern "C" int xas_maxpool3x3s2_fwd(const float* x, int N, int H, int W, int C, float* y, int8_t* idx, void* stream) {
  XAS_REQUIRE(x && y && idx && N > 0 && H > 0 && W > 0 && C % 4 == 0, "maxpool: bad arguments");
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  XAS_REQUIRE((long)N * H < 0x7fffffffl, "maxpool: too many rows");
  const long rows = (long)N * Ho;                               // one block per output row (grid-stride beyond 8 192 blocks)
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3((unsigned)(rows < 8192 ? rows : 8192)), dim3(256), 0, as_stream(stream), x, N, H, W, C, Ho,
                     Wo, y, idx);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_maxpool3x3s2_bwd(const float* dy, const int8_t* idx, int N, int H, int W, int C, float* dx,
                                    void* stream) {
  XAS_REQUIRE(dy && dx && idx && N > 0 && H > 0 && W > 0 && C % 4 == 0, "maxpool bwd: bad arguments");
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  XAS_REQUIRE((long)N * H < 0x7fffffffl, "maxpool bwd: too many rows");
  const long rows = (long)N * H;
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)(rows < 16384 ? rows : 16384)), dim3(256), 0, as_stream(stream), dy, idx, N, H,
                     W, C, Ho, Wo, dx);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_upsample2x_fwd(const float* x, int N, int H, int W, int C, float* y, void* stream) {
  XAS_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C % 4 == 0, "upsample2x: bad arguments");
  const long segs = cdiv((long)2 * W * (C / 4), 256), blocks = (long)N * 2 * H * segs;
  XAS_REQUIRE(blocks < 0x7ffffff0l && (long)N * 4 * H * W * C < (1l << 40), "upsample2x: tensor too large");
  hipLaunchKernelGGL(upsample2x_fwd_kernel, dim3((unsigned)(8 * cdiv(blocks, 8))), dim3(256), 0, as_stream(stream), x, N, H,
                     W, C, y, (unsigned)segs, (unsigned)blocks);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_upsample2x_bwd(const float* dy, int N, int H, int W, int C, float* dx, void* stream) {
  XAS_REQUIRE(dy && dx && N > 0 && H > 0 && W > 0 && C % 4 == 0, "upsample2x bwd: bad arguments");
  const long segs = cdiv((long)W * (C / 4), 256), blocks = (long)N * H * segs;
  XAS_REQUIRE(blocks < 0x7ffffff0l && (long)N * 4 * H * W * C < (1l << 40), "upsample2x bwd: tensor too large");
  hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3((unsigned)(8 * cdiv(blocks, 8))), dim3(256), 0, as_stream(stream), dy, N,
                     H, W, C, dx, (unsigned)segs, (unsigned)blocks);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_sigmoid_fwd(const float* x, long n, float* y, void* stream) {
  XAS_REQUIRE(x && y && n > 0, "sigmoid: bad arguments");
  hipLaunchKernelGGL(sigmoid_fwd_kernel, dim3(ew_grid(n)), dim3(256), 0, as_stream(stream), x, n, y);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_sigmoid_bwd(const float* y, const float* dy, long n, float* dx, void* stream) {
  XAS_REQUIRE(y && dy && dx && n > 0, "sigmoid bwd: bad arguments");
  hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, as_stream(stream), y, dy, n, dx);
  XAS_LAUNCH_CHECK();
  return 0;
}
