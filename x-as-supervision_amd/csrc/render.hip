// Z-buffered triangle rasteriser of the online pseudo-image path (xas_mesh_render, include/xas_hip.h): forward only, no
// atomics, a pure function of its inputs bit for bit.
//
// Two launches.  render_setup_kernel: one thread per (sample, face) writes the face's pixel box (8 bytes, scanned by every
// tile) and, for a face that can hit a pixel, a 64-byte record: vertices, shaded colour, signed area.  render_raster_kernel:
// one workgroup per (sample, 16x16 tile); it walks the boxes kChunk at a time, compacts the records of the faces whose box
// meets the tile into LDS IN FACE ORDER (ballot + wave prefix), and every thread then resolves its own pixel against that
// list before the next chunk is read - so no number of faces on one tile overflows anything, and the first face to reach
// the smallest depth, the one with the smallest index, keeps the pixel.
//
// Every decision (coverage, depth order) is taken in double precision with the operations and their order fixed below and
// in tests/_render_oracle.py; contraction to fused multiply-adds is switched off for the file so that the compiler keeps them.
#include "common.h"

#pragma clang fp contract(off)

namespace xas {
namespace {

constexpr int kTile = 16;                      // pixels per tile side; one thread per pixel
constexpr int kRasterThreads = kTile * kTile;
constexpr int kChunk = kRasterThreads;         // faces looked at per compaction round: one per thread
constexpr int kSetupThreads = 256;
constexpr int kMaxSize = 4096;                 // the box stores pixel indices in 16 bits
constexpr unsigned short kEmptyLo = 0xffffu;   // box.x0 of a face that hits no pixel: larger than any tile's last column

struct FaceBox { unsigned short x0, y0, x1, y1; };     // closed pixel range; x0 = kEmptyLo: skipped
struct FaceRec {
  float v[9];          // a, b, c: x px, y px, depth
  float rgb[3];        // shaded, rounded once
  double area;         // (b - a) x (c - a), never 0
  FaceBox box;
};
static_assert(sizeof(FaceBox) == 8 && sizeof(FaceRec) == 64 && alignof(FaceRec) == 8, "face record layout");

__host__ __device__ inline size_t boxes_bytes(long n) { return ((size_t)n * sizeof(FaceBox) + 63) / 64 * 64; }

// (q - p) x (s - p) for p = (px, py) ...: the edge function of the specification, five double operations in this order
__device__ __forceinline__ double edge(double px, double py, double qx, double qy, double sx, double sy) {
  return (qx - px) * (sy - py) - (qy - py) * (sx - px);
}

__global__ __launch_bounds__(kSetupThreads) void render_setup_kernel(
    const float* __restrict__ verts, const int* __restrict__ faces, const float* __restrict__ face_rgb,
    const float* __restrict__ light, float ambient, float depth_scale, int B, int Nv, int F, int S,
    FaceBox* __restrict__ boxes, FaceRec* __restrict__ recs) {
  const long i = (long)blockIdx.x * kSetupThreads + threadIdx.x;
  if (i >= (long)B * F) return;
  const int b = (int)(i / F), f = (int)(i % F);
  FaceBox box = {kEmptyLo, kEmptyLo, 0, 0};
  const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  bool ok = i0 >= 0 && i0 < Nv && i1 >= 0 && i1 < Nv && i2 >= 0 && i2 < Nv;
  float v[9];
  if (ok) {
    const float* vb = verts + (size_t)b * Nv * 3;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      v[e] = vb[(size_t)i0 * 3 + e];
      v[3 + e] = vb[(size_t)i1 * 3 + e];
      v[6 + e] = vb[(size_t)i2 * 3 + e];
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) ok = ok && isfinite(v[e]);
  }
  double area = 0.0;
  if (ok) {
    area = edge(v[0], v[1], v[3], v[4], v[6], v[7]);
    ok = area != 0.0;
  }
  if (ok) {                                             // pixel centres inside the closed box of the vertices, inside the patch
    const float lx = fmaxf(ceilf(fminf(fminf(v[0], v[3]), v[6])), 0.f), hx = fminf(floorf(fmaxf(fmaxf(v[0], v[3]), v[6])), (float)(S - 1));
    const float ly = fmaxf(ceilf(fminf(fminf(v[1], v[4]), v[7])), 0.f), hy = fminf(floorf(fmaxf(fmaxf(v[1], v[4]), v[7])), (float)(S - 1));
    ok = lx <= hx && ly <= hy;
    if (ok) box = {(unsigned short)lx, (unsigned short)ly, (unsigned short)hx, (unsigned short)hy};
  }
  boxes[i] = box;
  if (!ok) return;
  // flat shade: unit normal of the triangle in (x, y, depth * depth_scale), turned towards the viewer (negative depth part)
  const double ds = (double)depth_scale;
  const double e1x = (double)v[3] - (double)v[0], e1y = (double)v[4] - (double)v[1], e1z = ((double)v[5] - (double)v[2]) * ds;
  const double e2x = (double)v[6] - (double)v[0], e2y = (double)v[7] - (double)v[1], e2z = ((double)v[8] - (double)v[2]) * ds;
  double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  if (nz > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
  const double nl = sqrt((nx * nx + ny * ny) + nz * nz);
  double lx = 0.0, ly = 0.0, lz = -1.0;
  if (light) {
    lx = (double)light[0]; ly = (double)light[1]; lz = (double)light[2];
    const double ll = sqrt((lx * lx + ly * ly) + lz * lz);
    lx = lx / ll; ly = ly / ll; lz = lz / ll;
  }
  const double d = ((nx / nl) * lx + (ny / nl) * ly) + (nz / nl) * lz;
  const double shade = (double)ambient + (1.0 - (double)ambient) * (d > 0.0 ? d : 0.0);      // NaN counts as unlit
  FaceRec r;
#pragma unroll
  for (int e = 0; e < 9; ++e) r.v[e] = v[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) r.rgb[e] = (float)((face_rgb ? (double)face_rgb[f * 3 + e] : 1.0) * shade);
  r.area = area;
  r.box = box;
  recs[i] = r;
}

__global__ __launch_bounds__(kRasterThreads) void render_raster_kernel(
    const FaceBox* __restrict__ boxes, const FaceRec* __restrict__ recs, float background, int F, int S, int tiles_x,
    float* __restrict__ img, float* __restrict__ mask, float* __restrict__ zbuf, int* __restrict__ face_id) {
  __shared__ float4 s_rec[kChunk * 4];          // the compacted records of this round (64 bytes each)
  __shared__ int s_fid[kChunk];
  __shared__ int s_cnt[kRasterThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, tx0 = (blockIdx.x % tiles_x) * kTile, ty0 = (blockIdx.x / tiles_x) * kTile;
  const int tx1 = tx0 + kTile - 1, ty1 = ty0 + kTile - 1;
  const int px = tx0 + (tid & (kTile - 1)), py = ty0 + tid / kTile;
  const bool inside = px < S && py < S;
  const double dpx = (double)px, dpy = (double)py;
  const FaceBox* bx = boxes + (size_t)b * F;
  const float4* rc = reinterpret_cast<const float4*>(recs + (size_t)b * F);

  double best = __longlong_as_double(0x7ff0000000000000LL);   // +inf
  int best_f = -1;
  float cr = background, cg = background, cb = background;

  for (int base = 0; base < F; base += kChunk) {
    const int f = base + tid;
    bool hit = false;
    if (f < F) {
      const FaceBox q = bx[f];
      hit = q.x0 <= tx1 && q.x1 >= tx0 && q.y0 <= ty1 && q.y1 >= ty0;      // kEmptyLo fails the first test on every tile
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = __popcll(m & ((1ull << lane) - 1ull)), n = 0;
#pragma unroll
    for (int w = 0; w < kRasterThreads / 64; ++w) {
      const int c = s_cnt[w];
      off += w < wave ? c : 0;
      n += c;
    }
    if (hit) {                                   // off < n <= kChunk
#pragma unroll
      for (int e = 0; e < 4; ++e) s_rec[off * 4 + e] = rc[(size_t)f * 4 + e];
      s_fid[off] = f;
    }
    __syncthreads();
    if (inside) {
      const FaceRec* list = reinterpret_cast<const FaceRec*>(s_rec);
      for (int j = 0; j < n; ++j) {
        const FaceRec& r = list[j];
        if (px < (int)r.box.x0 || px > (int)r.box.x1 || py < (int)r.box.y0 || py > (int)r.box.y1) continue;
        const double ax = r.v[0], ay = r.v[1], bx_ = r.v[3], by = r.v[4], cx = r.v[6], cy = r.v[7];
        const double w0 = edge(bx_, by, cx, cy, dpx, dpy);     // (c - b) x (p - b): weight of a
        const double w1 = edge(cx, cy, ax, ay, dpx, dpy);      // (a - c) x (p - c): weight of b
        const double w2 = edge(ax, ay, bx_, by, dpx, dpy);     // (b - a) x (p - a): weight of c
        const double area = r.area;
        const bool cov = area > 0.0 ? (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) : (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0);
        if (!cov) continue;
        const double z = ((w0 * (double)r.v[2] + w1 * (double)r.v[5]) + w2 * (double)r.v[8]) / area;
        if (z < best) {                          // strict: of equal depths the first, the smaller face index, stays
          best = z;
          best_f = s_fid[j];
          cr = r.rgb[0]; cg = r.rgb[1]; cb = r.rgb[2];
        }
      }
    }
    // the next round's first barrier orders these reads before its writes to s_rec; s_cnt is rewritten only after this
    // round's second barrier, which every thread passed after reading it
  }
  if (!inside) return;
  const size_t plane = (size_t)S * S, pix = (size_t)py * S + px;
  float* ib = img + (size_t)b * 3 * plane + pix;
  ib[0] = cr; ib[plane] = cg; ib[2 * plane] = cb;
  mask[(size_t)b * plane + pix] = best_f >= 0 ? 1.f : 0.f;
  if (zbuf) zbuf[(size_t)b * plane + pix] = (float)best;
  if (face_id) face_id[(size_t)b * plane + pix] = best_f;
}

}  // namespace
}  // namespace xas

using namespace xas;

extern "C" size_t xas_mesh_render_workspace_bytes(int B, int F, int S) {
  if (B <= 0 || F <= 0 || S <= 0) return 0;
  return boxes_bytes((long)B * F) + (size_t)B * F * sizeof(FaceRec);
}

extern "C" int xas_mesh_render(const float* verts, const int* faces, const float* face_rgb, const float* light, float ambient,
                               float depth_scale, float background, int B, int Nv, int F, int S, float* img, float* mask,
                               float* zbuf, int* face_id, void* workspace, void* stream) {
  XAS_REQUIRE(S > 0 && S <= kMaxSize, "mesh_render: S=%d (needs 1 <= S <= %d)", S, kMaxSize);
  XAS_REQUIRE(B >= 0 && F >= 0 && Nv >= 0, "mesh_render: bad shape B=%d Nv=%d F=%d (none may be negative)", B, Nv, F);
  XAS_REQUIRE(B <= 65535 && (long)B * F < 0x7fffffffL, "mesh_render: B=%d F=%d (needs B <= 65535 and B*F < 2^31)", B, F);
  if (B == 0) return 0;
  XAS_REQUIRE(img && mask, "mesh_render: null buffer (img and mask are required)");
  XAS_REQUIRE(F == 0 || (faces && (verts || Nv == 0)), "mesh_render: null buffer (verts and faces are required with F=%d)", F);
  XAS_REQUIRE(F == 0 || workspace, "mesh_render: null workspace with B=%d F=%d (xas_mesh_render_workspace_bytes)", B, F);
  XAS_REQUIRE(((uintptr_t)workspace & 15) == 0, "mesh_render: the workspace must be 16-byte aligned");
  FaceBox* boxes = reinterpret_cast<FaceBox*>(workspace);
  FaceRec* recs = reinterpret_cast<FaceRec*>(reinterpret_cast<char*>(workspace) + boxes_bytes((long)B * F));
  if (F > 0) {
    hipLaunchKernelGGL(render_setup_kernel, dim3((unsigned)cdiv((long)B * F, kSetupThreads)), dim3(kSetupThreads), 0,
                       as_stream(stream), verts, faces, face_rgb, light, ambient, depth_scale, B, Nv, F, S, boxes, recs);
    XAS_LAUNCH_CHECK();
  }
  const int tiles = (int)cdiv(S, kTile);
  hipLaunchKernelGGL(render_raster_kernel, dim3(tiles * tiles, B), dim3(kRasterThreads), 0, as_stream(stream), boxes, recs,
                     background, F, S, tiles, img, mask, zbuf, face_id);
  XAS_LAUNCH_CHECK();
  return 0;
}
