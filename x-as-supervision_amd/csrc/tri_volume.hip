// Volumetric multi-view fusion on the device (gfx950), one kernel:
//   triangulate_volume : product of the views' heat-map distributions over a voxel grid round the triangulated point, and its
//                     soft-argmax in world space (no reference counterpart: eval.py --tri-volume; xas_hip.h has the arithmetic)
// One workgroup of 256 threads per (b, joint).  The camera constants of the workgroup's sample sit in LDS as doubles, one
// VolView per view, written once by thread v.  Per level the G^3 voxels are strided over the threads; every thread keeps an
// online-softmax record (VolRec) of its voxels, the records of a wave merge by a butterfly of shuffles (the merge is
// symmetric bit for bit, so every lane ends with the same record), the four waves' records through LDS in wave order by
// thread 0, which also moves the centre for the next level.  No atomics: the result is a pure function of the inputs.
// A sample reads the 2x2x2 logits round its clamped point as four pairs: the two depth neighbours are adjacent floats.
#include "multiview.h"

namespace xas {

constexpr int kVolThreads = 256, kVolWaves = kVolThreads / 64;

struct VolCubes {
  const float* p[XAS_TRI_MAX_VIEWS];
};

struct VolView {
  double r[9], t[3], fx, fy, cx, cy, a[4], ta[2], pz, wt;
  size_t off;                                                         // of (b, channel chan) in the view's logits, in floats
  int take;
};

// Online-softmax record of a set of voxels: m = the largest score, s = sum of e = exp(score - m), x = sum of e * d and
// xx = sum of e * d d^T with d the voxel's offset from the level's centre, best / arg = the first voxel of the largest score,
// bad = a logit that is not finite was read.
struct VolRec {
  double m, s, x[3], xx[6], best;
  int arg, bad;
};

__device__ __forceinline__ void vol_merge(VolRec& a, const VolRec& b) {
  const double m = a.m > b.m ? a.m : b.m;
  const double fa = a.m == m ? 1.0 : exp(a.m - m), fb = b.m == m ? 1.0 : exp(b.m - m);   // (-inf) - (-inf) never formed
  a.m = m;
  a.s = a.s * fa + b.s * fb;
#pragma unroll
  for (int n = 0; n < 3; ++n) a.x[n] = a.x[n] * fa + b.x[n] * fb;
#pragma unroll
  for (int n = 0; n < 6; ++n) a.xx[n] = a.xx[n] * fa + b.xx[n] * fb;
  if (b.best > a.best || (b.best == a.best && b.arg < a.arg)) { a.best = b.best; a.arg = b.arg; }
  a.bad |= b.bad;
}

__device__ __forceinline__ VolRec vol_wave_merge(VolRec r) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    VolRec q;
    q.m = __shfl_xor(r.m, o, 64); q.s = __shfl_xor(r.s, o, 64); q.best = __shfl_xor(r.best, o, 64);
#pragma unroll
    for (int n = 0; n < 3; ++n) q.x[n] = __shfl_xor(r.x[n], o, 64);
#pragma unroll
    for (int n = 0; n < 6; ++n) q.xx[n] = __shfl_xor(r.xx[n], o, 64);
    q.arg = __shfl_xor(r.arg, o, 64); q.bad = __shfl_xor(r.bad, o, 64);
    vol_merge(r, q);
  }
  return r;
}

// Clamp to [0, top]; NaN goes to 0, so the cell index is in range whatever the cameras hold.
__device__ __forceinline__ double vol_clamp(double c, double top) {
  const double lo = c > 0.0 ? c : 0.0;
  return lo < top ? lo : top;
}

// sample_v(X) of the header: the trilinear logit at the clamped cube point of X minus pen * (cells the clamp removed).
__device__ __forceinline__ double vol_sample(const VolView& c, const float* __restrict__ cube, const double (&X)[3], int D,
                                             size_t KD, double cell_xy, double cell_z, double pen, int& bad) {
  const double xc = c.r[0] * X[0] + c.r[1] * X[1] + c.r[2] * X[2] + c.t[0];
  const double yc = c.r[3] * X[0] + c.r[4] * X[1] + c.r[5] * X[2] + c.t[1];
  const double zc = c.r[6] * X[0] + c.r[7] * X[1] + c.r[8] * X[2] + c.t[2];
  const double top = (double)(D - 1);
  double w = 0.0, h = 0.0, d = 0.0, o = 3.0 * (double)D;
  if (zc > 0.0) {
    const double u = c.fx * xc / zc + c.cx, v = c.fy * yc / zc + c.cy;
    const double pw = (c.a[0] * u + c.a[1] * v + c.ta[0]) * cell_xy, ph = (c.a[2] * u + c.a[3] * v + c.ta[1]) * cell_xy;
    const double pd = ((zc - c.pz) * cell_z + 1.0) * (0.5 * (double)D);
    w = vol_clamp(pw, top); h = vol_clamp(ph, top); d = vol_clamp(pd, top);
    o = fabs(pw - w) + fabs(ph - h) + fabs(pd - d);
  }
  const int w0 = min((int)w, D - 2), h0 = min((int)h, D - 2), d0 = min((int)d, D - 2);   // w, h, d in [0, D - 1]: floor
  const double fw = w - (double)w0, fh = h - (double)h0, fd = d - (double)d0;
  const float* p = cube + c.off + ((size_t)h0 * D + w0) * KD + d0;
  float q[4][2];
  __builtin_memcpy(q[0], p, 8);
  __builtin_memcpy(q[1], p + KD, 8);
  __builtin_memcpy(q[2], p + (size_t)D * KD, 8);
  __builtin_memcpy(q[3], p + (size_t)D * KD + KD, 8);
  double l[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    bad |= !(fabsf(q[n][0]) < INFINITY) | !(fabsf(q[n][1]) < INFINITY);
    l[n] = (1.0 - fd) * (double)q[n][0] + fd * (double)q[n][1];
  }
  const double l0 = (1.0 - fw) * l[0] + fw * l[1], l1 = (1.0 - fw) * l[2] + fw * l[3];
  return (1.0 - fh) * l0 + fh * l1 - pen * o;
}

__global__ __launch_bounds__(kVolThreads) void triangulate_volume_kernel(
    VolCubes cubes, const int* __restrict__ chan, const float* __restrict__ ti, const float* __restrict__ km,
    const float* __restrict__ pv, const float* __restrict__ rw, const float* __restrict__ tw, const float* __restrict__ init,
    const unsigned char* __restrict__ views, const float* __restrict__ weight, int B, int V, int K, int D, int G, int levels,
    float side_mm, float beta_, float pen_, float S_, float rect_, float* __restrict__ xyz, float* __restrict__ cov,
    unsigned char* __restrict__ status) {
  __shared__ VolView sh_view[XAS_TRI_MAX_VIEWS];
  __shared__ VolRec sh_rec[kVolWaves];
  __shared__ double sh_centre[3];
  __shared__ int sh_bad;
  const int i = blockIdx.x, b = i / K, k = i % K, tid = threadIdx.x;
  const size_t KD = (size_t)K * D;
  if (tid < V) {                                                      // thread v: the constants of view v for this sample
    const int v = tid;
    const size_t vb = (size_t)v * B + b;
    VolView& c = sh_view[v];
    const int ch = chan ? chan[vb * K + k] : k;
    const float wt = weight ? weight[vb * K + k] : 1.f;
    const bool sel = !views || ((views[i] >> v) & 1);
    c.take = sel && view_valid(wt) && ch >= 0 && ch < K;
    c.wt = (double)wt;
    c.off = (size_t)b * D * D * KD + (size_t)(c.take ? ch : 0) * D;
#pragma unroll
    for (int n = 0; n < 9; ++n) c.r[n] = (double)rw[vb * 9 + n];
#pragma unroll
    for (int n = 0; n < 3; ++n) c.t[n] = (double)tw[vb * 3 + n];
    c.fx = (double)km[vb * 9]; c.fy = (double)km[vb * 9 + 4]; c.cx = (double)km[vb * 9 + 2]; c.cy = (double)km[vb * 9 + 5];
    c.a[0] = (double)ti[vb * 6]; c.a[1] = (double)ti[vb * 6 + 1]; c.ta[0] = (double)ti[vb * 6 + 2];
    c.a[2] = (double)ti[vb * 6 + 3]; c.a[3] = (double)ti[vb * 6 + 4]; c.ta[1] = (double)ti[vb * 6 + 5];
    c.pz = (double)pv[vb * 3 + 2];
  }
  const float x0 = init[(size_t)i * 3], x1 = init[(size_t)i * 3 + 1], x2 = init[(size_t)i * 3 + 2];
  if (tid == 0) {
    sh_centre[0] = (double)x0; sh_centre[1] = (double)x1; sh_centre[2] = (double)x2;
    sh_bad = 0;
  }
  __syncthreads();
  int ntake = 0;
  for (int v = 0; v < V; ++v) ntake += sh_view[v].take;
  const bool finite = fabsf(x0) < INFINITY && fabsf(x1) < INFINITY && fabsf(x2) < INFINITY;
  int st = (ntake >= 2 && finite) ? 0 : 1;                            // everything up to here is uniform over the workgroup
  VolRec total = {};
  const double S = (double)S_, cell_xy = (double)D / (S - 1.0), cell_z = S / (double)rect_ / (S - 1.0);
  const double beta = (double)beta_, pen = (double)pen_;
  const int G3 = G * G * G;
  double side = (double)side_mm, centre[3] = {0.0, 0.0, 0.0};
  for (int lvl = 0; st == 0 && lvl < levels; ++lvl, side *= 0.5) {
#pragma unroll
    for (int n = 0; n < 3; ++n) centre[n] = sh_centre[n];
    VolRec rec = {};
    rec.m = -INFINITY; rec.best = -INFINITY; rec.arg = G3;
    for (int idx = tid; idx < G3; idx += kVolThreads) {
      const int ix = idx % G, iy = (idx / G) % G, iz = idx / (G * G);
      const double d[3] = {(((double)ix + 0.5) / (double)G - 0.5) * side, (((double)iy + 0.5) / (double)G - 0.5) * side,
                           (((double)iz + 0.5) / (double)G - 0.5) * side};
      const double X[3] = {centre[0] + d[0], centre[1] + d[1], centre[2] + d[2]};
      double score = 0.0;
      for (int v = 0; v < V; ++v)
        if (sh_view[v].take) score += sh_view[v].wt * vol_sample(sh_view[v], cubes.p[v], X, D, KD, cell_xy, cell_z, pen, rec.bad);
      score *= beta;
      if (score > rec.best) { rec.best = score; rec.arg = idx; }
      double e = 1.0;
      if (score > rec.m) {                                            // the sums so far move to the new maximum
        const double f = exp(rec.m - score);                          // exp(-inf) = 0 at the first voxel
        rec.m = score;
        rec.s *= f;
#pragma unroll
        for (int n = 0; n < 3; ++n) rec.x[n] *= f;
#pragma unroll
        for (int n = 0; n < 6; ++n) rec.xx[n] *= f;
      } else {
        e = exp(score - rec.m);
      }
      rec.s += e;
#pragma unroll
      for (int n = 0; n < 3; ++n) rec.x[n] += e * d[n];
      rec.xx[0] += e * d[0] * d[0]; rec.xx[1] += e * d[0] * d[1]; rec.xx[2] += e * d[0] * d[2];
      rec.xx[3] += e * d[1] * d[1]; rec.xx[4] += e * d[1] * d[2]; rec.xx[5] += e * d[2] * d[2];
    }
    rec = vol_wave_merge(rec);
    if ((tid & 63) == 0) sh_rec[tid >> 6] = rec;
    __syncthreads();
    if (tid == 0) {
      VolRec t = sh_rec[0];
      for (int wv = 1; wv < kVolWaves; ++wv) vol_merge(t, sh_rec[wv]);
      sh_rec[0] = t;
      sh_bad = t.bad;
#pragma unroll
      for (int n = 0; n < 3; ++n) sh_centre[n] = centre[n] + t.x[n] / t.s;    // the next level's centre, in double
    }
    __syncthreads();
    total = sh_rec[0];
    if (sh_bad) st = 3;
    __syncthreads();                                                  // sh_rec is written again at the next level
  }
  if (tid != 0) return;
  float* o = xyz + (size_t)i * 3;
  if (st != 0) {                                                      // passed through: init bit for bit, NaN stays NaN
    o[0] = x0; o[1] = x1; o[2] = x2;
    if (cov)
      for (int n = 0; n < 6; ++n) cov[(size_t)i * 6 + n] = NAN;
    if (status) status[i] = (unsigned char)st;
    return;
  }
  const double mean[3] = {total.x[0] / total.s, total.x[1] / total.s, total.x[2] / total.s};
#pragma unroll
  for (int n = 0; n < 3; ++n) o[n] = (float)(centre[n] + mean[n]);
  if (cov) {
    float* cv = cov + (size_t)i * 6;
    cv[0] = (float)(total.xx[0] / total.s - mean[0] * mean[0]); cv[1] = (float)(total.xx[1] / total.s - mean[0] * mean[1]);
    cv[2] = (float)(total.xx[2] / total.s - mean[0] * mean[2]); cv[3] = (float)(total.xx[3] / total.s - mean[1] * mean[1]);
    cv[4] = (float)(total.xx[4] / total.s - mean[1] * mean[2]); cv[5] = (float)(total.xx[5] / total.s - mean[2] * mean[2]);
  }
  const int ix = total.arg % G, iy = (total.arg / G) % G, iz = total.arg / (G * G);
  const bool face = ix == 0 || ix == G - 1 || iy == 0 || iy == G - 1 || iz == 0 || iz == G - 1;
  if (status) status[i] = face ? 2 : 0;
}

}  // namespace xas

using namespace xas;

extern "C" int xas_triangulate_volume(const float* const* logits, const int* chan, const float* trans_image, const float* k_mat,
                                      const float* pelvis, const float* rot_world, const float* trans_world, const float* init,
                                      const unsigned char* views, const float* weight, int B, int V, int K, int D, int G,
                                      int levels, float side_mm, float beta, float out_penalty, float image_size,
                                      float rect_width, float* xyz, float* cov, unsigned char* status, void* stream) {
  XAS_REQUIRE(logits && trans_image && k_mat && pelvis && rot_world && trans_world && init && xyz,
              "triangulate_volume: null buffer (logits, the five camera arrays, init and xyz are required)");
  XAS_REQUIRE(D >= 4 && D <= 128 && D % 4 == 0, "triangulate_volume: D=%d cells per side (needs a multiple of 4 in [4,128], the head's range)", D);
  if (tri_check_views("triangulate_volume", V, 1)) return 1;
  XAS_REQUIRE(G >= 2 && G <= 32, "triangulate_volume: G=%d voxels per side (needs 2 <= G <= 32)", G);
  XAS_REQUIRE(levels >= 1 && levels <= 4, "triangulate_volume: levels=%d (needs 1 <= levels <= 4)", levels);
  XAS_REQUIRE(side_mm > 0.f && side_mm < INFINITY, "triangulate_volume: side_mm %f (needs a finite side > 0 mm)", (double)side_mm);
  XAS_REQUIRE(beta > 0.f && beta < INFINITY, "triangulate_volume: beta %f (needs a finite beta > 0)", (double)beta);
  XAS_REQUIRE(out_penalty > 0.f && out_penalty < INFINITY, "triangulate_volume: out_penalty %f (needs a finite out_penalty > 0)",
              (double)out_penalty);
  if (tri_check_shape("triangulate_volume", B, K, "B > 0, K >= 1")) return 1;
  XAS_REQUIRE(image_size > 1.f && image_size < INFINITY && rect_width > 0.f && rect_width < INFINITY,
              "triangulate_volume: image_size %f, rect_width %f (needs a patch size > 1 and a depth range > 0)", (double)image_size,
              (double)rect_width);
  VolCubes cubes = {};
  for (int v = 0; v < V; ++v) {
    XAS_REQUIRE(logits[v], "triangulate_volume: logits[%d] is null (a host array of V = %d device pointers)", v, V);
    cubes.p[v] = logits[v];
  }
  hipLaunchKernelGGL(triangulate_volume_kernel, dim3((unsigned)((long)B * K)), dim3(kVolThreads), 0, as_stream(stream), cubes, chan,
                     trans_image, k_mat, pelvis, rot_world, trans_world, init, views, weight, B, V, K, D, G, levels, side_mm, beta,
                     out_penalty, image_size, rect_width, xyz, cov, status);
  XAS_LAUNCH_CHECK();
  return 0;
}
