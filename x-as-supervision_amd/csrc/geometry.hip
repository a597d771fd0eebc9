// Patch->world geometry and the fused line-mask renderer (max over lines).  gfx950.
//
// patch_to_world : modules/util.py:128-152 -> :61-95, all hypotheses in one launch, with
//                  closed-form 2x2 / 3x3 inverses instead of two batched LU solves.
// world_to_patch : modules/util.py:155-168 -> :116-125, :98-113, the other direction, with the optional row-vector
//                  rotation, scale and pelvis shift of project_smpl_to_patch_kps (:356-383, :343-352) in front of it.
// draw_lines_max : modules/util.py:21-59 + torch.max(dim=1) at modules/model.py:94,96.
//                  max_l exp(e_l) == exp(max_l e_l): one exp per pixel, nothing but the
//                  [B,1,S,S] mask ever reaches HBM (the reference keeps ten 419 MB
//                  intermediates for autograd).  Backward recomputes the winner line.
#include <float.h>

#include "common.h"

namespace xas {

struct CamParams {
  float i00, i01, i10, i11, t0, t1;   // inverse crop affine, translation
  float fx, fy, cx, cy, pz;           // intrinsics, pelvis depth
  float r[9];                         // R^-1 row-major
  float tw[3];
};

__device__ __forceinline__ CamParams load_cam(const float* ti, const float* km, const float* pv, const float* rw,
                                              const float* tw, int b, bool full = true) {
  CamParams c;
  const float* A = ti + b * 6;
  const float a00 = A[0], a01 = A[1], a10 = A[3], a11 = A[4];
  const float det = a00 * a11 - a01 * a10;
  c.i00 = a11 / det; c.i01 = -a01 / det; c.i10 = -a10 / det; c.i11 = a00 / det;
  c.t0 = A[2]; c.t1 = A[5];
  c.pz = pv[b * 3 + 2];
  if (!full) return c;                               // XAS_GEO_IMAGE: intrinsics / extrinsics are not needed (may be NULL)
  const float* Kc = km + b * 9;
  c.fx = Kc[0]; c.fy = Kc[4]; c.cx = Kc[2]; c.cy = Kc[5];
  const float* R = rw + b * 9;
  const float m00 = R[4] * R[8] - R[5] * R[7], m01 = R[2] * R[7] - R[1] * R[8], m02 = R[1] * R[5] - R[2] * R[4];
  const float m10 = R[5] * R[6] - R[3] * R[8], m11 = R[0] * R[8] - R[2] * R[6], m12 = R[2] * R[3] - R[0] * R[5];
  const float m20 = R[3] * R[7] - R[4] * R[6], m21 = R[1] * R[6] - R[0] * R[7], m22 = R[0] * R[4] - R[1] * R[3];
  const float d3 = R[0] * m00 + R[1] * m10 + R[2] * m20;
  c.r[0] = m00 / d3; c.r[1] = m01 / d3; c.r[2] = m02 / d3;
  c.r[3] = m10 / d3; c.r[4] = m11 / d3; c.r[5] = m12 / d3;
  c.r[6] = m20 / d3; c.r[7] = m21 / d3; c.r[8] = m22 / d3;
  c.tw[0] = tw[b * 3]; c.tw[1] = tw[b * 3 + 1]; c.tw[2] = tw[b * 3 + 2];
  return c;
}

__global__ void patch_to_world_fwd_kernel(const float* __restrict__ kps, const float* ti, const float* km,
                                          const float* pv, const float* rw, const float* tw, int B, int HK,
                                          float S, float rect, int flags, float* __restrict__ world) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * HK) return;
  const int b = i / HK;
  const CamParams c = load_cam(ti, km, pv, rw, tw, b, !(flags & XAS_GEO_IMAGE));
  float p0 = kps[i * 3], p1 = kps[i * 3 + 1], p2 = kps[i * 3 + 2];
  if (flags & XAS_GEO_PATCH) {
    if (flags & XAS_GEO_NORM) {
      p0 = (p0 + 1.f) / 2.f * (S - 1.f);
      p1 = (p1 + 1.f) / 2.f * (S - 1.f);
      p2 = p2 * (S - 1.f);
    }
    const float du = p0 - c.t0, dv = p1 - c.t1;
    p0 = c.i00 * du + c.i01 * dv;
    p1 = c.i10 * du + c.i11 * dv;
    p2 = p2 * (1.0f / S * rect) + c.pz;
  }
  if (flags & XAS_GEO_IMAGE) {                       // patch -> image only (triangulation input, util.py:180-182)
    world[i * 3] = p0; world[i * 3 + 1] = p1; world[i * 3 + 2] = p2;
    return;
  }
  float o0, o1, o2;
  if (flags & XAS_GEO_MONO) {
    o0 = -p0; o1 = -(p2 + 128.f); o2 = -p1;
  } else {
    const float q0 = (p0 - c.cx) / c.fx * p2 - c.tw[0];
    const float q1 = (p1 - c.cy) / c.fy * p2 - c.tw[1];
    const float q2 = p2 - c.tw[2];
    o0 = c.r[0] * q0 + c.r[1] * q1 + c.r[2] * q2;
    o1 = c.r[3] * q0 + c.r[4] * q1 + c.r[5] * q2;
    o2 = c.r[6] * q0 + c.r[7] * q1 + c.r[8] * q2;
  }
  world[i * 3] = o0; world[i * 3 + 1] = o1; world[i * 3 + 2] = o2;
}

__global__ void patch_to_world_bwd_kernel(const float* __restrict__ kps, const float* __restrict__ gw, const float* ti,
                                          const float* km, const float* pv, const float* rw, const float* tw, int B,
                                          int HK, float S, float rect, int flags, float* __restrict__ gk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * HK) return;
  const int b = i / HK;
  const CamParams c = load_cam(ti, km, pv, rw, tw, b);
  float p0 = kps[i * 3], p1 = kps[i * 3 + 1], p2 = kps[i * 3 + 2];
  if (flags & XAS_GEO_PATCH) {
    if (flags & XAS_GEO_NORM) {
      p0 = (p0 + 1.f) / 2.f * (S - 1.f);
      p1 = (p1 + 1.f) / 2.f * (S - 1.f);
      p2 = p2 * (S - 1.f);
    }
    const float du = p0 - c.t0, dv = p1 - c.t1;
    p0 = c.i00 * du + c.i01 * dv;
    p1 = c.i10 * du + c.i11 * dv;
    p2 = p2 * (1.0f / S * rect) + c.pz;
  }
  const float g0 = gw[i * 3], g1 = gw[i * 3 + 1], g2 = gw[i * 3 + 2];
  float d0, d1, d2;      // gradient w.r.t. (p0,p1,p2) after the patch stage
  if (flags & XAS_GEO_MONO) {
    d0 = -g0; d2 = -g1; d1 = -g2;
  } else {
    const float q0 = c.r[0] * g0 + c.r[3] * g1 + c.r[6] * g2;
    const float q1 = c.r[1] * g0 + c.r[4] * g1 + c.r[7] * g2;
    const float q2 = c.r[2] * g0 + c.r[5] * g1 + c.r[8] * g2;
    d0 = q0 * p2 / c.fx;
    d1 = q1 * p2 / c.fy;
    d2 = q0 * (p0 - c.cx) / c.fx + q1 * (p1 - c.cy) / c.fy + q2;
  }
  if (flags & XAS_GEO_PATCH) {
    const float e0 = c.i00 * d0 + c.i10 * d1;
    const float e1 = c.i01 * d0 + c.i11 * d1;
    d0 = e0; d1 = e1;
    d2 = d2 * (1.0f / S * rect);
    if (flags & XAS_GEO_NORM) {
      d0 *= (S - 1.f) / 2.f; d1 *= (S - 1.f) / 2.f; d2 *= (S - 1.f);
    }
  }
  gk[i * 3] = d0; gk[i * 3 + 1] = d1; gk[i * 3 + 2] = d2;
}

// ------------------------------------------------------------------ world -> patch
struct ProjParams {
  float a00, a01, a10, a11, t0, t1;   // crop affine (forward)
  float fx, fy, cx, cy, pz;           // intrinsics, pelvis depth
  float r[9];                         // rot_world row-major
  float tw[3];
  float pw[3];                        // pelvis in world coordinates (pelvis_origin), else 0
  float g[9];                         // pre_rot row-major (has_rot)
};

__device__ __forceinline__ ProjParams load_proj(const float* pre_rot, int pelvis_origin, const float* ti, const float* km,
                                                const float* pv, const float* rw, const float* tw, int b, int flags) {
  ProjParams c;
  const float* R = rw + b * 9;
#pragma unroll
  for (int e = 0; e < 9; ++e) c.r[e] = R[e];
  c.tw[0] = tw[b * 3]; c.tw[1] = tw[b * 3 + 1]; c.tw[2] = tw[b * 3 + 2];
  const float* Kc = km + b * 9;
  c.fx = Kc[0]; c.fy = Kc[4]; c.cx = Kc[2]; c.cy = Kc[5];
  c.a00 = c.a11 = 1.f; c.a01 = c.a10 = c.t0 = c.t1 = 0.f; c.pz = 0.f;
  if (!(flags & (XAS_GEO_IMAGE | XAS_GEO_WORLD))) {
    const float* A = ti + b * 6;
    c.a00 = A[0]; c.a01 = A[1]; c.t0 = A[2]; c.a10 = A[3]; c.a11 = A[4]; c.t1 = A[5];
    c.pz = pv[b * 3 + 2];
  }
  c.pw[0] = c.pw[1] = c.pw[2] = 0.f;
  if (pelvis_origin) {                                 // inv(rot_world) (pelvis - trans_world), adjugate / determinant (util.py:350)
    const float m00 = R[4] * R[8] - R[5] * R[7], m01 = R[2] * R[7] - R[1] * R[8], m02 = R[1] * R[5] - R[2] * R[4];
    const float m10 = R[5] * R[6] - R[3] * R[8], m11 = R[0] * R[8] - R[2] * R[6], m12 = R[2] * R[3] - R[0] * R[5];
    const float m20 = R[3] * R[7] - R[4] * R[6], m21 = R[1] * R[6] - R[0] * R[7], m22 = R[0] * R[4] - R[1] * R[3];
    const float d3 = R[0] * m00 + R[1] * m10 + R[2] * m20;
    const float q0 = pv[b * 3] - c.tw[0], q1 = pv[b * 3 + 1] - c.tw[1], q2 = pv[b * 3 + 2] - c.tw[2];
    c.pw[0] = m00 / d3 * q0 + m01 / d3 * q1 + m02 / d3 * q2;
    c.pw[1] = m10 / d3 * q0 + m11 / d3 * q1 + m12 / d3 * q2;
    c.pw[2] = m20 / d3 * q0 + m21 / d3 * q1 + m22 / d3 * q2;
  }
  if (pre_rot) {
#pragma unroll
    for (int e = 0; e < 9; ++e) c.g[e] = pre_rot[b * 9 + e];
  }
  return c;
}

// steps 1-2: (p . pre_rot) * pre_scale + pelvis_world  (row vector times matrix, torch.bmm(joints, global_rot), util.py:376-380)
__device__ __forceinline__ void to_world(const ProjParams& c, bool has_rot, float scale, float& p0, float& p1, float& p2) {
  if (has_rot) {
    const float q0 = (p0 * c.g[0] + p1 * c.g[3] + p2 * c.g[6]) * scale;
    const float q1 = (p0 * c.g[1] + p1 * c.g[4] + p2 * c.g[7]) * scale;
    const float q2 = (p0 * c.g[2] + p1 * c.g[5] + p2 * c.g[8]) * scale;
    p0 = q0; p1 = q1; p2 = q2;
  }
  p0 += c.pw[0]; p1 += c.pw[1]; p2 += c.pw[2];
}

__global__ void world_to_patch_fwd_kernel(const float* __restrict__ pts, const float* pre_rot, float pre_scale,
                                          int pelvis_origin, const float* ti, const float* km, const float* pv,
                                          const float* rw, const float* tw, int B, int HK, float S, float rect, int flags,
                                          float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * HK) return;
  const int b = i / HK;
  const ProjParams c = load_proj(pre_rot, pelvis_origin, ti, km, pv, rw, tw, b, flags);
  float p0 = pts[i * 3], p1 = pts[i * 3 + 1], p2 = pts[i * 3 + 2];
  to_world(c, pre_rot != nullptr, pre_scale, p0, p1, p2);
  if (flags & XAS_GEO_WORLD) {                         // world mm (convert_verts, convert_pelvis_to_world)
    out[i * 3] = p0; out[i * 3 + 1] = p1; out[i * 3 + 2] = p2;
    return;
  }
  const float c0 = c.r[0] * p0 + c.r[1] * p1 + c.r[2] * p2 + c.tw[0];
  const float c1 = c.r[3] * p0 + c.r[4] * p1 + c.r[5] * p2 + c.tw[1];
  const float c2 = c.r[6] * p0 + c.r[7] * p1 + c.r[8] * p2 + c.tw[2];
  const float u = c0 / c2 * c.fx + c.cx, v = c1 / c2 * c.fy + c.cy;      // no clamp: c2 <= 0 gives what IEEE division gives
  if (flags & XAS_GEO_IMAGE) {                         // world -> image only (u px, v px, depth mm), util.py:116-125
    out[i * 3] = u; out[i * 3 + 1] = v; out[i * 3 + 2] = c2;
    return;
  }
  float z = (c2 - c.pz) / (1.0f / S * rect);
  float x = c.a00 * u + c.a01 * v + c.t0;
  float y = c.a10 * u + c.a11 * v + c.t1;
  if (flags & XAS_GEO_NORM) {
    x = x / (S - 1.f) * 2.f - 1.f;
    y = y / (S - 1.f) * 2.f - 1.f;
    z = z / (S - 1.f);
  }
  out[i * 3] = x; out[i * 3 + 1] = y; out[i * 3 + 2] = z;
}

// One block per sample: its threads walk the sample's Hy*K points (grad_pts), and the nine sums of grad_pre_rot are formed
// in a FIXED order (per-thread strided sum, butterfly wave sum, waves in order through LDS) - no floating-point atomics, so
// the op is bit-reproducible run to run.
constexpr int kProjBwdThreads = 256;

__global__ __launch_bounds__(kProjBwdThreads) void world_to_patch_bwd_kernel(
    const float* __restrict__ pts, const float* __restrict__ go, const float* pre_rot, float pre_scale, int pelvis_origin,
    const float* ti, const float* km, const float* pv, const float* rw, const float* tw, int HK, float S, float rect,
    int flags, float* __restrict__ gp, float* __restrict__ grot) {
  __shared__ float sm[20];
  const int b = blockIdx.x;
  const ProjParams c = load_proj(pre_rot, pelvis_origin, ti, km, pv, rw, tw, b, flags);
  const bool has_rot = pre_rot != nullptr;
  float acc[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) acc[e] = 0.f;
  for (int n = threadIdx.x; n < HK; n += kProjBwdThreads) {
    const size_t i = (size_t)b * HK + n;
    const float s0 = pts[i * 3], s1 = pts[i * 3 + 1], s2 = pts[i * 3 + 2];
    float g0 = go[i * 3], g1 = go[i * 3 + 1], g2 = go[i * 3 + 2];
    float d0, d1, d2;                                  // gradient w.r.t. the world point
    if (flags & XAS_GEO_WORLD) {
      d0 = g0; d1 = g1; d2 = g2;
    } else {
      float p0 = s0, p1 = s1, p2 = s2;
      to_world(c, has_rot, pre_scale, p0, p1, p2);
      const float c0 = c.r[0] * p0 + c.r[1] * p1 + c.r[2] * p2 + c.tw[0];
      const float c1 = c.r[3] * p0 + c.r[4] * p1 + c.r[5] * p2 + c.tw[1];
      const float c2 = c.r[6] * p0 + c.r[7] * p1 + c.r[8] * p2 + c.tw[2];
      if (!(flags & XAS_GEO_IMAGE)) {
        if (flags & XAS_GEO_NORM) { g0 = g0 * 2.f / (S - 1.f); g1 = g1 * 2.f / (S - 1.f); g2 = g2 / (S - 1.f); }
        const float e0 = c.a00 * g0 + c.a10 * g1, e1 = c.a01 * g0 + c.a11 * g1;
        g0 = e0; g1 = e1;
        g2 = g2 / (1.0f / S * rect);
      }
      const float k0 = g0 * c.fx / c2, k1 = g1 * c.fy / c2;             // d/dc0, d/dc1
      const float k2 = g2 - (k0 * c0 + k1 * c1) / c2;                   // d/dc2
      d0 = c.r[0] * k0 + c.r[3] * k1 + c.r[6] * k2;
      d1 = c.r[1] * k0 + c.r[4] * k1 + c.r[7] * k2;
      d2 = c.r[2] * k0 + c.r[5] * k1 + c.r[8] * k2;
    }
    if (has_rot) {
      d0 *= pre_scale; d1 *= pre_scale; d2 *= pre_scale;
      acc[0] += s0 * d0; acc[1] += s0 * d1; acc[2] += s0 * d2;
      acc[3] += s1 * d0; acc[4] += s1 * d1; acc[5] += s1 * d2;
      acc[6] += s2 * d0; acc[7] += s2 * d1; acc[8] += s2 * d2;
      const float e0 = c.g[0] * d0 + c.g[1] * d1 + c.g[2] * d2;
      const float e1 = c.g[3] * d0 + c.g[4] * d1 + c.g[5] * d2;
      const float e2 = c.g[6] * d0 + c.g[7] * d1 + c.g[8] * d2;
      d0 = e0; d1 = e1; d2 = e2;
    }
    gp[i * 3] = d0; gp[i * 3 + 1] = d1; gp[i * 3 + 2] = d2;
  }
  if (!has_rot) return;                                // uniform over the block
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const float r = block_sum(acc[e], sm);
    if (threadIdx.x == 0) grot[b * 9 + e] = r;
  }
}

// ------------------------------------------------------------------ line renderer
constexpr int kMaxLines = 32;
constexpr int kLineThreads = 256;
constexpr int kPixPerThread = 4;

struct LineSeg { float ax, ay, bx, by, vx, vy, den, scale; };

__device__ __forceinline__ void load_lines(LineSeg* segs, const float* kps, long sb, long sj, int b,
                                           const int* parents, const int* children, int L, unsigned fine,
                                           float body_width) {
  if (threadIdx.x < L) {
    const int l = threadIdx.x;
    const float* a = kps + b * sb + children[l] * sj;   // start = child, end = parent (util.py:35-36)
    const float* e = kps + b * sb + parents[l] * sj;
    LineSeg s;
    s.ax = a[0]; s.ay = a[1]; s.bx = e[0]; s.by = e[1];
    s.vx = s.bx - s.ax; s.vy = s.by - s.ay;
    s.den = 1e-8f + (s.vx * s.vx + s.vy * s.vy);
    s.scale = ((fine >> l) & 1u) ? 2.f : 1.f;
    segs[l] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ float seg_exponent(const LineSeg& s, float gx, float gy, float body_width, float* t_out) {
  const float dax = gx - s.ax, day = gy - s.ay;
  const float t = (dax * s.vx + day * s.vy) / s.den;
  float d2;
  if (t <= 0.f) {
    d2 = dax * dax + day * day;
  } else if (t >= 1.f) {
    const float dbx = gx - s.bx, dby = gy - s.by;
    d2 = dbx * dbx + dby * dby;
  } else {
    const float rx = gx - (s.ax + t * s.vx), ry = gy - (s.ay + t * s.vy);
    d2 = rx * rx + ry * ry;
  }
  *t_out = t;
  return (-d2 / body_width) * s.scale;
}

// The line a pixel takes its value from, for both passes: the first line whose exponent is NaN if there is one (a non-finite
// joint makes the whole mask of its sample NaN, as exp(...) followed by torch.max gives), else the first maximum.
struct LineWinner { float e, t; int line; };

__device__ __forceinline__ LineWinner winning_line(const LineSeg* segs, int L, float gx, float gy, float body_width) {
  LineWinner w = {-INFINITY, 0.f, 0};
  for (int l = 0; l < L; ++l) {
    float t;
    const float ex = seg_exponent(segs[l], gx, gy, body_width, &t);
    if (ex > w.e || (ex != ex && w.e == w.e)) { w.e = ex; w.t = t; w.line = l; }      // a NaN wins and stays
  }
  return w;
}

__global__ void draw_lines_max_fwd_kernel(const float* __restrict__ kps, long sb, long sj, const int* parents,
                                          const int* children, int L, unsigned fine, float body_width, int S,
                                          float* __restrict__ mask) {
  __shared__ LineSeg segs[kMaxLines];
  const int b = blockIdx.y;
  load_lines(segs, kps, sb, sj, b, parents, children, L, fine, body_width);
  const int pix0 = (blockIdx.x * kLineThreads + threadIdx.x) * kPixPerThread;
  if (pix0 >= S * S) return;
  const float fs = (float)(S - 1);
  float out[kPixPerThread];
#pragma unroll
  for (int q = 0; q < kPixPerThread; ++q) {
    const int pix = pix0 + q;
    const float gx = 2.f * ((float)(pix % S) / fs) - 1.f, gy = 2.f * ((float)(pix / S) / fs) - 1.f;
    out[q] = __expf(winning_line(segs, L, gx, gy, body_width).e);
  }
  float* o = mask + (size_t)b * S * S + pix0;
  if (pix0 + kPixPerThread <= S * S && ((S * S) % kPixPerThread) == 0) {
    *reinterpret_cast<float4*>(o) = make_float4(out[0], out[1], out[2], out[3]);
  } else {
    for (int q = 0; q < kPixPerThread && pix0 + q < S * S; ++q) o[q] = out[q];
  }
}

// Backward of the max-over-lines mask.  Every pixel sends a gradient to the two end points of its winning line.
// The per-block sums are formed in a FIXED order (per-line scan of the block's pixel records by one wave, butterfly
// wave sum, then lines -> joints in line order), never with floating-point atomics, so the detector gradient is
// reproducible run to run.
__global__ void draw_lines_max_bwd_kernel(const float* __restrict__ kps, long sb, long sj, const int* parents,
                                          const int* children, int L, unsigned fine, float body_width, int S, int K,
                                          const float* __restrict__ gmask, float* __restrict__ partial) {
  constexpr int kRec = kLineThreads * kPixPerThread;
  __shared__ LineSeg segs[kMaxLines];
  __shared__ int rec_line[kRec];
  __shared__ float rec_g[4][kRec];
  __shared__ float line_sum[kMaxLines][4];
  const int b = blockIdx.y;
  load_lines(segs, kps, sb, sj, b, parents, children, L, fine, body_width);
  const int pix0 = (blockIdx.x * kLineThreads + threadIdx.x) * kPixPerThread;
  const float fs = (float)(S - 1);
#pragma unroll
  for (int q = 0; q < kPixPerThread; ++q) {
    const int pix = pix0 + q;
    const int e = q * kLineThreads + threadIdx.x;
    int bl = -1;
    float gax = 0.f, gay = 0.f, gbx = 0.f, gby = 0.f;
    if (pix < S * S) {
      const float go = gmask[(size_t)b * S * S + pix];
      const float gx = 2.f * ((float)(pix % S) / fs) - 1.f, gy = 2.f * ((float)(pix / S) / fs) - 1.f;
      const LineWinner w = winning_line(segs, L, gx, gy, body_width);
      const float bt = w.t;
      const float ge = go * __expf(w.e);
      if (ge != 0.f) {
        bl = w.line;
        const LineSeg s = segs[w.line];
        const float gd2 = -ge * s.scale / body_width;
        if (bt <= 0.f) {
          gax = -2.f * (gx - s.ax) * gd2; gay = -2.f * (gy - s.ay) * gd2;
        } else if (bt >= 1.f) {
          gbx = -2.f * (gx - s.bx) * gd2; gby = -2.f * (gy - s.by) * gd2;
        } else {
          const float rx = gx - (s.ax + bt * s.vx), ry = gy - (s.ay + bt * s.vy);
          const float grx = 2.f * rx * gd2, gry = 2.f * ry * gd2;
          const float gt = -(grx * s.vx + gry * s.vy);
          const float gnum = gt / s.den, gden = -gt * bt / s.den;
          const float gvx = -bt * grx + (gx - s.ax) * gnum + 2.f * s.vx * gden;
          const float gvy = -bt * gry + (gy - s.ay) * gnum + 2.f * s.vy * gden;
          gax = -grx - s.vx * gnum - gvx; gay = -gry - s.vy * gnum - gvy;
          gbx = gvx; gby = gvy;
        }
      }
    }
    rec_line[e] = bl;
    rec_g[0][e] = gax; rec_g[1][e] = gay; rec_g[2][e] = gbx; rec_g[3][e] = gby;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int l = wave; l < L; l += kLineThreads / 64) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int e = lane; e < kRec; e += 64) {
      if (rec_line[e] == l) { s0 += rec_g[0][e]; s1 += rec_g[1][e]; s2 += rec_g[2][e]; s3 += rec_g[3][e]; }
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    // A line with a non-finite end point (den is then non-finite too) has a NaN exponent at every pixel; autograd sends NaN to
    // both its end points whether or not it is the winner (0 * NaN), and so does this.
    if (!(fabsf(segs[l].den) <= FLT_MAX)) s0 = s1 = s2 = s3 = NAN;
    if (lane == 0) { line_sum[l][0] = s0; line_sum[l][1] = s1; line_sum[l][2] = s2; line_sum[l][3] = s3; }
  }
  __syncthreads();
  float* o = partial + ((size_t)b * gridDim.x + blockIdx.x) * K * 2;
  for (int i = threadIdx.x; i < K * 2; i += blockDim.x) {
    const int j = i >> 1, c = i & 1;
    float s = 0.f;
    for (int l = 0; l < L; ++l) {
      if (children[l] == j) s += line_sum[l][c];
      if (parents[l] == j) s += line_sum[l][2 + c];
    }
    o[i] = s;
  }
}

__global__ void lines_bwd_reduce_kernel(const float* __restrict__ partial, int nblk, int K2, float* __restrict__ out) {
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < K2; i += blockDim.x) {
    float s = 0.f;
    for (int j = 0; j < nblk; ++j) s += partial[((size_t)b * nblk + j) * K2 + i];
    out[(size_t)b * K2 + i] = s;
  }
}

}  // namespace xas

using namespace xas;

extern "C" int xas_patch_to_world_fwd(const float* kps, const float* trans_image, const float* k_mat,
                                      const float* pelvis, const float* rot_world, const float* trans_world, int B,
                                      int Hy, int K, float image_size, float rect_width, int flags, float* world,
                                      void* stream) {
  XAS_REQUIRE(kps && world && trans_image && pelvis, "patch_to_world: null buffer");
  XAS_REQUIRE((flags & XAS_GEO_IMAGE) || (k_mat && rot_world && trans_world), "patch_to_world: null camera buffer");
  XAS_REQUIRE(B > 0 && Hy > 0 && K > 0, "patch_to_world: bad shape B=%d Hy=%d K=%d", B, Hy, K);
  const int n = B * Hy * K;
  hipLaunchKernelGGL(patch_to_world_fwd_kernel, dim3(cdiv(n, 128)), dim3(128), 0, as_stream(stream), kps, trans_image,
                     k_mat, pelvis, rot_world, trans_world, B, Hy * K, image_size, rect_width, flags, world);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_patch_to_world_bwd(const float* kps, const float* grad_world, const float* trans_image,
                                      const float* k_mat, const float* pelvis, const float* rot_world,
                                      const float* trans_world, int B, int Hy, int K, float image_size,
                                      float rect_width, int flags, float* grad_kps, void* stream) {
  XAS_REQUIRE(kps && grad_world && grad_kps && trans_image && k_mat && pelvis && rot_world && trans_world,
              "patch_to_world bwd: null buffer");
  XAS_REQUIRE(B > 0 && Hy > 0 && K > 0, "patch_to_world bwd: bad shape");
  XAS_REQUIRE(!(flags & XAS_GEO_IMAGE), "patch_to_world bwd: XAS_GEO_IMAGE is a forward-only (evaluation) mode");
  const int n = B * Hy * K;
  hipLaunchKernelGGL(patch_to_world_bwd_kernel, dim3(cdiv(n, 128)), dim3(128), 0, as_stream(stream), kps, grad_world,
                     trans_image, k_mat, pelvis, rot_world, trans_world, B, Hy * K, image_size, rect_width, flags,
                     grad_kps);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_world_to_patch_fwd(const float* pts, const float* pre_rot, float pre_scale, int pelvis_origin,
                                      const float* trans_image, const float* k_mat, const float* pelvis,
                                      const float* rot_world, const float* trans_world, int B, int Hy, int K,
                                      float image_size, float rect_width, int flags, float* out, void* stream) {
  XAS_REQUIRE(pts && out && k_mat && rot_world && trans_world, "world_to_patch: null buffer");
  XAS_REQUIRE((flags & (XAS_GEO_IMAGE | XAS_GEO_WORLD)) || (trans_image && pelvis), "world_to_patch: null crop / pelvis buffer");
  XAS_REQUIRE(!pelvis_origin || pelvis, "world_to_patch: pelvis_origin needs the pelvis");
  XAS_REQUIRE(!(flags & ~(XAS_GEO_NORM | XAS_GEO_IMAGE | XAS_GEO_WORLD)), "world_to_patch: unknown flag in %d", flags);
  XAS_REQUIRE(B > 0 && Hy > 0 && K > 0 && (long)B * Hy * K <= 0x7fffffffL / 3, "world_to_patch: bad shape B=%d Hy=%d K=%d",
              B, Hy, K);
  const int n = B * Hy * K;
  hipLaunchKernelGGL(world_to_patch_fwd_kernel, dim3(cdiv(n, 128)), dim3(128), 0, as_stream(stream), pts, pre_rot,
                     pre_scale, pelvis_origin, trans_image, k_mat, pelvis, rot_world, trans_world, B, Hy * K, image_size,
                     rect_width, flags, out);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_world_to_patch_bwd(const float* pts, const float* grad_out, const float* pre_rot, float pre_scale,
                                      int pelvis_origin, const float* trans_image, const float* k_mat, const float* pelvis,
                                      const float* rot_world, const float* trans_world, int B, int Hy, int K,
                                      float image_size, float rect_width, int flags, float* grad_pts, float* grad_pre_rot,
                                      void* stream) {
  XAS_REQUIRE(pts && grad_out && grad_pts && k_mat && rot_world && trans_world, "world_to_patch bwd: null buffer");
  XAS_REQUIRE((flags & (XAS_GEO_IMAGE | XAS_GEO_WORLD)) || (trans_image && pelvis),
              "world_to_patch bwd: null crop / pelvis buffer");
  XAS_REQUIRE(!pelvis_origin || pelvis, "world_to_patch bwd: pelvis_origin needs the pelvis");
  XAS_REQUIRE(!pre_rot == !grad_pre_rot, "world_to_patch bwd: grad_pre_rot goes with pre_rot");
  XAS_REQUIRE(!(flags & ~(XAS_GEO_NORM | XAS_GEO_IMAGE | XAS_GEO_WORLD)), "world_to_patch bwd: unknown flag in %d", flags);
  XAS_REQUIRE(B > 0 && Hy > 0 && K > 0 && (long)B * Hy * K <= 0x7fffffffL / 3,
              "world_to_patch bwd: bad shape B=%d Hy=%d K=%d", B, Hy, K);
  hipLaunchKernelGGL(world_to_patch_bwd_kernel, dim3(B), dim3(kProjBwdThreads), 0, as_stream(stream), pts, grad_out,
                     pre_rot, pre_scale, pelvis_origin, trans_image, k_mat, pelvis, rot_world, trans_world, Hy * K,
                     image_size, rect_width, flags, grad_pts, grad_pre_rot);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_lines_nblk(int S) { return (int)cdiv((long)S * S, kLineThreads * kPixPerThread); }

extern "C" int xas_draw_lines_max_fwd(const float* kps, long kp_stride_b, long kp_stride_j, int B, int K,
                                      const int* parents, const int* children, int L, unsigned fine_mask,
                                      float body_width, int S, float* mask, void* stream) {
  XAS_REQUIRE(kps && parents && children && mask, "draw_lines: null buffer");
  XAS_REQUIRE(L >= 1 && L <= kMaxLines && K >= 1 && K <= 64 && S >= 2 && B >= 1, "draw_lines: bad shape L=%d K=%d S=%d", L, K, S);
  XAS_REQUIRE(body_width > 0.f, "draw_lines: body_width must be > 0");
  hipLaunchKernelGGL(draw_lines_max_fwd_kernel, dim3(xas_lines_nblk(S), B), dim3(kLineThreads), 0, as_stream(stream),
                     kps, kp_stride_b, kp_stride_j, parents, children, L, fine_mask, body_width, S, mask);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_draw_lines_max_bwd(const float* kps, long kp_stride_b, long kp_stride_j, int B, int K,
                                      const int* parents, const int* children, int L, unsigned fine_mask,
                                      float body_width, int S, const float* grad_mask, float* partial,
                                      float* grad_kps_xy, void* stream) {
  XAS_REQUIRE(kps && parents && children && grad_mask && partial && grad_kps_xy, "draw_lines bwd: null buffer");
  XAS_REQUIRE(L >= 1 && L <= kMaxLines && K >= 1 && K <= 64 && S >= 2 && B >= 1, "draw_lines bwd: bad shape L=%d K=%d S=%d", L, K,
              S);
  XAS_REQUIRE(body_width > 0.f, "draw_lines bwd: body_width must be > 0");
  const int nblk = xas_lines_nblk(S);
  hipLaunchKernelGGL(draw_lines_max_bwd_kernel, dim3(nblk, B), dim3(kLineThreads), 0, as_stream(stream), kps,
                     kp_stride_b, kp_stride_j, parents, children, L, fine_mask, body_width, S, K, grad_mask, partial);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(lines_bwd_reduce_kernel, dim3(B), dim3(64), 0, as_stream(stream), partial, nblk, K * 2,
                     grad_kps_xy);
  XAS_LAUNCH_CHECK();
  return 0;
}
