// Evaluation path on the device (gfx950): hypothesis selection, multi-view DLT triangulation and the pose
// metrics.  All of it is tiny per-joint work (B*K ~ 600 points); the point of these kernels is that a whole
// evaluation batch stays on the GPU with ONE host synchronisation, instead of the reference's per-hypothesis
// tensor chains, a batched fp32 SVD and three numpy round trips per prediction set.
//
//   eval_select     : eval.py:117-148 + eval_utils.py:7-43 (switch_points, best/confident, per_act_mse)
//   projection      : modules/util.py:188 (P = K [R | t])
//   triangulate_dlt : modules/util.py:198-230 (null vector of the weighted DLT system)
//   triangulate_robust : the same DLT over the largest set of views that agree within a pixel threshold (no reference
//                     counterpart: eval.py --tri robust)
//   multiview_resolve : the left/right exchange of every view and the depth hypothesis of every view and joint, decided by the
//                     agreement of the views instead of the labels (stands beside eval_utils.py:7-29 and eval.py:129-148,
//                     on the DLT of modules/util.py:198-230: eval.py --resolve views)
//   triangulate_refine : Levenberg-Marquardt on the weighted reprojection error in pixels, from the DLT or robust point (no
//                     reference counterpart: eval.py --tri-refine lm)
//   triangulate_skeleton : the same refinement with the joints of a sample coupled by left/right limb symmetry, one wave per
//                     sample (no reference counterpart: eval.py --tri-skeleton)
//   triangulate_volume : product of the views' heat-map distributions over a voxel grid round the triangulated point, and its
//                     soft-argmax in world space (no reference counterpart: eval.py --tri-volume)
//   pose_metrics    : metrics.py:5-244 (MPJPE under none / scale / procrustes alignment, 3DPCK, AUC hit counts)
//
// Small symmetric eigenproblems (4x4) are solved with cyclic Jacobi rotations in double precision, fully unrolled
// so that the matrices live in registers: the DLT null vector is the eigenvector of A^T A with the smallest
// eigenvalue, and the Procrustes rotation is Horn's unit quaternion, the eigenvector of a 4x4 matrix built from
// the 3x3 correlation with the LARGEST eigenvalue (always a proper rotation: the same matrix as the reference's
// SVD solution with its det(R) = +1 fix, metrics.py:41-49).
#include "common.h"

namespace xas {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Cyclic Jacobi on a symmetric 4x4 (upper part used).  On return a[i][i] are the eigenvalues and the COLUMNS of v
// the eigenvectors.  12 sweeps: convergence is quadratic, 6-8 are enough for double precision.
__device__ __forceinline__ void jacobi4(double (&a)[4][4], double (&v)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 12; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      diag += a[i][i] * a[i][i];
#pragma unroll
      for (int j = i + 1; j < 4; ++j) off += a[i][j] * a[i][j];
    }
    if (off <= 1e-60 * diag || off == 0.0) break;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = a[p][q];
        if (apq != 0.0) {
          const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          a[p][p] -= t * apq;
          a[q][q] += t * apq;
          a[p][q] = 0.0; a[q][p] = 0.0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (r != p && r != q) {
              const double arp = a[r][p], arq = a[r][q];
              a[r][p] = c * arp - s * arq; a[p][r] = a[r][p];
              a[r][q] = s * arp + c * arq; a[q][r] = a[r][q];
            }
            const double vrp = v[r][p], vrq = v[r][q];
            v[r][p] = c * vrp - s * vrq;
            v[r][q] = s * vrp + c * vrq;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// eval_select: one block (one wave) per sample, lane = joint.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void eval_select_kernel(const float* __restrict__ kps, const float* __restrict__ joints,
                                                         const int* __restrict__ perm, int Hy, int K, int C, float S,
                                                         int flags, float* __restrict__ sel3d,
                                                         float* __restrict__ sel2d, float* __restrict__ err2d,
                                                         unsigned char* __restrict__ swapped) {
  const int b = blockIdx.x, k = threadIdx.x;
  const bool on = k < K;
  float g[3] = {0.f, 0.f, 0.f};
  if (on) {
    for (int c = 0; c < C; ++c) g[c] = joints[((size_t)b * K + k) * C + c];
    if (!(flags & XAS_EVAL_GT_NORMALISED)) {                       // eval.py:124-125
      g[0] = g[0] / (S - 1.f) * 2.f - 1.f;
      g[1] = g[1] / (S - 1.f) * 2.f - 1.f;
      g[2] = g[2] / (S - 1.f);
    }
  }
  const int kp = on ? perm[k] : 0;
  float best3[3] = {0.f, 0.f, 0.f}, best2[2] = {0.f, 0.f};
  float e3min = INFINITY, e2min = INFINITY;
  bool took = false;
  for (int h = 0; h < Hy; ++h) {
    float p[3] = {0.f, 0.f, 0.f}, m[3] = {0.f, 0.f, 0.f};
    if (on) {
      const float* src = kps + (((size_t)b * Hy + h) * K) * C;
      for (int c = 0; c < C; ++c) { p[c] = src[k * C + c]; m[c] = src[kp * C + c]; }
    }
    // eval_utils.py:16-27: L1 error over the first two coordinates, mirrored joint kept when strictly smaller
    float e_own = fabsf(p[0] - g[0]) + fabsf(p[1] - g[1]);
    float e_mir = fabsf(m[0] - g[0]) + fabsf(m[1] - g[1]);
    if (flags & XAS_EVAL_SWITCH_ALL) {                              // one decision per sample (sum over joints too)
      e_own = wave_sum(on ? e_own : 0.f);
      e_mir = wave_sum(on ? e_mir : 0.f);
    }
    took = !(flags & XAS_EVAL_NO_SWITCH) && e_mir < e_own;
    if (took) { p[0] = m[0]; p[1] = m[1]; p[2] = m[2]; }
    const float d0 = p[0] - g[0], d1 = p[1] - g[1], d2 = p[2] - g[2];
    const float e2 = __fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1));
    const float e3 = __fadd_rn(e2, __fmul_rn(d2, d2));
    const bool first = (flags & XAS_EVAL_CONFIDENT) ? (h == 0) : false;
    const bool better3 = (flags & XAS_EVAL_CONFIDENT) ? first : (e3 < e3min);       // argmin: first minimum wins
    const bool better2 = (flags & XAS_EVAL_CONFIDENT) ? first : (e2 < e2min);
    if (better3) { e3min = e3; best3[0] = p[0]; best3[1] = p[1]; best3[2] = p[2]; }
    if (better2) { e2min = e2; best2[0] = p[0]; best2[1] = p[1]; }
  }
  if (on) {
    if (sel3d) for (int c = 0; c < C; ++c) sel3d[((size_t)b * K + k) * C + c] = best3[c];
    if (sel2d) { sel2d[((size_t)b * K + k) * 2] = best2[0]; sel2d[((size_t)b * K + k) * 2 + 1] = best2[1]; }
    if (swapped) swapped[(size_t)b * K + k] = took ? 1 : 0;          // the reference keeps the LAST hypothesis' flags
  }
  if (err2d) {                                                       // eval_utils.py:32-43
    const float a0 = (best2[0] + 1.f) / 2.f - (g[0] + 1.f) / 2.f, a1 = (best2[1] + 1.f) / 2.f - (g[1] + 1.f) / 2.f;
    const float d = on ? sqrtf(__fadd_rn(__fmul_rn(a0, a0), __fmul_rn(a1, a1))) : 0.f;
    const float s = wave_sum(d);
    if (k == 0) err2d[b] = s / (float)K;
  }
}

// ------------------------------------------------------------------------------------------------------
// projection matrices: P[b] = K[b] [R[b] | t[b]]   (3x4)
// ------------------------------------------------------------------------------------------------------
__global__ void projection_kernel(const float* __restrict__ km, const float* __restrict__ rw, const float* __restrict__ tw,
                                  int B, float* __restrict__ P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * 12) return;
  const int b = i / 12, r = (i % 12) / 4, c = i % 4;
  const float* Kc = km + (size_t)b * 9;
  float acc = 0.f;
  for (int j = 0; j < 3; ++j) {
    const float rt = c < 3 ? rw[(size_t)b * 9 + j * 3 + c] : tw[(size_t)b * 3 + j];
    acc += Kc[r * 3 + j] * rt;
  }
  P[i] = acc;
}

// ------------------------------------------------------------------------------------------------------
// DLT pieces shared by triangulate_dlt and triangulate_robust.  Rows are formed in fp32 as the reference forms them
// (util.py:215-221; u P2 - P0 with one rounding), then A^T A and its smallest eigenvector are computed in double.
// ------------------------------------------------------------------------------------------------------
// One view's contribution to the upper triangle of A^T A, row-major (00 01 02 03 11 12 13 22 23 33): its two rows
// a_u = c (u P2 - P0), a_v = c (v P2 - P1) in fp32, their outer products in double.
__device__ __forceinline__ void dlt_view_gram(float u, float w, float c, const float* __restrict__ Pm, double (&t)[10]) {
  float au[4], av[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // u P2 - P0 as ONE fused multiply-add, written out: that is what the compiler has always made of this line in
    // triangulate_kernel, but left to itself it does not make it in every kernel, and the null vector of a nearly singular
    // system moves by tens of fp32 ulps with the last bit of a row
    au[j] = __fmul_rn(c, __builtin_fmaf(u, Pm[8 + j], -Pm[j]));
    av[j] = __fmul_rn(c, __builtin_fmaf(w, Pm[8 + j], -Pm[4 + j]));
  }
  int n = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int cc = r; cc < 4; ++cc) t[n++] = (double)au[r] * (double)au[cc] + (double)av[r] * (double)av[cc];
}

// g (upper triangle) += one view.  Both kernels add their views through here in ascending view order, so the same set
// of views gives the same matrix bit for bit.
template <typename T>
__device__ __forceinline__ void dlt_gram_add(double (&g)[4][4], const T& t) {
  int n = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int cc = r; cc < 4; ++cc) g[r][cc] += t[n++];
}

// Homogeneous null vector of the accumulated system: eigenvector of the smallest eigenvalue (g's upper triangle is used).
// NOT inlined: inlined into two kernels the compiler contracts the rotations' multiply-adds differently in each, and the
// two then differ in the last bits.  One body that both call makes the same matrix give the same vector by construction.
__device__ __noinline__ void dlt_null_vector(double (&g)[4][4], double (&X)[4]) {
#pragma unroll
  for (int r = 1; r < 4; ++r)
#pragma unroll
    for (int cc = 0; cc < r; ++cc) g[r][cc] = g[cc][r];
  double vec[4][4];
  jacobi4(g, vec);
  int best = 0;
  double lo = g[0][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (g[j][j] < lo) { lo = g[j][j]; best = j; }
#pragma unroll
  for (int r = 0; r < 4; ++r) X[r] = best == 0 ? vec[r][0] : (best == 1 ? vec[r][1] : (best == 2 ? vec[r][2] : vec[r][3]));
}

// ------------------------------------------------------------------------------------------------------
// triangulate_dlt: thread per (b, joint).  points [B][V][K][3] = (u, v, weight), P [B][V][3][4].
// ------------------------------------------------------------------------------------------------------
__global__ void triangulate_kernel(const float* __restrict__ pts, const float* __restrict__ P, int B, int V, int K,
                                   float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i % K;
  double g[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) g[r][c] = 0.0;
  float wsum = 0.f;
  int wpos = 0;
  for (int v = 0; v < V; ++v) {
    const float* q = pts + (((size_t)b * V + v) * K + k) * 3;
    const float c = q[2];
    wsum += c;
    wpos += c > 0.f ? 1 : 0;
    double t[10];
    dlt_view_gram(q[0], q[1], c, P + ((size_t)b * V + v) * 12, t);
    dlt_gram_add(g, t);
  }
  double X[4];
  dlt_null_vector(g, X);
  float* o = out + (size_t)i * 4;
  o[0] = (float)(X[0] / X[3]); o[1] = (float)(X[1] / X[3]); o[2] = (float)(X[2] / X[3]);
  o[3] = wsum / (float)wpos;                                          // util.py:207-209 (mean weight)
}

// ------------------------------------------------------------------------------------------------------
// triangulate_robust: exhaustive consensus over the subsets of the views, one wave per (b, joint), lane = subset mask.
// With V <= 6 the 2^V masks fit the 64 lanes, so nothing is sampled: every subset of >= 2 valid views is solved (DLT,
// as above), scored by how many valid views reproject within the threshold, and the best one's inlier set F is the
// answer.  F is itself a subset of >= 2 valid views, so the lane whose mask IS F has already solved exactly the system
// that triangulate_dlt restricted to F would solve, and has F's residuals: it writes the result.  No second solve.
// ------------------------------------------------------------------------------------------------------
struct TriView {
  double gram[10];        // dlt_view_gram of the view
  float P[12];
  float u, v, w, pad;
};

// h = P X of homogeneous X in one view, in double from the fp32 entries; false if X lies behind the camera (or on its
// principal plane).  The one projection, and the one meaning of "behind", of everything that reprojects in this file.
__device__ __forceinline__ bool project_view(const float* __restrict__ Pm, const double (&X)[4], double (&h)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
    h[r] = (double)Pm[4 * r] * X[0] + (double)Pm[4 * r + 1] * X[1] + (double)Pm[4 * r + 2] * X[2] + (double)Pm[4 * r + 3] * X[3];
  return !(h[2] / X[3] <= 0.0);
}

// Squared reprojection residual (px^2) of homogeneous X in one view, in double; +inf behind the camera.
__device__ __forceinline__ double reproj_r2(const TriView& s, const double (&X)[4]) {
  double h[3];
  if (!project_view(s.P, X, h)) return INFINITY;
  const double du = h[0] / h[2] - (double)s.u, dv = h[1] / h[2] - (double)s.v;
  return du * du + dv * dv;
}

__global__ __launch_bounds__(64) void triangulate_robust_kernel(const float* __restrict__ pts, const float* __restrict__ P,
                                                                int V, int K, float threshold_px, float* __restrict__ out,
                                                                unsigned char* __restrict__ inliers,
                                                                float* __restrict__ resid) {
  __shared__ TriView sv[XAS_TRI_MAX_VIEWS];
  const int i = blockIdx.x, b = i / K, k = i % K;
  const int lane = threadIdx.x;
  bool ok = false;
  if (lane < V) {                                                     // lane v stages view v
    const float* q = pts + (((size_t)b * V + lane) * K + k) * 3;
    const float* Pm = P + ((size_t)b * V + lane) * 12;
    TriView& s = sv[lane];
    s.u = q[0]; s.v = q[1]; s.w = q[2]; s.pad = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) s.P[j] = Pm[j];
    double t[10];
    dlt_view_gram(s.u, s.v, s.w, Pm, t);
#pragma unroll
    for (int j = 0; j < 10; ++j) s.gram[j] = t[j];
    ok = s.w > 0.f && s.w < INFINITY;                                 // valid: finite and positive weight
  }
  const int valid = (int)__ballot(ok);                                // bits < V only
  __syncthreads();

  // --- candidate = this lane's mask, if it is a set of >= 2 valid views
  const bool cand = (lane & ~valid) == 0 && __popc(lane) >= 2;
  double X[4] = {0.0, 0.0, 0.0, 0.0}, r2[XAS_TRI_MAX_VIEWS];
  int cnt = -1, inl = 0;
  double cost = INFINITY;
  if (cand) {
    double g[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) g[r][c] = 0.0;
#pragma unroll
    for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v)
      if ((lane >> v) & 1) dlt_gram_add(g, sv[v].gram);
    dlt_null_vector(g, X);
    cnt = 0;
    cost = 0.0;
#pragma unroll
    for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v) {
      r2[v] = 0.0;
      if ((valid >> v) & 1) {
        r2[v] = reproj_r2(sv[v], X);
        if (sqrt(r2[v]) < (double)threshold_px) { ++cnt; cost += r2[v]; inl |= 1 << v; }
      }
    }
  }
  // --- wave arg-best: more inliers, then smaller sum of squared inlier residuals, then smaller mask.  A total order
  // (masks are distinct), so the xor butterfly leaves the same winner in every lane.
  int bcnt = cnt, binl = inl, bid = lane;
  double bcost = cost;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ocnt = __shfl_xor(bcnt, o, 64), oinl = __shfl_xor(binl, o, 64), oid = __shfl_xor(bid, o, 64);
    const double ocost = __shfl_xor(bcost, o, 64);
    const bool take = ocnt > bcnt || (ocnt == bcnt && (ocost < bcost || (ocost == bcost && oid < bid)));
    if (take) { bcnt = ocnt; binl = oinl; bid = oid; bcost = ocost; }
  }
  const int used = bcnt >= 2 ? binl : valid;                          // no consensus of two views: all valid views
  const int nused = __popc(used);
  float* o = out + (size_t)i * 4;
  if (__popc(valid) < 2) {                                            // nothing to solve
    if (lane == 0) {
      float wsum = 0.f;
      for (int v = 0; v < V; ++v) wsum += ((valid >> v) & 1) ? sv[v].w : 0.f;
      o[0] = NAN; o[1] = NAN; o[2] = NAN; o[3] = wsum / (float)nused;
      if (inliers) inliers[i] = 0;
      if (resid) resid[i] = NAN;
    }
    return;
  }
  if (lane != used) return;                                           // the lane that solved exactly the views used
  float wsum = 0.f;
  double rsum = 0.0;
#pragma unroll
  for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v)
    if ((used >> v) & 1) { wsum += sv[v].w; rsum += r2[v]; }
  o[0] = (float)(X[0] / X[3]); o[1] = (float)(X[1] / X[3]); o[2] = (float)(X[2] / X[3]);
  o[3] = wsum / (float)nused;
  if (inliers) inliers[i] = (unsigned char)(bcnt >= 2 ? binl : 0);
  if (resid) resid[i] = (float)sqrt(rsum / (double)nused);
}

// ------------------------------------------------------------------------------------------------------
// multiview_resolve: which views carry a left/right pair exchanged, and which depth hypothesis each view holds, from the
// views' agreement alone.  One wave per (b, joint a with a <= perm[a]); for a pair (a, c = perm[a]) lane = exchange mask:
// bit v set gives joint a view v's point of joint c and joint c that of joint a.  The lowest valid view (the anchor) keeps
// its naming, which halves the masks (m and ~m name the same two points); every other mask over the valid views solves
// both joints by the DLT above and is scored by the sum of their squared reprojection residuals.  The winning lane holds
// both solutions, so nothing is solved twice.  Then lane = (joint, view) picks the hypothesis whose single-view world
// point is nearest the triangulated one, and, only if labels are given, the pair is named once for all views.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void multiview_resolve_kernel(const float* __restrict__ pts, const float* __restrict__ P,
                                                               const float* __restrict__ kps, const float* __restrict__ world,
                                                               const int* __restrict__ perm, const float* __restrict__ gt,
                                                               int V, int Hy, int K, float S, float* __restrict__ sel,
                                                               float* __restrict__ xyzw, unsigned char* __restrict__ swap,
                                                               unsigned char* __restrict__ hyp,
                                                               unsigned char* __restrict__ named) {
  __shared__ TriView sv[2][XAS_TRI_MAX_VIEWS];                        // [0] joint a, [1] joint c
  const int i = blockIdx.x, b = i / K, a = i % K;
  int c = perm[a];
  if (c < 0 || c >= K || perm[c] != a) c = a;                         // not a pair table here: the joint stands alone
  if (c < a) return;                                                  // the pair belongs to the block of its lower joint
  const bool paired = c != a;
  const int lane = threadIdx.x;
  const int j = lane >> 5, v = lane & 31;                             // lanes 0..V-1: joint a's views, 32..32+V-1: joint c's
  const bool stager = v < V && (j == 0 || paired);
  const int k = j ? c : a, kp = j ? a : c;                            // this lane's joint and its partner
  bool ok = false;
  if (stager) {
    const float* q = pts + (((size_t)b * V + v) * K + k) * 3;
    const float* Pm = P + ((size_t)b * V + v) * 12;
    TriView& s = sv[j][v];
    s.u = q[0]; s.v = q[1]; s.w = q[2]; s.pad = 0.f;
#pragma unroll
    for (int n = 0; n < 12; ++n) s.P[n] = Pm[n];
    double t[10];
    dlt_view_gram(s.u, s.v, s.w, Pm, t);
#pragma unroll
    for (int n = 0; n < 10; ++n) s.gram[n] = t[n];
    ok = s.w > 0.f && s.w < INFINITY;
  }
  const unsigned long long bal = __ballot(ok);
  const int va = (int)(bal & 63ull), vc = (int)((bal >> 32) & 63ull);
  const int valid = paired ? (va & vc) : va;                          // a view counts for the pair if it sees both joints
  __syncthreads();
  const int nvalid = __popc(valid);
  const bool solved = nvalid >= 2;
  const int anchor = valid ? __ffs(valid) - 1 : 0;

  // --- stage 1: candidate = this lane's mask, if it exchanges valid views only and leaves the anchor alone
  const bool cand = solved && (lane & ~valid) == 0 && !((lane >> anchor) & 1) && (paired || lane == 0);
  double Xa[4] = {0.0, 0.0, 0.0, 0.0}, Xc[4] = {0.0, 0.0, 0.0, 0.0};
  double cost = INFINITY;
  if (cand) {
    cost = 0.0;
#pragma unroll 1
    for (int jj = 0; jj < 2; ++jj) {
      if (jj == 1 && !paired) break;
      double g[4][4], X[4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) g[r][cc] = 0.0;
#pragma unroll
      for (int w = 0; w < XAS_TRI_MAX_VIEWS; ++w)
        if ((valid >> w) & 1) dlt_gram_add(g, sv[jj ^ ((lane >> w) & 1)][w].gram);
      dlt_null_vector(g, X);
#pragma unroll
      for (int w = 0; w < XAS_TRI_MAX_VIEWS; ++w)
        if ((valid >> w) & 1) cost += reproj_r2(sv[jj ^ ((lane >> w) & 1)][w], X);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (jj == 0) Xa[r] = X[r]; else Xc[r] = X[r];
      }
    }
    if (!(cost < INFINITY)) cost = INFINITY;                          // NaN too: the order below must be total
  }
  // --- wave arg-best: a candidate before none, then the smaller cost, then the smaller mask (a total order)
  int bnc = cand ? 0 : 1, bid = lane;
  double bcost = cost;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int onc = __shfl_xor(bnc, o, 64), oid = __shfl_xor(bid, o, 64);
    const double ocost = __shfl_xor(bcost, o, 64);
    const bool take = onc < bnc || (onc == bnc && (ocost < bcost || (ocost == bcost && oid < bid)));
    if (take) { bnc = onc; bid = oid; bcost = ocost; }
  }
  const int win = solved ? bid : 0;
  float xa[3], xc[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    xa[r] = solved ? __shfl((float)(Xa[r] / Xa[3]), win, 64) : NAN;
    xc[r] = solved ? (paired ? __shfl((float)(Xc[r] / Xc[3]), win, 64) : xa[r]) : NAN;
  }
  float wa = 0.f, wc = 0.f;                                           // mean weight of the views used, ascending
#pragma unroll
  for (int w = 0; w < XAS_TRI_MAX_VIEWS; ++w)
    if ((valid >> w) & 1) {
      const int bit = (win >> w) & 1;
      wa += sv[bit][w].w;
      if (paired) wc += sv[1 ^ bit][w].w;
    }
  wa = wa / (float)nvalid;
  wc = wc / (float)nvalid;

  // --- stage 2: lane = (joint, view), every view, valid or not
  const bool swapped = ((win >> v) & 1) != 0;
  const int src = swapped ? kp : k;
  int hs = 0;
  float s3[3] = {0.f, 0.f, 0.f};
  if (stager) {
    const double x0 = j ? xc[0] : xa[0], x1 = j ? xc[1] : xa[1], x2 = j ? xc[2] : xa[2];
    double best = INFINITY;
    for (int h = 0; h < Hy; ++h) {
      const float* wp = world + ((((size_t)b * V + v) * Hy + h) * K + src) * 3;
      const double d0 = (double)wp[0] - x0, d1 = (double)wp[1] - x1, d2 = (double)wp[2] - x2;
      const double d = d0 * d0 + d1 * d1 + d2 * d2;
      if (d < best) { best = d; hs = h; }                             // first minimum; NaN or inf never wins: h = 0
    }
    const float* q = kps + ((((size_t)b * V + v) * Hy + hs) * K + src) * 3;
    s3[0] = q[0]; s3[1] = q[1]; s3[2] = q[2];
  }
  // --- stage 3: which of the two consistent namings is "left" - the one bit only labels can give
  bool ex = false;
  if (gt && paired && solved) {                                       // uniform over the wave
    float own = 0.f, oth = 0.f;
    if (stager && ((valid >> v) & 1)) {
      const float* gk = gt + (((size_t)b * V + v) * K + k) * 3;
      const float* gp = gt + (((size_t)b * V + v) * K + kp) * 3;
      own = fabsf(s3[0] - (gk[0] / (S - 1.f) * 2.f - 1.f)) + fabsf(s3[1] - (gk[1] / (S - 1.f) * 2.f - 1.f));
      oth = fabsf(s3[0] - (gp[0] / (S - 1.f) * 2.f - 1.f)) + fabsf(s3[1] - (gp[1] / (S - 1.f) * 2.f - 1.f));
    }
    const double sown = wave_sum_d((double)own), soth = wave_sum_d((double)oth);
    ex = soth < sown;
  }
  if (stager) {
    const int dst = (ex && ((valid >> v) & 1)) ? kp : k;
    const size_t o = ((size_t)b * V + v) * K + dst;
    sel[o * 3] = s3[0]; sel[o * 3 + 1] = s3[1]; sel[o * 3 + 2] = s3[2];
    if (hyp) hyp[o] = (unsigned char)hs;
  }
  if (lane == 0) {
    const unsigned char fm = (unsigned char)(ex ? (win ^ valid) : win);
    const size_t oa = (size_t)b * K + a, oc = (size_t)b * K + c;
    if (xyzw) {
      float* o = xyzw + oa * 4;
      o[0] = ex ? xc[0] : xa[0]; o[1] = ex ? xc[1] : xa[1]; o[2] = ex ? xc[2] : xa[2]; o[3] = ex ? wc : wa;
      if (paired) {
        o = xyzw + oc * 4;
        o[0] = ex ? xa[0] : xc[0]; o[1] = ex ? xa[1] : xc[1]; o[2] = ex ? xa[2] : xc[2]; o[3] = ex ? wa : wc;
      }
    }
    if (swap) { swap[oa] = fm; swap[oc] = fm; }
    if (named && gt) { named[oa] = ex ? 1 : 0; named[oc] = ex ? 1 : 0; }
  }
}

// ------------------------------------------------------------------------------------------------------
// triangulate_refine: Levenberg-Marquardt on the weighted reprojection error from the DLT / robust result, thread per
// (b, joint) as triangulate_kernel.  A few hundred joints of 3x3 algebra in double: latency-bound, no throughput to win.
// A thread keeps its V points (u, v, scale) in registers and re-reads the sample's projection matrices at every
// linearisation: at most 72 floats that all threads of a sample share, so they stay in the caches, where holding them
// would cost every thread 72 more registers.  Every loop over the views is unrolled to XAS_TRI_MAX_VIEWS and predicated by
// the mask of the views used, so no array is indexed at run time and no view >= V is ever read.
// ------------------------------------------------------------------------------------------------------
// Inverse of the symmetric 3x3 a (upper triangle 00 01 02 11 12 22) by its adjugate.  A singular a gives inf / NaN.
__device__ __forceinline__ void sym3_inverse(const double (&a)[6], double (&inv)[6]) {
  const double c00 = a[3] * a[5] - a[4] * a[4], c01 = a[2] * a[4] - a[1] * a[5], c02 = a[1] * a[4] - a[2] * a[3];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  inv[0] = c00 / det; inv[1] = c01 / det; inv[2] = c02 / det;
  inv[3] = (a[0] * a[5] - a[2] * a[2]) / det;
  inv[4] = (a[1] * a[2] - a[0] * a[4]) / det;
  inv[5] = (a[0] * a[3] - a[1] * a[1]) / det;
}

// The problem at one point X: cost C, sum of the squared unweighted pixel residuals r2, Gauss-Newton Hessian H (upper
// triangle) and gradient g with the IRLS weights of X itself.  false if X lies behind a view used.
struct RefineFit {
  double C, r2, H[6], g[3];
};

__device__ __forceinline__ bool refine_linearise(const float* __restrict__ Pb, int used, const float (&pu)[XAS_TRI_MAX_VIEWS],
                                                 const float (&pv)[XAS_TRI_MAX_VIEWS], const float (&ps)[XAS_TRI_MAX_VIEWS],
                                                 double huber, const double (&X)[3], RefineFit& f) {
  f.C = 0.0; f.r2 = 0.0;
#pragma unroll
  for (int n = 0; n < 6; ++n) f.H[n] = 0.0;
#pragma unroll
  for (int n = 0; n < 3; ++n) f.g[n] = 0.0;
  const double Xh[4] = {X[0], X[1], X[2], 1.0};
  bool front = true;
#pragma unroll
  for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v) {
    if (!((used >> v) & 1)) continue;
    const float* Pm = Pb + v * 12;
    double h[3];
    front = project_view(Pm, Xh, h) && front;
    const double pu_ = h[0] / h[2], pv_ = h[1] / h[2];
    const double ru = pu_ - (double)pu[v], rv = pv_ - (double)pv[v];
    const double s = (double)ps[v], rr = ru * ru + rv * rv, e = s * sqrt(rr);
    const bool tail = huber > 0.0 && e > huber;
    f.r2 += rr;
    f.C += tail ? 2.0 * huber * e - huber * huber : e * e;
    const double wt = (tail ? huber / e : 1.0) * s * s;
    double ju[3], jv[3];                                              // d(u, v) / dX
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      ju[n] = ((double)Pm[n] - pu_ * (double)Pm[8 + n]) / h[2];
      jv[n] = ((double)Pm[4 + n] - pv_ * (double)Pm[8 + n]) / h[2];
      f.g[n] += wt * (ju[n] * ru + jv[n] * rv);
    }
    int n = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = r; c < 3; ++c) f.H[n++] += wt * (ju[r] * ju[c] + jv[r] * jv[c]);
  }
  return front;
}

__global__ __launch_bounds__(64) void triangulate_refine_kernel(const float* __restrict__ pts, const float* __restrict__ P,
                                                                const float* __restrict__ init,
                                                                const unsigned char* __restrict__ views, int B, int V, int K,
                                                                int flags, float huber_, int max_iter, float* __restrict__ out,
                                                                float* __restrict__ resid, float* __restrict__ cov,
                                                                unsigned char* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i % K;
  const float* Pb = P + (size_t)b * V * 12;
  float pu[XAS_TRI_MAX_VIEWS], pv[XAS_TRI_MAX_VIEWS], ps[XAS_TRI_MAX_VIEWS];
  int valid = 0;
#pragma unroll
  for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v) {
    pu[v] = 0.f; pv[v] = 0.f; ps[v] = 0.f;
    if (v < V) {
      const float* q = pts + (((size_t)b * V + v) * K + k) * 3;
      pu[v] = q[0]; pv[v] = q[1];
      ps[v] = (flags & XAS_REFINE_WEIGHTED) ? q[2] : 1.f;
      valid |= (q[2] > 0.f && q[2] < INFINITY) ? 1 << v : 0;          // the rule of triangulate_robust_kernel
    }
  }
  const int sel = views ? views[i] : 0;
  const int used = sel ? (valid & sel) : valid;                       // a zero byte is the robust kernel's fallback: all valid views
  const int nused = __popc(used);
  const double huber = (double)huber_;

  const float* in = init + (size_t)i * 4;
  const float x0 = in[0], x1 = in[1], x2 = in[2];
  double X[3] = {(double)x0, (double)x1, (double)x2};
  RefineFit fit;
  const bool finite = fabs(X[0]) < INFINITY && fabs(X[1]) < INFINITY && fabs(X[2]) < INFINITY;
  const bool solve = nused >= 2 && finite && refine_linearise(Pb, used, pu, pv, ps, huber, X, fit);
  float* o = out + (size_t)i * 4;
  o[3] = in[3];
  if (!solve) {                                                       // passed through: init bit for bit, NaN stays NaN
    o[0] = x0; o[1] = x1; o[2] = x2;
    if (resid) { resid[(size_t)i * 2] = NAN; resid[(size_t)i * 2 + 1] = NAN; }
    if (cov)
      for (int n = 0; n < 6; ++n) cov[(size_t)i * 6 + n] = NAN;
    if (status) status[i] = 2;
    return;
  }
  const double r2_init = fit.r2;
  double lambda = 1e-3;
  int st = 1;
  for (int it = 0; it < max_iter; ++it) {
    const double a[6] = {fit.H[0] * (1.0 + lambda), fit.H[1], fit.H[2], fit.H[3] * (1.0 + lambda), fit.H[4],
                         fit.H[5] * (1.0 + lambda)};                  // H + lambda diag(H)
    double inv[6];
    sym3_inverse(a, inv);
    const double d[3] = {-(inv[0] * fit.g[0] + inv[1] * fit.g[1] + inv[2] * fit.g[2]),
                         -(inv[1] * fit.g[0] + inv[3] * fit.g[1] + inv[4] * fit.g[2]),
                         -(inv[2] * fit.g[0] + inv[4] * fit.g[1] + inv[5] * fit.g[2])};
    const double Xt[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
    RefineFit trial;
    const bool front = refine_linearise(Pb, used, pu, pv, ps, huber, Xt, trial);
    if (front && trial.C < fit.C) {                                   // NaN never passes
      X[0] = Xt[0]; X[1] = Xt[1]; X[2] = Xt[2];
      fit = trial;
      lambda *= 0.1;
      if (sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < 1e-5) { st = 0; break; }
    } else {
      lambda *= 10.0;
      if (lambda > 1e12) break;
    }
  }
  o[0] = (float)X[0]; o[1] = (float)X[1]; o[2] = (float)X[2];
  if (resid) {
    resid[(size_t)i * 2] = (float)sqrt(r2_init / (double)nused);
    resid[(size_t)i * 2 + 1] = (float)sqrt(fit.r2 / (double)nused);
  }
  if (cov) {
    double c[6];
    sym3_inverse(fit.H, c);
#pragma unroll
    for (int n = 0; n < 6; ++n) cov[(size_t)i * 6 + n] = (float)c[n];
  }
  if (status) status[i] = (unsigned char)st;
}

// ------------------------------------------------------------------------------------------------------
// triangulate_skeleton: the refinement above with the joints of a sample coupled by left/right limb symmetry, so one
// Levenberg-Marquardt problem per SAMPLE in up to 3 * 24 unknowns.  One wave per sample; everything the lanes share lives in
// LDS (SkShared, 61 KB static):
//   H, Lm    the Gauss-Newton matrix and the Cholesky factor of its damped copy, lower triangles packed row by row
//            (row i starts at i (i + 1) / 2).  H is kept because a rejected trial factors it again under a larger lambda.
//   term     the 12 numbers of every (joint, view) residual term: cost, |r|^2, the 3x3 block, the gradient, in-front flag
//   X, lu, le  two copies of the point and of the limbs' unit vectors and residuals: `cur` and the trial; accepting a trial
//            swaps the index, nothing is copied
// Division of labour.  Residual terms: lane = (joint, view) pair, strided over K V.  Sums over the views of a joint, in
// ascending view order: lane = joint.  Limb residuals: lane = limb pair.  H: lane = a 3x3 block (joint, joint) that it alone
// assembles and stores, from the terms and from every limb that couples the two joints, in ascending limb order - no two lanes
// ever add to one entry, so no atomics and one order of summation.  Cholesky, column by column: lane = row (two rows per lane
// past 64); the pivot leaves its lane by a cross-lane read, so a column costs one barrier.  Triangular solves: the right-hand
// side stays in registers, lane = row, one cross-lane read per column.  Rows of joints that no limb couples to an earlier joint
// start at their own block (`first`), which confines the inner products to the envelope: the shipped skeleton is two 18x18
// blocks and six 3x3 ones, not one 54x54.  Every value a branch depends on is read from lane 0, so the wave never diverges
// round a barrier.
// ------------------------------------------------------------------------------------------------------
constexpr int kSkJ = XAS_SKEL_MAX_JOINTS, kSkL = XAS_SKEL_MAX_LIMBS, kSkN = 3 * kSkJ, kSkTri = kSkN * (kSkN + 1) / 2;

struct SkLimbs {
  int j[kSkL][4];                                                     // far_a, near_a, far_b, near_b: checked by the host
};

struct SkShared {
  double H[kSkTri], Lm[kSkTri];
  double term[kSkJ][XAS_TRI_MAX_VIEWS][12];                           // C, r2, H 00 01 02 11 12 22, g 0 1 2, in front (1 / 0)
  double X[2][kSkJ][3];
  double lu[2][kSkL][2][3], le[2][kSkL];                              // unit vectors of limb a and b (0 where flat), |a| - |b|
  double g[kSkN];
  float P[XAS_TRI_MAX_VIEWS][12];
  float pu[kSkJ][XAS_TRI_MAX_VIEWS], pv[kSkJ][XAS_TRI_MAX_VIEWS], ps[kSkJ][XAS_TRI_MAX_VIEWS];
  int used[kSkJ];                                                     // mask of the views used
  int slot[kSkJ], joint[kSkJ], first[kSkJ];                           // joint -> free slot, slot -> joint, slot -> first coupled slot
  int lj[kSkL][4];
};
static_assert(sizeof(SkShared) <= 64 * 1024, "triangulate_skeleton: static LDS of one block");

__device__ __forceinline__ double lane0(double v) { return __shfl(v, 0, 64); }

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ int sk_idx(int i, int j) { return i * (i + 1) / 2 + j; }        // j <= i

// The residual terms of the joints in `mask` at X[src], then each joint's sums on its own lane: cost, |r|^2 and whether it lies
// in front of every view it uses.  Starts with a barrier (X[src] was just written, `term` may still be read) and ends past one.
__device__ __forceinline__ void sk_reproj(SkShared& s, int src, int V, int K, unsigned mask, double huber, int lane, double& Ck,
                                          double& r2k, bool& frontk) {
  __syncthreads();
  for (int t = lane; t < K * V; t += 64) {
    const int k = t / V, v = t - k * V;
    if (!((mask >> k) & 1) || !((s.used[k] >> v) & 1)) continue;
    const float* Pm = s.P[v];
    const double Xh[4] = {s.X[src][k][0], s.X[src][k][1], s.X[src][k][2], 1.0};
    double h[3];
    const bool front = project_view(Pm, Xh, h);
    const double pu_ = h[0] / h[2], pv_ = h[1] / h[2];
    const double ru = pu_ - (double)s.pu[k][v], rv = pv_ - (double)s.pv[k][v];
    const double sc = (double)s.ps[k][v], rr = ru * ru + rv * rv, e = sc * sqrt(rr);
    const bool tail = huber > 0.0 && e > huber;
    const double wt = (tail ? huber / e : 1.0) * sc * sc;
    double* o = s.term[k][v];
    o[0] = tail ? 2.0 * huber * e - huber * huber : e * e;
    o[1] = rr;
    double ju[3], jv[3];                                              // d(u, v) / dX
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      ju[n] = ((double)Pm[n] - pu_ * (double)Pm[8 + n]) / h[2];
      jv[n] = ((double)Pm[4 + n] - pv_ * (double)Pm[8 + n]) / h[2];
      o[8 + n] = wt * (ju[n] * ru + jv[n] * rv);
    }
    int n = 2;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = r; c < 3; ++c) o[n++] = wt * (ju[r] * ju[c] + jv[r] * jv[c]);
    o[11] = front ? 1.0 : 0.0;
  }
  __syncthreads();
  Ck = 0.0; r2k = 0.0; frontk = true;
  if (lane < K && ((mask >> lane) & 1))
    for (int v = 0; v < V; ++v)
      if ((s.used[lane] >> v) & 1) {
        Ck += s.term[lane][v][0];
        r2k += s.term[lane][v][1];
        frontk = frontk && s.term[lane][v][11] != 0.0;
      }
}

// The limb pairs in `active` at X[src], lane = pair: unit vectors and |a| - |b| to LDS; -> |a| - |b| (0 on the other lanes).
__device__ __forceinline__ double sk_limbs(SkShared& s, int src, int L, unsigned active, int lane) {
  if (lane >= L || !((active >> lane) & 1)) return 0.0;
  double len[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int f = s.lj[lane][2 * m], n = s.lj[lane][2 * m + 1];
    double d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = s.X[src][f][c] - s.X[src][n][c];
    len[m] = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) s.lu[src][lane][m][c] = d[c];
  }
  const bool flat = !(len[0] >= 1e-9 && len[1] >= 1e-9);              // a limb with no direction: the pair's Jacobian row is 0
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 3; ++c) s.lu[src][lane][m][c] = flat ? 0.0 : s.lu[src][lane][m][c] / len[m];
  const double e = len[0] - len[1];
  s.le[src][lane] = e;
  return e;
}

// d (|a| - |b|) / d (coordinate c of joint k) of limb pair l: +ua at far_a, -ua at near_a, -ub at far_b, +ub at near_b, summed
// where a joint stands in more than one of the four places.
__device__ __forceinline__ double sk_coef(const SkShared& s, int src, int l, int k, int c) {
  double v = 0.0;
  if (s.lj[l][0] == k) v += s.lu[src][l][0][c];
  if (s.lj[l][1] == k) v -= s.lu[src][l][0][c];
  if (s.lj[l][2] == k) v -= s.lu[src][l][1][c];
  if (s.lj[l][3] == k) v += s.lu[src][l][1][c];
  return v;
}

__device__ __forceinline__ bool sk_touches(const SkShared& s, int l, int k) {
  return s.lj[l][0] == k || s.lj[l][1] == k || s.lj[l][2] == k || s.lj[l][3] == k;
}

// H and g at X[src] from `term` and the limbs: every lane assembles whole 3x3 blocks (slot bi >= slot bj) and whole entries of g.
__device__ __forceinline__ void sk_assemble(SkShared& s, int src, int V, int nfree, int L, unsigned active, double sym_w, int lane) {
  __syncthreads();
  for (int p = lane; p < nfree * (nfree + 1) / 2; p += 64) {
    int bi = (int)((sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);
    while (bi * (bi + 1) / 2 > p) --bi;
    while ((bi + 1) * (bi + 2) / 2 <= p) ++bi;
    const int bj = p - bi * (bi + 1) / 2, ki = s.joint[bi], kj = s.joint[bj];
    double h[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (bi == bj)
      for (int v = 0; v < V; ++v)
        if ((s.used[ki] >> v) & 1) {
          const double* t = s.term[ki][v];
          h[0][0] += t[2]; h[0][1] += t[3]; h[0][2] += t[4]; h[1][1] += t[5]; h[1][2] += t[6]; h[2][2] += t[7];
        }
    h[1][0] = h[0][1]; h[2][0] = h[0][2]; h[2][1] = h[1][2];
    for (int l = 0; l < L; ++l) {
      if (!((active >> l) & 1) || !sk_touches(s, l, ki) || !sk_touches(s, l, kj)) continue;
      double ci[3], cj[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { ci[c] = sk_coef(s, src, l, ki, c); cj[c] = sk_coef(s, src, l, kj, c); }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) h[r][c] += sym_w * ci[r] * cj[c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (bi > bj || c <= r) s.H[sk_idx(3 * bi + r, 3 * bj + c)] = h[r][c];
  }
  for (int i = lane; i < 3 * nfree; i += 64) {
    const int k = s.joint[i / 3], c = i % 3;
    double gi = 0.0;
    for (int v = 0; v < V; ++v)
      if ((s.used[k] >> v) & 1) gi += s.term[k][v][8 + c];
    for (int l = 0; l < L; ++l)
      if (((active >> l) & 1) && sk_touches(s, l, k)) gi += sym_w * s.le[src][l] * sk_coef(s, src, l, k, c);
    s.g[i] = gi;
  }
  __syncthreads();
}

// Cholesky of H + lambda diag(H) into Lm, left-looking: at column j the lane of row i >= j forms H_ij - sum_k L_ik L_jk over the
// envelope; the pivot is read from row j's lane.  inv[h] = 1 / L_ii of rows lane + 64 h.  false at a pivot that is not > 0.
__device__ __forceinline__ bool sk_factor(SkShared& s, int n, double lambda, int lane, double (&inv)[2]) {
  inv[0] = 0.0; inv[1] = 0.0;
  for (int j = 0; j < n; ++j) {
    __syncthreads();                                                  // column j - 1 is in Lm
    const int fj = 3 * s.first[j / 3];
    double v[2] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < j || i >= n) continue;
      const int fi = 3 * s.first[i / 3];
      if (j < fi) continue;                                           // outside the envelope: L_ij = 0
      double a = s.H[sk_idx(i, j)];
      if (i == j) a *= 1.0 + lambda;
      for (int k = fi > fj ? fi : fj; k < j; ++k) a -= s.Lm[sk_idx(i, k)] * s.Lm[sk_idx(j, k)];
      v[h] = a;
    }
    const double d = j < 64 ? __shfl(v[0], j, 64) : __shfl(v[1], j - 64, 64);
    if (!(d > 0.0)) return false;                                     // the same d on every lane; NaN fails too
    const double sd = sqrt(d);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < j || i >= n) continue;
      s.Lm[sk_idx(i, j)] = i == j ? sd : v[h] / sd;
      if (i == j) inv[h] = 1.0 / sd;
    }
  }
  __syncthreads();
  return true;
}

// Lm Lm^T d = -g; d[h] = the entry of rows lane + 64 h.  The right-hand side never leaves the registers: column j's value is
// read from its lane, and the factor's next column is loaded while this one is applied.
__device__ __forceinline__ void sk_solve(const SkShared& s, int n, int lane, const double (&inv)[2], double (&d)[2]) {
  const int i0 = lane, i1 = lane + 64;
  d[0] = i0 < n ? -s.g[i0] : 0.0;
  d[1] = i1 < n ? -s.g[i1] : 0.0;
  auto below = [&](int i, int j) { return i > j && i < n ? s.Lm[sk_idx(i, j)] : 0.0; };   // L_ij, column j
  auto left = [&](int i, int j) { return i < j ? s.Lm[sk_idx(j, i)] : 0.0; };             // L_ji, row j
  double c0 = below(i0, 0), c1 = below(i1, 0);
  for (int j = 0; j < n; ++j) {
    const double n0 = below(i0, j + 1), n1 = below(i1, j + 1);
    const double y = j < 64 ? __shfl(d[0] * inv[0], j, 64) : __shfl(d[1] * inv[1], j - 64, 64);
    d[0] = i0 == j ? y : d[0] - c0 * y;
    d[1] = i1 == j ? y : d[1] - c1 * y;
    c0 = n0; c1 = n1;
  }
  c0 = left(i0, n - 1); c1 = left(i1, n - 1);
  for (int j = n - 1; j >= 0; --j) {
    const double n0 = j > 0 ? left(i0, j - 1) : 0.0, n1 = j > 0 ? left(i1, j - 1) : 0.0;
    const double y = j < 64 ? __shfl(d[0] * inv[0], j, 64) : __shfl(d[1] * inv[1], j - 64, 64);
    d[0] = i0 == j ? y : d[0] - c0 * y;
    d[1] = i1 == j ? y : d[1] - c1 * y;
    c0 = n0; c1 = n1;
  }
}

__global__ __launch_bounds__(64) void triangulate_skeleton_kernel(const float* __restrict__ pts, const float* __restrict__ P,
                                                                  const float* __restrict__ init,
                                                                  const unsigned char* __restrict__ views, SkLimbs limbs, int V,
                                                                  int K, int L, int flags, float huber_, float sym_w_,
                                                                  int max_iter, float* __restrict__ out, float* __restrict__ resid,
                                                                  float* __restrict__ sym, float* __restrict__ cost,
                                                                  unsigned char* __restrict__ status) {
  __shared__ SkShared s;
  const int b = blockIdx.x, lane = threadIdx.x;
  const double huber = (double)huber_, sym_w = (double)sym_w_;
  for (int t = lane; t < V * 12; t += 64) s.P[t / 12][t % 12] = P[(size_t)b * V * 12 + t];
  for (int t = lane; t < L * 4; t += 64) s.lj[t / 4][t % 4] = limbs.j[t / 4][t % 4];
  // lane = joint: its points, the views it uses (the rules of triangulate_refine_kernel) and its start
  const size_t i = (size_t)b * K + (lane < K ? lane : 0);
  float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
  int nused = 0;
  bool cand = false;
  if (lane < K) {
    int valid = 0;
    for (int v = 0; v < V; ++v) {
      const float* q = pts + (((size_t)b * V + v) * K + lane) * 3;
      s.pu[lane][v] = q[0]; s.pv[lane][v] = q[1];
      s.ps[lane][v] = (flags & XAS_REFINE_WEIGHTED) ? q[2] : 1.f;
      valid |= (q[2] > 0.f && q[2] < INFINITY) ? 1 << v : 0;
    }
    const int sel = views ? views[i] : 0;
    const int used = sel ? (valid & sel) : valid;
    s.used[lane] = used;
    nused = __popc(used);
    const float* in = init + i * 4;
    x0 = in[0]; x1 = in[1]; x2 = in[2]; x3 = in[3];
    s.X[0][lane][0] = (double)x0; s.X[0][lane][1] = (double)x1; s.X[0][lane][2] = (double)x2;
    cand = nused >= 2 && fabsf(x0) < INFINITY && fabsf(x1) < INFINITY && fabsf(x2) < INFINITY;
  }
  const unsigned candmask = (unsigned)__ballot(cand);
  double Ck, r2k;
  bool frontk;
  sk_reproj(s, 0, V, K, candmask, huber, lane, Ck, r2k, frontk);      // its first barrier publishes the staging above
  const bool isfree = cand && frontk;                                 // FREE: triangulate_refine would not pass it through
  const unsigned freemask = (unsigned)__ballot(isfree);
  const int nfree = __popc(freemask), n = 3 * nfree;
  const int myslot = __popc(freemask & ((1u << (lane & 31)) - 1u));    // read where lane < K <= 24 only
  if (lane < K) s.slot[lane] = isfree ? myslot : -1;
  if (isfree) s.joint[myslot] = lane;
  bool act = lane < L;
  if (act)
#pragma unroll
    for (int m = 0; m < 4; ++m) act = act && ((freemask >> limbs.j[lane & (kSkL - 1)][m]) & 1);
  const unsigned active = (unsigned)__ballot(act);
  __syncthreads();
  if (isfree) {                                                       // the envelope: the lowest slot a limb couples this joint to
    int f = myslot;
    for (int l = 0; l < L; ++l)
      if (((active >> l) & 1) && sk_touches(s, l, lane))
#pragma unroll
        for (int m = 0; m < 4; ++m) f = min(f, s.slot[s.lj[l][m]]);
    s.first[myslot] = f;
  }
  const double e_init = sk_limbs(s, 0, L, active, lane);
  double r2_init = r2k, r2_cur = r2k, e_cur = e_init;
  double C = lane0(wave_sum_d(isfree ? Ck : 0.0) + sym_w * wave_sum_d(e_init * e_init));
  const double C_init = C;
  int cur = 0, st = 1;
  if (nfree > 0) {
    sk_assemble(s, 0, V, nfree, L, active, sym_w, lane);
    double lambda = 1e-3;
    for (int it = 0; it < max_iter; ++it) {
      double inv[2], d[2];
      bool accept = false;
      double Ct = 0.0, r2t = 0.0, et = 0.0, big = 0.0;
      if (sk_factor(s, n, lambda, lane, inv)) {
        sk_solve(s, n, lane, inv, d);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int u = lane + 64 * h;
          if (u < n) s.X[cur ^ 1][s.joint[u / 3]][u % 3] = s.X[cur][s.joint[u / 3]][u % 3] + d[h];
          else d[h] = 0.0;
        }
        big = lane0(wave_max_d(fmax(fabs(d[0]), fabs(d[1]))));
        double Ckt;
        bool frontt;
        sk_reproj(s, cur ^ 1, V, K, freemask, huber, lane, Ckt, r2t, frontt);
        et = sk_limbs(s, cur ^ 1, L, active, lane);
        Ct = lane0(wave_sum_d(isfree ? Ckt : 0.0) + sym_w * wave_sum_d(et * et));
        accept = __all(frontt) && Ct < C;                             // NaN never passes
      }
      if (accept) {
        cur ^= 1; C = Ct; r2_cur = r2t; e_cur = et;
        lambda *= 0.1;
        if (big < 1e-5) { st = 0; break; }
        sk_assemble(s, cur, V, nfree, L, active, sym_w, lane);
      } else {
        lambda *= 10.0;
        if (lambda > 1e12) break;
      }
    }
  }
  if (lane < K) {
    float* o = out + i * 4;
    o[3] = x3;
    if (isfree) {
      o[0] = (float)s.X[cur][lane][0]; o[1] = (float)s.X[cur][lane][1]; o[2] = (float)s.X[cur][lane][2];
    } else {                                                          // fixed: init bit for bit, NaN stays NaN
      o[0] = x0; o[1] = x1; o[2] = x2;
    }
    if (resid) {
      resid[i * 2] = isfree ? (float)sqrt(r2_init / (double)nused) : NAN;
      resid[i * 2 + 1] = isfree ? (float)sqrt(r2_cur / (double)nused) : NAN;
    }
    if (status) status[i] = isfree ? (unsigned char)st : 2;
  }
  if (sym && lane < L) {
    sym[((size_t)b * L + lane) * 2] = act ? (float)e_init : NAN;
    sym[((size_t)b * L + lane) * 2 + 1] = act ? (float)e_cur : NAN;
  }
  if (cost && lane == 0) { cost[(size_t)b * 2] = (float)C_init; cost[(size_t)b * 2 + 1] = (float)C; }
}

// ------------------------------------------------------------------------------------------------------
// multiview_consistency: the training step's multi-view term and its backward pass through the DLT's null vector, thread per
// (b, joint) as triangulate_kernel.  [B,V,K]-sized data and a 4x4 eigenproblem per joint in double: latency-bound.  Every loop
// over the views is unrolled to XAS_TRI_MAX_VIEWS and predicated by the view count or the mask of the valid views, so no
// array is indexed at run time and no view >= V is ever read.  A thread writes only its own joint's outputs: no atomics.
// ------------------------------------------------------------------------------------------------------
// What both passes know about one joint after the solve.
struct MvJoint {
  double u[XAS_TRI_MAX_VIEWS], v[XAS_TRI_MAX_VIEWS];                  // image pixels of every view < V
  double i00[XAS_TRI_MAX_VIEWS], i01[XAS_TRI_MAX_VIEWS], i10[XAS_TRI_MAX_VIEWS], i11[XAS_TRI_MAX_VIEWS];   // inverse crop affines
  float c[XAS_TRI_MAX_VIEWS];                                         // the views' weights (1 without)
  double G[10];                                                       // Gram matrix over the valid views, upper triangle
  double x[4];                                                        // its null vector
  double X[4];                                                        // (x[:3] / x[3], 1)
  int valid, n;
};

// The patch stage of patch_to_world_fwd_kernel (geometry.hip) in fp32, rounding for rounding what the compiler makes of it there:
// every product and difference rounded on its own, but for one fused multiply-add per coordinate, u = fma(i00, du, i01 dv) and
// v = fma(i11, dv, i10 du).  Contraction is switched off here because __fmul_rn and its kin do not stop it (left to itself
// the compiler fuses (x + 1) / 2 (S - 1) - t0 in this kernel and not in that one), and a point moves by 1e-4 mm with the last
// bit of u.  So the DLT starts from the very numbers triangulate_kernel gets from xas_patch_to_world_fwd with XAS_GEO_IMAGE.
__device__ __forceinline__ void mv_patch_stage(const float* __restrict__ A, const float* __restrict__ q, float S, float& u, float& v,
                                               float& i00, float& i01, float& i10, float& i11) {
#pragma clang fp contract(off)
  const float a00 = A[0], a01 = A[1], a10 = A[3], a11 = A[4];
  const float m0 = a00 * a11, m1 = a01 * a10;
  const float det = m0 - m1;
  i00 = a11 / det; i01 = -a01 / det; i10 = -a10 / det; i11 = a00 / det;
  const float h0 = (q[0] + 1.f) / 2.f, h1 = (q[1] + 1.f) / 2.f;
  const float p0 = h0 * (S - 1.f), p1 = h1 * (S - 1.f);
  const float du = p0 - A[2], dv = p1 - A[5];
  const float t0 = i01 * dv, t1 = i10 * du;
  u = __builtin_fmaf(i00, du, t0);
  v = __builtin_fmaf(i11, dv, t1);
}

// Patch stage, validity, Gram matrix and null vector of joint (b, k).  false: passed through.
__device__ __forceinline__ bool mv_solve(const float* __restrict__ kps_xy, const float* __restrict__ ti,
                                         const float* __restrict__ P, const float* __restrict__ weight, int b, int k, int V,
                                         int K, float S, MvJoint& j) {
  double g[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) g[r][cc] = 0.0;
  j.valid = 0;
#pragma unroll
  for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v) {
    j.u[v] = 0.0; j.v[v] = 0.0; j.c[v] = 0.f;
    j.i00[v] = 0.0; j.i01[v] = 0.0; j.i10[v] = 0.0; j.i11[v] = 0.0;
    if (v < V) {
      const size_t bv = (size_t)b * V + v;
      float uf, vf, i00, i01, i10, i11;
      mv_patch_stage(ti + bv * 6, kps_xy + (bv * K + k) * 2, S, uf, vf, i00, i01, i10, i11);
      j.u[v] = (double)uf; j.v[v] = (double)vf;
      j.i00[v] = (double)i00; j.i01[v] = (double)i01; j.i10[v] = (double)i10; j.i11[v] = (double)i11;
      j.c[v] = weight ? weight[bv * K + k] : 1.f;
      if (j.c[v] > 0.f && j.c[v] < INFINITY) {                        // the rule of triangulate_robust_kernel
        j.valid |= 1 << v;
        double t[10];
        dlt_view_gram(uf, vf, j.c[v], P + bv * 12, t);
        dlt_gram_add(g, t);
      }
    }
  }
  j.n = __popc(j.valid);
  int m = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int cc = r; cc < 4; ++cc) j.G[m++] = g[r][cc];
  if (j.n < 2) return false;
  double x[4];                                                        // not j.x: what the call takes by reference lives in scratch
  dlt_null_vector(g, x);
#pragma unroll
  for (int r = 0; r < 4; ++r) j.x[r] = x[r];
  j.X[0] = j.x[0] / j.x[3]; j.X[1] = j.x[1] / j.x[3]; j.X[2] = j.x[2] / j.x[3]; j.X[3] = 1.0;
  if (!(fabs(j.X[0]) < INFINITY && fabs(j.X[1]) < INFINITY && fabs(j.X[2]) < INFINITY)) return false;
  bool front = true;
#pragma unroll
  for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v)
    if ((j.valid >> v) & 1) {
      double h[3];
      front = project_view(P + ((size_t)b * V + v) * 12, j.X, h) && front;
    }
  return front;
}

// argmin_h |world[b][v][h][k] - X|^2 of one view: first minimum, NaN or inf never wins (the rule of multiview_resolve_kernel).
__device__ __forceinline__ int mv_nearest(const float* __restrict__ world, size_t bv, int Hy, int K, int k, const double (&X)[4],
                                          double (&d)[3]) {
  int hs = 0;
  double best = INFINITY;
  for (int h = 0; h < Hy; ++h) {
    const float* wp = world + ((bv * Hy + h) * K + k) * 3;
    const double d0 = (double)wp[0] - X[0], d1 = (double)wp[1] - X[1], d2 = (double)wp[2] - X[2];
    const double dd = d0 * d0 + d1 * d1 + d2 * d2;
    if (dd < best) { best = dd; hs = h; }
  }
  const float* wp = world + ((bv * Hy + hs) * K + k) * 3;
  d[0] = (double)wp[0] - X[0]; d[1] = (double)wp[1] - X[1]; d[2] = (double)wp[2] - X[2];
  return hs;
}

__global__ __launch_bounds__(64) void multiview_consistency_fwd_kernel(
    const float* __restrict__ kps_xy, const float* __restrict__ ti, const float* __restrict__ world, const float* __restrict__ P,
    const float* __restrict__ weight, int B, int V, int Hy, int K, float S, float huber_, float* __restrict__ reproj,
    float* __restrict__ depth, float* __restrict__ xyz, int* __restrict__ hsel, unsigned char* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i % K;
  MvJoint j;
  const bool solved = mv_solve(kps_xy, ti, P, weight, b, k, V, K, S, j);
  const double huber = (double)huber_;
  double rsum = 0.0, dsum = 0.0;
#pragma unroll
  for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v) {
    if (v >= V) continue;
    const size_t bv = (size_t)b * V + v;
    int hs = 0;
    if (solved) {
      double d[3];
      hs = mv_nearest(world, bv, Hy, K, k, j.X, d);
      if ((j.valid >> v) & 1) {
        dsum += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        double h[3];
        project_view(P + bv * 12, j.X, h);
        const double ru = h[0] / h[2] - j.u[v], rv = h[1] / h[2] - j.v[v];
        const double e = sqrt(ru * ru + rv * rv);
        rsum += (huber > 0.0 && e > huber) ? 2.0 * huber * e - huber * huber : ru * ru + rv * rv;
      }
    }
    hsel[bv * K + k] = hs;
  }
  reproj[i] = solved ? (float)(rsum / (double)j.n) : 0.f;
  depth[i] = solved ? (float)(dsum / (double)j.n) : 0.f;
#pragma unroll
  for (int r = 0; r < 3; ++r) xyz[(size_t)i * 3 + r] = solved ? (float)j.X[r] : NAN;
  status[i] = solved ? 0 : 2;
}

__global__ __launch_bounds__(64) void multiview_consistency_bwd_kernel(
    const float* __restrict__ kps_xy, const float* __restrict__ ti, const float* __restrict__ world, const float* __restrict__ P,
    const float* __restrict__ weight, const float* __restrict__ g_reproj, const float* __restrict__ g_depth, int B, int V, int Hy,
    int K, float S, float huber_, int flags, float* __restrict__ grad_kps_xy, float* __restrict__ grad_world) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i % K;
  MvJoint j;
  const bool solved = mv_solve(kps_xy, ti, P, weight, b, k, V, K, S, j);
  const double huber = (double)huber_;
  const double a = solved ? (double)g_reproj[i] / (double)j.n : 0.0, dw = solved ? (double)g_depth[i] / (double)j.n : 0.0;
  double gu[XAS_TRI_MAX_VIEWS], gv[XAS_TRI_MAX_VIEWS];                // d / d (u_v, v_v)
  double gX[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v) {
    gu[v] = 0.0; gv[v] = 0.0;
    if (v >= V) continue;
    const size_t bv = (size_t)b * V + v;
    const bool on = solved && ((j.valid >> v) & 1);
    int hs = 0;
    double d[3] = {0.0, 0.0, 0.0};
    if (on) {
      hs = mv_nearest(world, bv, Hy, K, k, j.X, d);
      const float* Pm = P + bv * 12;
      double h[3];
      project_view(Pm, j.X, h);
      const double pu = h[0] / h[2], pv = h[1] / h[2];
      const double ru = pu - j.u[v], rv = pv - j.v[v];
      const double e = sqrt(ru * ru + rv * rv);
      const double wt = 2.0 * a * ((huber > 0.0 && e > huber) ? huber / e : 1.0);
      gu[v] = -wt * ru; gv[v] = -wt * rv;
#pragma unroll
      for (int n = 0; n < 3; ++n) {
        const double ju = ((double)Pm[n] - pu * (double)Pm[8 + n]) / h[2], jv = ((double)Pm[4 + n] - pv * (double)Pm[8 + n]) / h[2];
        gX[n] += wt * (ju * ru + jv * rv) - 2.0 * dw * d[n];
      }
    }
    for (int h = 0; h < Hy; ++h) {                                    // every hypothesis of every view < V is written
      float* o = grad_world + ((bv * Hy + h) * K + k) * 3;
      const bool sel = on && h == hs;
#pragma unroll
      for (int n = 0; n < 3; ++n) o[n] = sel ? (float)(2.0 * dw * d[n]) : 0.f;
    }
  }
  if (solved && !(flags & XAS_MV_DETACH_TARGET)) {
    // through X: all four eigenpairs of G.  x itself stays dlt_null_vector's, the one the forward pass solved with
    double g[4][4], vec[4][4];
    int m = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int cc = r; cc < 4; ++cc) { g[r][cc] = j.G[m]; g[cc][r] = j.G[m]; ++m; }
    jacobi4(g, vec);
    int best = 0;
    double lo = g[0][0];
#pragma unroll
    for (int n = 1; n < 4; ++n)
      if (g[n][n] < lo) { lo = g[n][n]; best = n; }
    double next = INFINITY, hi = lo;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      if (n != best && g[n][n] < next) next = g[n][n];
      if (g[n][n] > hi) hi = g[n][n];
    }
    // lambda_1 - lambda_0 below what the eigenvectors of a double G resolve (views that coincide, rays that are parallel): x is
    // any vector of a plane there and has no derivative, so the term is left out and the joint gets its detached gradient
    const bool gap = next - lo > XAS_MV_MIN_GAP * hi;
    const double x3 = j.x[3];
    const double gx[4] = {gX[0] / x3, gX[1] / x3, gX[2] / x3, -(gX[0] * j.x[0] + gX[1] * j.x[1] + gX[2] * j.x[2]) / (x3 * x3)};
    double mv[4] = {0.0, 0.0, 0.0, 0.0};                              // sum_j (v_j . g_x) / (lambda_0 - lambda_j) v_j:  g_G = sym(mv x^T)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      if (n == best || !gap) continue;
      const double cf = (vec[0][n] * gx[0] + vec[1][n] * gx[1] + vec[2][n] * gx[2] + vec[3][n] * gx[3]) / (lo - g[n][n]);
#pragma unroll
      for (int r = 0; r < 4; ++r) mv[r] += cf * vec[r][n];
    }
#pragma unroll
    for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v)
      if ((j.valid >> v) & 1) {
        const float* Pm = P + ((size_t)b * V + v) * 12;
        double mp2 = 0.0, xp2 = 0.0, aum = 0.0, aux = 0.0, avm = 0.0, avx = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double p2 = (double)Pm[8 + r];
          const double au = j.u[v] * p2 - (double)Pm[r], av = j.v[v] * p2 - (double)Pm[4 + r];
          mp2 += mv[r] * p2; xp2 += j.x[r] * p2;
          aum += au * mv[r]; aux += au * j.x[r];
          avm += av * mv[r]; avx += av * j.x[r];
        }
        const double c2 = (double)j.c[v] * (double)j.c[v];            // 2 c^2 a^T sym(mv x^T) P2
        gu[v] += c2 * (aum * xp2 + aux * mp2);
        gv[v] += c2 * (avm * xp2 + avx * mp2);
      }
  }
  const double half = ((double)S - 1.0) / 2.0;
#pragma unroll
  for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v)
    if (v < V) {
      float* o = grad_kps_xy + (((size_t)b * V + v) * K + k) * 2;
      const bool on = solved && ((j.valid >> v) & 1);                 // exact zeros elsewhere, whatever the affine holds
      o[0] = on ? (float)((j.i00[v] * gu[v] + j.i10[v] * gv[v]) * half) : 0.f;
      o[1] = on ? (float)((j.i01[v] * gu[v] + j.i11[v] * gv[v]) * half) : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------
// triangulate_volume: volumetric fusion of the views' heat-map cubes (eval.py --tri-volume; xas_hip.h has the arithmetic).
// One workgroup of 256 threads per (b, joint).  The camera constants of the workgroup's sample sit in LDS as doubles, one
// VolView per view, written once by thread v.  Per level the G^3 voxels are strided over the threads; every thread keeps an
// online-softmax record (VolRec) of its voxels, the records of a wave merge by a butterfly of shuffles (the merge is
// symmetric bit for bit, so every lane ends with the same record), the four waves' records through LDS in wave order by
// thread 0, which also moves the centre for the next level.  No atomics: the result is a pure function of the inputs.
// A sample reads the 2x2x2 logits round its clamped point as four pairs: the two depth neighbours are adjacent floats.
// ------------------------------------------------------------------------------------------------------
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
    c.take = sel && wt > 0.f && wt < INFINITY && ch >= 0 && ch < K;
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

// ------------------------------------------------------------------------------------------------------
// pose_metrics: one wave per sample, lane = joint.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float norm3(float a, float b, float c) {
  return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), __fmul_rn(c, c)));
}

__global__ __launch_bounds__(64) void pose_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                          const unsigned char* __restrict__ mask, int K, float in_div,
                                                          int pck_align, float pck_threshold, float* __restrict__ err,
                                                          float* __restrict__ aligned, float* __restrict__ pck,
                                                          int* __restrict__ auc_hits, long NK) {
  const int n = blockIdx.x, k = threadIdx.x;
  const bool on = k < K;
  float p[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f};
  if (on) {
    for (int c = 0; c < 3; ++c) {
      p[c] = pred[((size_t)n * K + k) * 3 + c] / in_div;
      g[c] = gt[((size_t)n * K + k) * 3 + c] / in_div;
    }
  }
  const float vis = on ? (mask ? (mask[(size_t)n * K + k] ? 1.f : 0.f) : 1.f) : 0.f;
  float e[3];
  e[0] = norm3(p[0] - g[0], p[1] - g[1], p[2] - g[2]);
  // --- scale alignment (metrics.py:106-110): all joints, visible or not
  const double pp = wave_sum_d(on ? (double)p[0] * p[0] + (double)p[1] * p[1] + (double)p[2] * p[2] : 0.0);
  const double pg = wave_sum_d(on ? (double)p[0] * g[0] + (double)p[1] * g[1] + (double)p[2] * g[2] : 0.0);
  const float f = (float)(pg / pp);
  float a1[3] = {p[0] * f, p[1] * f, p[2] * f};
  e[1] = norm3(a1[0] - g[0], a1[1] - g[1], a1[2] - g[2]);
  // --- procrustes (metrics.py:5-62)
  const double invK = 1.0 / (double)K;
  double mu1[3], mu2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    mu1[c] = wave_sum_d(on ? (double)p[c] : 0.0) * invK;
    mu2[c] = wave_sum_d(on ? (double)g[c] : 0.0) * invK;
  }
  double x1[3], x2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { x1[c] = on ? p[c] - mu1[c] : 0.0; x2[c] = on ? g[c] - mu2[c] : 0.0; }
  const double var1 = wave_sum_d(x1[0] * x1[0] + x1[1] * x1[1] + x1[2] * x1[2]);
  double S[3][3];                                                     // S = sum src dst^T  (K of metrics.py:38)
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) S[r][c] = wave_sum_d(x1[r] * x2[c]);
  double N4[4][4], Q[4][4];
  N4[0][0] = S[0][0] + S[1][1] + S[2][2];
  N4[0][1] = S[1][2] - S[2][1]; N4[0][2] = S[2][0] - S[0][2]; N4[0][3] = S[0][1] - S[1][0];
  N4[1][1] = S[0][0] - S[1][1] - S[2][2]; N4[1][2] = S[0][1] + S[1][0]; N4[1][3] = S[2][0] + S[0][2];
  N4[2][2] = -S[0][0] + S[1][1] - S[2][2]; N4[2][3] = S[1][2] + S[2][1];
  N4[3][3] = -S[0][0] - S[1][1] + S[2][2];
#pragma unroll
  for (int r = 1; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < r; ++c) N4[r][c] = N4[c][r];
  jacobi4(N4, Q);                                                     // every lane solves the same 4x4 (no broadcast needed)
  int best = 0;
  double hi = N4[0][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (N4[j][j] > hi) { hi = N4[j][j]; best = j; }
  double q[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] = best == 0 ? Q[r][0] : (best == 1 ? Q[r][1] : (best == 2 ? Q[r][2] : Q[r][3]));
  const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
  double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                    {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                    {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
  double trRK = 0.0;                                                  // trace(R K) = sum_ij R[i][j] S[j][i]
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) trRK += R[r][c] * S[c][r];
  const double scale = trRK / var1;
  float a2[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    a2[r] = (float)(scale * (R[r][0] * x1[0] + R[r][1] * x1[1] + R[r][2] * x1[2]) + mu2[r]);
  e[2] = norm3(a2[0] - g[0], a2[1] - g[1], a2[2] - g[2]);

  if (!on) return;
  const size_t o = (size_t)n * K + k;
  if (err) { err[o] = e[0] * vis; err[NK + o] = e[1] * vis; err[2 * NK + o] = e[2] * vis; }
  if (aligned) {
    for (int c = 0; c < 3; ++c) { aligned[o * 3 + c] = a1[c]; aligned[(NK + o) * 3 + c] = a2[c]; }
  }
  const float ep = pck_align == 0 ? e[0] : (pck_align == 1 ? e[1] : e[2]);
  if (pck) pck[o] = (ep < pck_threshold ? 100.f : 0.f) * vis;           // metrics.py:172-173
  if (auc_hits) {                                                       // metrics.py:236-240, np.linspace(0, 0.15, 31)
    const double step = 0.15 / 30.0;
    for (int t = 0; t < 31; ++t) {
      const double thr = t == 30 ? 0.15 : t * step;
      const int hit = ((double)ep < thr && vis != 0.f) ? 1 : 0;
      const unsigned long long bal = __ballot(hit);
      if (k == 0) auc_hits[(size_t)n * 31 + t] = __popcll(bal);
    }
  }
}

}  // namespace xas

using namespace xas;

extern "C" int xas_eval_select(const float* kps, const float* joints, const int* perm, int B, int Hy, int K, int C,
                               float image_size, int flags, float* sel3d, float* sel2d, float* err2d,
                               unsigned char* swapped, void* stream) {
  XAS_REQUIRE(kps && joints && perm, "eval_select: null buffer");
  XAS_REQUIRE(B > 0 && Hy > 0 && K > 0 && K <= 64 && (C == 2 || C == 3), "eval_select: bad shape B=%d Hy=%d K=%d C=%d (K <= 64, C in {2,3})", B, Hy, K, C);
  XAS_REQUIRE(image_size > 1.f, "eval_select: image_size %f", (double)image_size);
  hipLaunchKernelGGL(eval_select_kernel, dim3(B), dim3(64), 0, as_stream(stream), kps, joints, perm, Hy, K, C, image_size,
                     flags, sel3d, sel2d, err2d, swapped);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_projection_matrix(const float* k_mat, const float* rot_world, const float* trans_world, int B, float* P,
                                     void* stream) {
  XAS_REQUIRE(k_mat && rot_world && trans_world && P && B > 0, "projection_matrix: bad arguments");
  hipLaunchKernelGGL(projection_kernel, dim3((unsigned)cdiv((long)B * 12, 128)), dim3(128), 0, as_stream(stream), k_mat,
                     rot_world, trans_world, B, P);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_triangulate_dlt(const float* points, const float* P, int B, int V, int K, float* out, void* stream) {
  XAS_REQUIRE(points && P && out, "triangulate_dlt: null buffer");
  XAS_REQUIRE(B > 0 && V >= 2 && K > 0, "triangulate_dlt: bad shape B=%d V=%d K=%d (needs >= 2 views)", B, V, K);
  hipLaunchKernelGGL(triangulate_kernel, dim3((unsigned)cdiv((long)B * K, 64)), dim3(64), 0, as_stream(stream), points, P, B,
                     V, K, out);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_triangulate_robust(const float* points, const float* P, int B, int V, int K, float threshold_px,
                                      float* out, unsigned char* inliers, float* resid, void* stream) {
  XAS_REQUIRE(points && P && out, "triangulate_robust: null buffer (points, P and out are required)");
  XAS_REQUIRE(V >= 2 && V <= XAS_TRI_MAX_VIEWS, "triangulate_robust: V=%d views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = %d)", V,
              XAS_TRI_MAX_VIEWS);
  XAS_REQUIRE(B > 0 && K > 0 && (long)B * K <= 0x7fffffffL, "triangulate_robust: bad shape B=%d K=%d (B, K > 0, B*K < 2^31)", B, K);
  XAS_REQUIRE(threshold_px > 0.f, "triangulate_robust: threshold_px %f (needs a threshold > 0 px)", (double)threshold_px);
  hipLaunchKernelGGL(triangulate_robust_kernel, dim3((unsigned)((long)B * K)), dim3(64), 0, as_stream(stream), points, P, V, K,
                     threshold_px, out, inliers, resid);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_multiview_resolve(const float* points, const float* P, const float* kps, const float* world,
                                     const int* perm, const float* gt, int B, int V, int Hy, int K, float image_size,
                                     float* sel, float* xyzw, unsigned char* swap, unsigned char* hyp,
                                     unsigned char* named, void* stream) {
  XAS_REQUIRE(points && P && kps && world && perm && sel,
              "multiview_resolve: null buffer (points, P, kps, world, perm and sel are required)");
  XAS_REQUIRE(V >= 2 && V <= XAS_TRI_MAX_VIEWS, "multiview_resolve: V=%d views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = %d)", V,
              XAS_TRI_MAX_VIEWS);
  XAS_REQUIRE(K >= 1 && K <= 64, "multiview_resolve: K=%d joints (needs 1 <= K <= 64)", K);
  XAS_REQUIRE(Hy >= 1 && Hy <= 255, "multiview_resolve: Hy=%d hypotheses (needs 1 <= Hy <= 255)", Hy);
  XAS_REQUIRE(B > 0 && (long)B * K <= 0x7fffffffL, "multiview_resolve: bad shape B=%d K=%d (B > 0, B*K < 2^31)", B, K);
  XAS_REQUIRE(!gt || image_size > 1.f, "multiview_resolve: image_size %f (labels need a patch size > 1)", (double)image_size);
  hipLaunchKernelGGL(multiview_resolve_kernel, dim3((unsigned)((long)B * K)), dim3(64), 0, as_stream(stream), points, P, kps,
                     world, perm, gt, V, Hy, K, image_size, sel, xyzw, swap, hyp, named);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_triangulate_refine(const float* points, const float* P, const float* init, const unsigned char* views,
                                      int B, int V, int K, int flags, float huber, int max_iter, float* out, float* resid,
                                      float* cov, unsigned char* status, void* stream) {
  XAS_REQUIRE(points && P && init && out, "triangulate_refine: null buffer (points, P, init and out are required)");
  XAS_REQUIRE(V >= 2 && V <= XAS_TRI_MAX_VIEWS, "triangulate_refine: V=%d views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = %d)", V,
              XAS_TRI_MAX_VIEWS);
  XAS_REQUIRE(B > 0 && K >= 1 && (long)B * K <= 0x7fffffffL, "triangulate_refine: bad shape B=%d K=%d (B > 0, K >= 1, B*K < 2^31)", B, K);
  XAS_REQUIRE(max_iter >= 1 && max_iter <= 64, "triangulate_refine: max_iter=%d trials (needs 1 <= max_iter <= 64)", max_iter);
  XAS_REQUIRE((flags & ~XAS_REFINE_WEIGHTED) == 0, "triangulate_refine: unknown flag bits 0x%x (XAS_REFINE_WEIGHTED = %d is the only flag)",
              flags & ~XAS_REFINE_WEIGHTED, XAS_REFINE_WEIGHTED);
  hipLaunchKernelGGL(triangulate_refine_kernel, dim3((unsigned)cdiv((long)B * K, 64)), dim3(64), 0, as_stream(stream), points, P,
                     init, views, B, V, K, flags, huber, max_iter, out, resid, cov, status);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_triangulate_skeleton(const float* points, const float* P, const float* init, const unsigned char* views,
                                        const int* limbs, int B, int V, int K, int L, int flags, float huber, float sym_w,
                                        int max_iter, float* out, float* resid, float* sym, float* cost, unsigned char* status,
                                        void* stream) {
  XAS_REQUIRE(points && P && init && out, "triangulate_skeleton: null buffer (points, P, init and out are required)");
  XAS_REQUIRE(out != init, "triangulate_skeleton: out must not overlap init (a fixed joint is copied from it)");
  XAS_REQUIRE(V >= 2 && V <= XAS_TRI_MAX_VIEWS, "triangulate_skeleton: V=%d views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = %d)", V,
              XAS_TRI_MAX_VIEWS);
  XAS_REQUIRE(K >= 3 && K <= XAS_SKEL_MAX_JOINTS, "triangulate_skeleton: K=%d joints (needs 3 <= K <= XAS_SKEL_MAX_JOINTS = %d)", K,
              XAS_SKEL_MAX_JOINTS);
  XAS_REQUIRE(L >= 0 && L <= XAS_SKEL_MAX_LIMBS, "triangulate_skeleton: L=%d limb pairs (needs 0 <= L <= XAS_SKEL_MAX_LIMBS = %d)", L,
              XAS_SKEL_MAX_LIMBS);
  XAS_REQUIRE(B > 0 && (long)B * K <= 0x7fffffffL, "triangulate_skeleton: bad shape B=%d K=%d (B > 0, B*K < 2^31)", B, K);
  XAS_REQUIRE(max_iter >= 1 && max_iter <= 64, "triangulate_skeleton: max_iter=%d trials (needs 1 <= max_iter <= 64)", max_iter);
  XAS_REQUIRE((flags & ~XAS_REFINE_WEIGHTED) == 0, "triangulate_skeleton: unknown flag bits 0x%x (XAS_REFINE_WEIGHTED = %d is the only flag)",
              flags & ~XAS_REFINE_WEIGHTED, XAS_REFINE_WEIGHTED);
  XAS_REQUIRE(sym_w >= 0.f && sym_w < INFINITY, "triangulate_skeleton: sym_w %f (needs a finite sym_w >= 0)", (double)sym_w);
  XAS_REQUIRE(L == 0 || limbs, "triangulate_skeleton: null limbs with L=%d (a host array [L][4])", L);
  SkLimbs table = {};
  for (int l = 0; l < L; ++l)
    for (int m = 0; m < 4; ++m) {
      const int j = limbs[4 * l + m];
      XAS_REQUIRE(j >= 0 && j < K, "triangulate_skeleton: limbs[%d][%d] = %d is no joint (needs 0 <= index < K = %d)", l, m, j, K);
      table.j[l][m] = j;
    }
  hipLaunchKernelGGL(triangulate_skeleton_kernel, dim3((unsigned)B), dim3(64), 0, as_stream(stream), points, P, init, views, table,
                     V, K, L, flags, huber, sym_w, max_iter, out, resid, sym, cost, status);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_triangulate_volume(const float* const* logits, const int* chan, const float* trans_image, const float* k_mat,
                                      const float* pelvis, const float* rot_world, const float* trans_world, const float* init,
                                      const unsigned char* views, const float* weight, int B, int V, int K, int D, int G,
                                      int levels, float side_mm, float beta, float out_penalty, float image_size,
                                      float rect_width, float* xyz, float* cov, unsigned char* status, void* stream) {
  XAS_REQUIRE(logits && trans_image && k_mat && pelvis && rot_world && trans_world && init && xyz,
              "triangulate_volume: null buffer (logits, the five camera arrays, init and xyz are required)");
  XAS_REQUIRE(D >= 4 && D <= 128 && D % 4 == 0, "triangulate_volume: D=%d cells per side (needs a multiple of 4 in [4,128], the head's range)", D);
  XAS_REQUIRE(V >= 1 && V <= XAS_TRI_MAX_VIEWS, "triangulate_volume: V=%d views (needs 1 <= V <= XAS_TRI_MAX_VIEWS = %d)", V,
              XAS_TRI_MAX_VIEWS);
  XAS_REQUIRE(G >= 2 && G <= 32, "triangulate_volume: G=%d voxels per side (needs 2 <= G <= 32)", G);
  XAS_REQUIRE(levels >= 1 && levels <= 4, "triangulate_volume: levels=%d (needs 1 <= levels <= 4)", levels);
  XAS_REQUIRE(side_mm > 0.f && side_mm < INFINITY, "triangulate_volume: side_mm %f (needs a finite side > 0 mm)", (double)side_mm);
  XAS_REQUIRE(beta > 0.f && beta < INFINITY, "triangulate_volume: beta %f (needs a finite beta > 0)", (double)beta);
  XAS_REQUIRE(out_penalty > 0.f && out_penalty < INFINITY, "triangulate_volume: out_penalty %f (needs a finite out_penalty > 0)",
              (double)out_penalty);
  XAS_REQUIRE(B > 0 && K >= 1 && (long)B * K <= 0x7fffffffL, "triangulate_volume: bad shape B=%d K=%d (B > 0, K >= 1, B*K < 2^31)", B, K);
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

// The argument checks that the two passes of the multi-view term share.
static int mv_check(const char* who, int B, int V, int Hy, int K, float image_size, float huber_px, int flags) {
  XAS_REQUIRE(V >= 2 && V <= XAS_TRI_MAX_VIEWS, "%s: V=%d views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = %d)", who, V, XAS_TRI_MAX_VIEWS);
  XAS_REQUIRE(Hy >= 1 && Hy <= 8, "%s: Hy=%d hypotheses (needs 1 <= Hy <= 8)", who, Hy);
  XAS_REQUIRE(B >= 1 && K >= 1 && (long)B * K <= 0x7fffffffL, "%s: bad shape B=%d K=%d (B >= 1, K >= 1, B*K < 2^31)", who, B, K);
  XAS_REQUIRE(image_size > 1.f, "%s: image_size %f (needs a patch size > 1)", who, (double)image_size);
  XAS_REQUIRE(huber_px >= 0.f && huber_px < INFINITY, "%s: huber_px %f (needs a finite huber_px >= 0; 0 = squared loss)", who,
              (double)huber_px);
  XAS_REQUIRE((flags & ~XAS_MV_DETACH_TARGET) == 0, "%s: unknown flag bits 0x%x (XAS_MV_DETACH_TARGET = %d is the only flag)", who,
              flags & ~XAS_MV_DETACH_TARGET, XAS_MV_DETACH_TARGET);
  return 0;
}

extern "C" int xas_multiview_consistency_fwd(const float* kps_xy, const float* trans_image, const float* world, const float* P,
                                             const float* weight, int B, int V, int Hy, int K, float image_size, float huber_px,
                                             int flags, float* reproj, float* depth, float* xyz, int* hsel,
                                             unsigned char* status, void* stream) {
  XAS_REQUIRE(kps_xy && trans_image && world && P && reproj && depth && xyz && hsel && status,
              "multiview_consistency_fwd: null buffer (everything but weight is required)");
  if (mv_check("multiview_consistency_fwd", B, V, Hy, K, image_size, huber_px, flags)) return 1;
  hipLaunchKernelGGL(multiview_consistency_fwd_kernel, dim3((unsigned)cdiv((long)B * K, 64)), dim3(64), 0, as_stream(stream),
                     kps_xy, trans_image, world, P, weight, B, V, Hy, K, image_size, huber_px, reproj, depth, xyz, hsel, status);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_multiview_consistency_bwd(const float* kps_xy, const float* trans_image, const float* world, const float* P,
                                             const float* weight, const float* g_reproj, const float* g_depth, int B, int V,
                                             int Hy, int K, float image_size, float huber_px, int flags, float* grad_kps_xy,
                                             float* grad_world, void* stream) {
  XAS_REQUIRE(kps_xy && trans_image && world && P && g_reproj && g_depth && grad_kps_xy && grad_world,
              "multiview_consistency_bwd: null buffer (everything but weight is required)");
  if (mv_check("multiview_consistency_bwd", B, V, Hy, K, image_size, huber_px, flags)) return 1;
  hipLaunchKernelGGL(multiview_consistency_bwd_kernel, dim3((unsigned)cdiv((long)B * K, 64)), dim3(64), 0, as_stream(stream),
                     kps_xy, trans_image, world, P, weight, g_reproj, g_depth, B, V, Hy, K, image_size, huber_px, flags,
                     grad_kps_xy, grad_world);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_pose_metrics(const float* pred, const float* gt, const unsigned char* mask, int N, int K, float in_div,
                                int pck_align, float pck_threshold, float* err, float* aligned, float* pck,
                                int* auc_hits, void* stream) {
  XAS_REQUIRE(pred && gt, "pose_metrics: null buffer");
  XAS_REQUIRE(N > 0 && K >= 3 && K <= 64, "pose_metrics: bad shape N=%d K=%d (3 <= K <= 64)", N, K);
  XAS_REQUIRE(in_div > 0.f && pck_align >= 0 && pck_align <= 2, "pose_metrics: bad in_div / pck_align");
  hipLaunchKernelGGL(pose_metrics_kernel, dim3(N), dim3(64), 0, as_stream(stream), pred, gt, mask, K, in_div, pck_align,
                     pck_threshold, err, aligned, pck, auc_hits, (long)N * K);
  XAS_LAUNCH_CHECK();
  return 0;
}
