// Multi-view triangulation on the device (gfx950): everything that solves the DLT null vector.  Tiny per-joint work (B*K ~ 600
// points, a 4x4 eigenproblem each), latency-bound; see evalpath.hip for why it runs on the device at all.
//   triangulate_dlt : modules/util.py:198-230 (null vector of the weighted DLT system)
//   triangulate_robust : the same DLT over the largest set of views that agree within a pixel threshold (no reference
//                     counterpart: eval.py --tri robust)
//   multiview_resolve : the left/right exchange of every view and the depth hypothesis of every view and joint, decided by the
//                     agreement of the views instead of the labels (stands beside eval_utils.py:7-29 and eval.py:129-148,
//                     on the DLT of modules/util.py:198-230: eval.py --resolve views)
//   multiview_consistency_fwd / _bwd : the TRAINING step's multi-view term, reprojection and depth agreement with the DLT point,
//                     and its backward pass through the null vector (no reference counterpart: train.py --mv-2d / --mv-3d)
// They stay in ONE translation unit, and dlt_null_vector in this file and out of multiview.h: all of them call its one compiled
// body (see its comment), the library has no relocatable device code, and the tests compare their results bit for bit.
// The DLT pieces they share come first.  Rows are formed in fp32 as the reference forms them (util.py:215-221; u P2 - P0 with
// one rounding), then A^T A and its smallest eigenvector are computed in double.
#include "multiview.h"

namespace xas {

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

// g (upper triangle) += one view; g starts as `double g[4][4] = {}`.  All kernels add their views through here in ascending
// view order, so the same set of views gives the same matrix bit for bit.
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
// two then differ in the last bits.  One body that all call makes the same matrix give the same vector by construction.
__device__ __noinline__ void dlt_null_vector(double (&g)[4][4], double (&X)[4]) {
#pragma unroll
  for (int r = 1; r < 4; ++r)
#pragma unroll
    for (int cc = 0; cc < r; ++cc) g[r][cc] = g[cc][r];
  double vec[4][4], lo;
  jacobi4(g, vec);
  jacobi4_column(vec, jacobi4_pick(g, false, lo), X);
}

// ------------------------------------------------------------------------------------------------------
// triangulate_dlt: thread per (b, joint).  points [B][V][K][3] = (u, v, weight), P [B][V][3][4].
// ------------------------------------------------------------------------------------------------------
__global__ void triangulate_kernel(const float* __restrict__ pts, const float* __restrict__ P, int B, int V, int K,
                                   float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i % K;
  double g[4][4] = {};
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
  float P[12], u, v, w, pad;
};

// Point q = (u, v, weight), matrix Pm and the view's DLT contribution into s; -> whether the view is valid.
__device__ __forceinline__ bool tri_stage_view(TriView& s, const float* __restrict__ q, const float* __restrict__ Pm) {
  s.u = q[0]; s.v = q[1]; s.w = q[2]; s.pad = 0.f;
#pragma unroll
  for (int j = 0; j < 12; ++j) s.P[j] = Pm[j];
  dlt_view_gram(s.u, s.v, s.w, Pm, s.gram);
  return view_valid(s.w);
}

// Wave arg-best -> the lane with the smallest key, then the smallest cost (no NaN), then the smallest lane id.  A total order,
// so the xor butterfly leaves the same winner in every lane; what else the winner holds is read from it with __shfl.
__device__ __forceinline__ int wave_arg_best(int key, double cost, int id) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int okey = __shfl_xor(key, o, 64), oid = __shfl_xor(id, o, 64);
    const double ocost = __shfl_xor(cost, o, 64);
    const bool take = okey < key || (okey == key && (ocost < cost || (ocost == cost && oid < id)));
    if (take) { key = okey; id = oid; cost = ocost; }
  }
  return id;
}

// Squared reprojection residual (px^2) of homogeneous X in one view, in double; +inf behind the camera.
__device__ __forceinline__ double reproj_r2(const TriView& s, const double (&X)[4]) {
  const ReprojTerm t = reproj_term(s.P, X, (double)s.u, (double)s.v, 1.0, 0.0);
  return t.front ? t.rr : INFINITY;
}

__global__ __launch_bounds__(64) void triangulate_robust_kernel(const float* __restrict__ pts, const float* __restrict__ P,
                                                                int V, int K, float threshold_px, float* __restrict__ out,
                                                                unsigned char* __restrict__ inliers,
                                                                float* __restrict__ resid) {
  __shared__ TriView sv[XAS_TRI_MAX_VIEWS];
  const int i = blockIdx.x, b = i / K, k = i % K;
  const int lane = threadIdx.x;
  bool ok = false;
  if (lane < V)                                                       // lane v stages view v
    ok = tri_stage_view(sv[lane], pts + (((size_t)b * V + lane) * K + k) * 3, P + ((size_t)b * V + lane) * 12);
  const int valid = (int)__ballot(ok);                                // bits < V only
  __syncthreads();

  // --- candidate = this lane's mask, if it is a set of >= 2 valid views
  const bool cand = (lane & ~valid) == 0 && __popc(lane) >= 2;
  double X[4] = {0.0, 0.0, 0.0, 0.0}, r2[XAS_TRI_MAX_VIEWS];
  int cnt = -1, inl = 0;
  double cost = INFINITY;
  if (cand) {
    double g[4][4] = {};
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
  // --- wave arg-best: more inliers, then smaller sum of squared inlier residuals, then smaller mask
  const int win = wave_arg_best(-cnt, cost, lane), bcnt = __shfl(cnt, win, 64), binl = __shfl(inl, win, 64);
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
// argmin_h |world[bv][h][k] - X|^2 over the depth hypotheses of one view bv = b V + v: the first minimum, and NaN or inf never
// wins (then h = 0).  d = the winner's world point minus X.
__device__ __forceinline__ int nearest_hypothesis(const float* __restrict__ world, size_t bv, int Hy, int K, int k, const double* X,
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
  if (stager) ok = tri_stage_view(sv[j][v], pts + (((size_t)b * V + v) * K + k) * 3, P + ((size_t)b * V + v) * 12);
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
      double g[4][4] = {}, X[4];
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
  // --- wave arg-best: a candidate before none, then the smaller cost, then the smaller mask
  const int best = wave_arg_best(cand ? 0 : 1, cost, lane), win = solved ? best : 0;
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
    const double X[3] = {j ? xc[0] : xa[0], j ? xc[1] : xa[1], j ? xc[2] : xa[2]};
    double d[3];
    hs = nearest_hypothesis(world, (size_t)b * V + v, Hy, K, src, X, d);
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
  double g[4][4] = {};
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
      if (view_valid(j.c[v])) {
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
      hs = nearest_hypothesis(world, bv, Hy, K, k, j.X, d);
      if ((j.valid >> v) & 1) {
        dsum += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        const ReprojTerm t = reproj_term(P + bv * 12, j.X, j.u[v], j.v[v], 1.0, huber);
        rsum += t.tail ? 2.0 * huber * t.e - huber * huber : t.rr;
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
      hs = nearest_hypothesis(world, bv, Hy, K, k, j.X, d);
      const ReprojTerm t = reproj_term(P + bv * 12, j.X, j.u[v], j.v[v], 1.0, huber);
      const double wt = 2.0 * a * t.w;
      gu[v] = -wt * t.ru; gv[v] = -wt * t.rv;
#pragma unroll
      for (int n = 0; n < 3; ++n) gX[n] += wt * t.grad(n) - 2.0 * dw * d[n];
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
    double lo;
    const int best = jacobi4_pick(g, false, lo);
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

}  // namespace xas

using namespace xas;

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
  if (tri_check_views("triangulate_robust", V, 2) || tri_check_shape("triangulate_robust", B, K, "B, K > 0")) return 1;
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
  if (tri_check_views("multiview_resolve", V, 2)) return 1;
  XAS_REQUIRE(K >= 1 && K <= 64, "multiview_resolve: K=%d joints (needs 1 <= K <= 64)", K);
  XAS_REQUIRE(Hy >= 1 && Hy <= 255, "multiview_resolve: Hy=%d hypotheses (needs 1 <= Hy <= 255)", Hy);
  if (tri_check_shape("multiview_resolve", B, K, "B > 0")) return 1;
  XAS_REQUIRE(!gt || image_size > 1.f, "multiview_resolve: image_size %f (labels need a patch size > 1)", (double)image_size);
  hipLaunchKernelGGL(multiview_resolve_kernel, dim3((unsigned)((long)B * K)), dim3(64), 0, as_stream(stream), points, P, kps,
                     world, perm, gt, V, Hy, K, image_size, sel, xyzw, swap, hyp, named);
  XAS_LAUNCH_CHECK();
  return 0;
}

// The argument checks that the two passes of the multi-view term share.
static int mv_check(const char* who, int B, int V, int Hy, int K, float image_size, float huber_px, int flags) {
  if (tri_check_views(who, V, 2)) return 1;
  XAS_REQUIRE(Hy >= 1 && Hy <= 8, "%s: Hy=%d hypotheses (needs 1 <= Hy <= 8)", who, Hy);
  if (tri_check_shape(who, B, K, "B >= 1, K >= 1")) return 1;
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
