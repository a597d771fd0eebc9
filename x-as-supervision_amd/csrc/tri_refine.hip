// Refinement of triangulated joints on the device (gfx950): Levenberg-Marquardt on the weighted reprojection error in pixels,
// from the DLT or robust point of triangulate.hip.  The two kernels share multiview.h's solver layer: the observations, the fit of
// a point, the pass-through rule, the LM schedule.  Their loops differ in what is uniform over the wave and where the barriers
// sit, so each keeps its own.
//   triangulate_refine : per joint, thread per (b, joint) (no reference counterpart: eval.py --tri-refine lm)
//   triangulate_skeleton : the joints of a sample coupled by left/right limb symmetry, one wave per sample (eval.py --tri-skeleton)
#include "multiview.h"

namespace xas {

// triangulate_refine: Levenberg-Marquardt on the weighted reprojection error from the DLT / robust result, thread per
// (b, joint) as triangulate_kernel.  A few hundred joints of 3x3 algebra in double: latency-bound, no throughput to win.
// A thread keeps its V points (u, v, scale) in registers and re-reads the sample's projection matrices at every
// linearisation: at most 72 floats that all threads of a sample share, so they stay in the caches, where holding them
// would cost every thread 72 more registers.
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
  ViewObs obs;
  load_obs(pts, b, V, K, k, flags, obs);
  const int used = views_used(obs.valid, views ? views[i] : 0);
  const int nused = __popc(used);
  const double huber = (double)huber_;

  const float* in = init + (size_t)i * 4;
  const float x0 = in[0], x1 = in[1], x2 = in[2];
  double X[3] = {(double)x0, (double)x1, (double)x2};
  PointFit fit;
  const bool solve = point_startable(nused, X) && point_fit(Pb, obs, used, huber, X, fit);   // multiview.h's pass-through rule
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
  double lambda = kLmLambda0;
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
    PointFit trial;
    const bool front = point_fit(Pb, obs, used, huber, Xt, trial);
    if (front && trial.C < fit.C) {                                   // NaN never passes
      X[0] = Xt[0]; X[1] = Xt[1]; X[2] = Xt[2];
      fit = trial;
      lambda *= kLmAccept;
      if (sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < kLmStepTol) { st = 0; break; }
    } else {
      lambda *= kLmReject;
      if (lambda > kLmLambdaMax) break;
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

// The residual terms of the joints in `mask` at X[src], then each joint's sums on its own lane: cost, |r|^2 and whether it lies
// in front of every view it uses.  Starts with a barrier (X[src] was just written, `term` may still be read) and ends past one.
__device__ __forceinline__ void sk_reproj(SkShared& s, int src, int V, int K, unsigned mask, double huber, int lane, double& Ck,
                                          double& r2k, bool& frontk) {
  __syncthreads();
  for (int t = lane; t < K * V; t += 64) {
    const int k = t / V, v = t - k * V;
    if (!((mask >> k) & 1) || !((s.used[k] >> v) & 1)) continue;
    const double Xh[4] = {s.X[src][k][0], s.X[src][k][1], s.X[src][k][2], 1.0};
    const ReprojTerm r = reproj_term(s.P[v], Xh, (double)s.pu[k][v], (double)s.pv[k][v], (double)s.ps[k][v], huber);
    double* o = s.term[k][v];
    o[0] = huber_cost(r, huber);
    o[1] = r.rr;
#pragma unroll
    for (int n = 0; n < 3; ++n) o[8 + n] = r.w * r.grad(n);
    reproj_block(r, o + 2);
    o[11] = r.front ? 1.0 : 0.0;
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
        if (bi > bj || c <= r) s.H[tri_idx(3 * bi + r, 3 * bj + c)] = h[r][c];
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
      double a = s.H[tri_idx(i, j)];
      if (i == j) a *= 1.0 + lambda;
      for (int k = fi > fj ? fi : fj; k < j; ++k) a -= s.Lm[tri_idx(i, k)] * s.Lm[tri_idx(j, k)];
      v[h] = a;
    }
    const double d = j < 64 ? __shfl(v[0], j, 64) : __shfl(v[1], j - 64, 64);
    if (!(d > 0.0)) return false;                                     // the same d on every lane; NaN fails too
    const double sd = sqrt(d);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < j || i >= n) continue;
      s.Lm[tri_idx(i, j)] = i == j ? sd : v[h] / sd;
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
  auto below = [&](int i, int j) { return i > j && i < n ? s.Lm[tri_idx(i, j)] : 0.0; };   // L_ij, column j
  auto left = [&](int i, int j) { return i < j ? s.Lm[tri_idx(j, i)] : 0.0; };             // L_ji, row j
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
  // lane = joint: its points, the views it uses and its start
  const size_t i = (size_t)b * K + (lane < K ? lane : 0);
  float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
  int nused = 0;
  bool cand = false;
  if (lane < K) {
    int valid = 0;
    for (int v = 0; v < V; ++v) {                                     // load_obs's per-view body, staged to LDS
      const float* q = pts + (((size_t)b * V + v) * K + lane) * 3;
      s.pu[lane][v] = q[0]; s.pv[lane][v] = q[1];
      s.ps[lane][v] = (flags & XAS_REFINE_WEIGHTED) ? q[2] : 1.f;
      valid |= view_valid(q[2]) ? 1 << v : 0;
    }
    const int used = views_used(valid, views ? views[i] : 0);
    s.used[lane] = used;
    nused = __popc(used);
    const float* in = init + i * 4;
    x0 = in[0]; x1 = in[1]; x2 = in[2]; x3 = in[3];
    s.X[0][lane][0] = (double)x0; s.X[0][lane][1] = (double)x1; s.X[0][lane][2] = (double)x2;
    cand = nused >= 2 && fabsf(x0) < INFINITY && fabsf(x1) < INFINITY && fabsf(x2) < INFINITY;   // point_startable, on the floats
  }
  const unsigned candmask = (unsigned)__ballot(cand);
  double Ck, r2k;
  bool frontk;
  sk_reproj(s, 0, V, K, candmask, huber, lane, Ck, r2k, frontk);      // its first barrier publishes the staging above
  const bool isfree = cand && frontk;                                 // FREE by multiview.h's pass-through rule
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
    double lambda = kLmLambda0;
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
        lambda *= kLmAccept;
        if (big < kLmStepTol) { st = 0; break; }
        sk_assemble(s, cur, V, nfree, L, active, sym_w, lane);
      } else {
        lambda *= kLmReject;
        if (lambda > kLmLambdaMax) break;
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

}  // namespace xas

using namespace xas;

extern "C" int xas_triangulate_refine(const float* points, const float* P, const float* init, const unsigned char* views,
                                      int B, int V, int K, int flags, float huber, int max_iter, float* out, float* resid,
                                      float* cov, unsigned char* status, void* stream) {
  XAS_REQUIRE(points && P && init && out, "triangulate_refine: null buffer (points, P, init and out are required)");
  if (tri_check_views("triangulate_refine", V, 2) || tri_check_shape("triangulate_refine", B, K, "B > 0, K >= 1")) return 1;
  if (tri_check_lm("triangulate_refine", max_iter, flags)) return 1;
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
  if (tri_check_views("triangulate_skeleton", V, 2)) return 1;
  XAS_REQUIRE(K >= 3 && K <= XAS_SKEL_MAX_JOINTS, "triangulate_skeleton: K=%d joints (needs 3 <= K <= XAS_SKEL_MAX_JOINTS = %d)", K,
              XAS_SKEL_MAX_JOINTS);
  XAS_REQUIRE(L >= 0 && L <= XAS_SKEL_MAX_LIMBS, "triangulate_skeleton: L=%d limb pairs (needs 0 <= L <= XAS_SKEL_MAX_LIMBS = %d)", L,
              XAS_SKEL_MAX_LIMBS);
  if (tri_check_shape("triangulate_skeleton", B, K, "B > 0") || tri_check_lm("triangulate_skeleton", max_iter, flags)) return 1;
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
