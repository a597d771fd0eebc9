// What the multi-view files share, each piece in its one copy.  Device-inline and host-inline only: nothing here is a symbol.
//   evalpath.hip, triangulate.hip, tri_volume.hip: the double reductions over a wave, the 4x4 eigenproblem, the projection of a
//       point, which views count, the argument checks.
//   tri_refine.hip, calibrate.hip, track_smooth.hip, the four Levenberg-Marquardt solvers over (points, P, init, views): those
//       and the solver layer below them.  ViewObs / load_obs: a joint's observations in registers.  ReprojTerm / reproj_term /
//       reproj_block / huber_cost: one view's term.  PointFit / fit_views / point_fit: cost, |r|^2, H and g of a point over the
//       views used.  point_startable and THE PASS-THROUGH RULE next to it: which points a solver refines.  chol3 / lsolve3 /
//       ltsolve3 / sym3_inverse / tri_idx: the 3x3 algebra and the packed triangle.  kLm*: the schedule.  tri_check_*: the checks.
#pragma once
#include "common.h"

namespace xas {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double lane0(double v) { return __shfl(v, 0, 64); }

// Small symmetric eigenproblems (4x4) are solved with cyclic Jacobi rotations in double precision, fully unrolled
// so that the matrices live in registers: the DLT null vector is the eigenvector of A^T A with the smallest
// eigenvalue, and the Procrustes rotation is Horn's unit quaternion, the eigenvector of a 4x4 matrix built from
// the 3x3 correlation with the LARGEST eigenvalue (always a proper rotation: the same matrix as the reference's
// SVD solution with its det(R) = +1 fix, metrics.py:41-49).
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

// The smallest (or `largest`) eigenvalue on the diagonal that jacobi4 left, the first of equals -> its index, val = its value.
__device__ __forceinline__ int jacobi4_pick(const double (&a)[4][4], bool largest, double& val) {
  int best = 0;
  val = a[0][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (largest ? a[j][j] > val : a[j][j] < val) { val = a[j][j]; best = j; }
  return best;
}

// x = column n of v (an eigenvector), picked without indexing the registers at run time.
__device__ __forceinline__ void jacobi4_column(const double (&v)[4][4], int n, double (&x)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) x[r] = n == 0 ? v[r][0] : (n == 1 ? v[r][1] : (n == 2 ? v[r][2] : v[r][3]));
}

// h = P X of homogeneous X in one view, in double from the fp32 entries; false if X lies behind the camera (or on its
// principal plane).  The one projection, and the one meaning of "behind", of everything that reprojects in these files.
__device__ __forceinline__ bool project_view(const float* __restrict__ Pm, const double (&X)[4], double (&h)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
    h[r] = (double)Pm[4 * r] * X[0] + (double)Pm[4 * r + 1] * X[1] + (double)Pm[4 * r + 2] * X[2] + (double)Pm[4 * r + 3] * X[3];
  return !(h[2] / X[3] <= 0.0);
}

// A view of a joint is valid if its weight is finite and positive.
__device__ __forceinline__ bool view_valid(float w) { return w > 0.f && w < INFINITY; }

// The views a refinement uses, from the mask of the valid ones and the joint's `views` byte: the byte's views among the valid
// ones; a zero byte (none given, or the robust kernel's "no consensus") stands for all valid views.
__device__ __forceinline__ int views_used(int valid, int sel) { return sel ? (valid & sel) : valid; }

// One view's reprojection term at the homogeneous point X, against the observed pixel (u, v) with scale s:
//   (ru, rv) the residual in pixels, rr = |r|^2, e = s |r|, tail = e lies on the linear part of the Huber loss (huber > 0),
//   w = the IRLS weight (huber / e on the tail, else 1) times s^2, ju / jv = d(u, v) / dX, front = project_view's answer.
// huber_cost forms the cost from e and tail: s^2 rr and e e are not the same number in the last bit.
struct ReprojTerm {
  double ru, rv, rr, e, w, ju[3], jv[3];
  bool tail, front;
  __device__ __forceinline__ double grad(int n) const { return ju[n] * ru + jv[n] * rv; }   // d(rr / 2) / dX[n]
};

__device__ __forceinline__ ReprojTerm reproj_term(const float* __restrict__ Pm, const double (&X)[4], double u, double v, double s, double huber) {
  ReprojTerm t;
  double h[3];
  t.front = project_view(Pm, X, h);
  const double pu = h[0] / h[2], pv = h[1] / h[2];
  t.ru = pu - u; t.rv = pv - v;
  t.rr = t.ru * t.ru + t.rv * t.rv;
  t.e = s * sqrt(t.rr);
  t.tail = huber > 0.0 && t.e > huber;
  t.w = (t.tail ? huber / t.e : 1.0) * s * s;
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    t.ju[n] = ((double)Pm[n] - pu * (double)Pm[8 + n]) / h[2];
    t.jv[n] = ((double)Pm[4 + n] - pv * (double)Pm[8 + n]) / h[2];
  }
  return t;
}

// The term's 3x3 Gauss-Newton block w (ju ju^T + jv jv^T), upper triangle 00 01 02 11 12 22.
__device__ __forceinline__ void reproj_block(const ReprojTerm& t, double* blk) {
  int n = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = r; c < 3; ++c) blk[n++] = t.w * (t.ju[r] * t.ju[c] + t.jv[r] * t.jv[c]);
}

// The term's Huber cost (huber > 0; else its square): e^2 on the quadratic part, 2 huber e - huber^2 on the linear one.
__device__ __forceinline__ double huber_cost(const ReprojTerm& t, double huber) {
  return t.tail ? 2.0 * huber * t.e - huber * huber : t.e * t.e;
}

// A joint's observations (u, v, scale) in registers and the mask of its valid views.  Every loop over the views is unrolled to
// XAS_TRI_MAX_VIEWS and predicated, so no array is indexed at run time; entries at v >= V are zero and never read.
struct ViewObs {
  float pu[XAS_TRI_MAX_VIEWS], pv[XAS_TRI_MAX_VIEWS], ps[XAS_TRI_MAX_VIEWS];
  int valid;
};

// Joint k of sample n of pts [N][V][K][3].  The scale is the weight under XAS_REFINE_WEIGHTED, else 1.
__device__ __forceinline__ void load_obs(const float* pts, int n, int V, int K, int k, int flags, ViewObs& o) {
  o.valid = 0;
#pragma unroll
  for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v) {
    o.pu[v] = 0.f; o.pv[v] = 0.f; o.ps[v] = 0.f;
    if (v < V) {
      const float* q = pts + (((size_t)n * V + v) * K + k) * 3;
      o.pu[v] = q[0]; o.pv[v] = q[1];
      o.ps[v] = (flags & XAS_REFINE_WEIGHTED) ? q[2] : 1.f;
      o.valid |= view_valid(q[2]) ? 1 << v : 0;
    }
  }
}

// The problem at one point: cost C, sum of the squared unweighted pixel residuals r2, Gauss-Newton Hessian H (upper triangle
// 00 01 02 11 12 22) and gradient g with the IRLS weights of the point itself.
struct PointFit {
  double C, r2, H[6], g[3];
  __device__ __forceinline__ void clear() {
    C = 0.0; r2 = 0.0;
#pragma unroll
    for (int n = 0; n < 6; ++n) H[n] = 0.0;
#pragma unroll
    for (int n = 0; n < 3; ++n) g[n] = 0.0;
  }
};

// f = the sum over the views in `used`, in ascending view order, of the terms that term(v) forms -> every one of them lies in
// front of its camera.  What a caller does not read of f is never computed: all of this is inlined into it.
template <class Term>
__device__ __forceinline__ bool fit_views(int used, double huber, Term term, PointFit& f) {
  f.clear();
  bool front = true;
#pragma unroll
  for (int v = 0; v < XAS_TRI_MAX_VIEWS; ++v) {
    if (!((used >> v) & 1)) continue;
    const ReprojTerm t = term(v);
    front = t.front && front;
    f.r2 += t.rr;
    f.C += huber_cost(t, huber);
    double blk[6];
    reproj_block(t, blk);
#pragma unroll
    for (int n = 0; n < 3; ++n) f.g[n] += t.w * t.grad(n);
#pragma unroll
    for (int n = 0; n < 6; ++n) f.H[n] += blk[n];
  }
  return front;
}

// The fit at the point X of a sample whose projection matrices are Pb [V][12]; false if X lies behind a view used.
__device__ __forceinline__ bool point_fit(const float* __restrict__ Pb, const ViewObs& o, int used, double huber, const double (&X)[3],
                                          PointFit& f) {
  const double Xh[4] = {X[0], X[1], X[2], 1.0};
  return fit_views(used, huber, [&](int v) { return reproj_term(Pb + v * 12, Xh, (double)o.pu[v], (double)o.pv[v], (double)o.ps[v], huber); }, f);
}

// THE PASS-THROUGH RULE of the four solvers.  A point is FREE, that is refined, if it uses at least two views
// (views_used), starts at a finite X, and that start lies in front of every view it uses (what the fit at the start
// answers).  Every other point is PASSED THROUGH: it comes back as its init bit for bit, NaN payload included, and takes no
// part in the problem.  point_startable is the part of the rule that needs no fit; the fit is formed only where it holds.
__device__ __forceinline__ bool point_startable(int nused, const double (&X)[3]) {
  return nused >= 2 && fabs(X[0]) < INFINITY && fabs(X[1]) < INFINITY && fabs(X[2]) < INFINITY;
}

// Inverse of the symmetric 3x3 a (upper triangle 00 01 02 11 12 22) by its adjugate.  A singular a gives inf / NaN.
__device__ __forceinline__ void sym3_inverse(const double (&a)[6], double (&inv)[6]) {
  const double c00 = a[3] * a[5] - a[4] * a[4], c01 = a[2] * a[4] - a[1] * a[5], c02 = a[1] * a[4] - a[2] * a[3];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  inv[0] = c00 / det; inv[1] = c01 / det; inv[2] = c02 / det;
  inv[3] = (a[0] * a[5] - a[2] * a[2]) / det;
  inv[4] = (a[1] * a[2] - a[0] * a[4]) / det;
  inv[5] = (a[0] * a[3] - a[1] * a[1]) / det;
}

// Cholesky of the symmetric 3x3 A (upper triangle 00 01 02 11 12 22): L (lower, 00 10 11 20 21 22) L^T = A -> every pivot was
// positive.  A pivot that is not leaves NaN in L, which no later comparison passes.
__device__ __forceinline__ bool chol3(const double (&A)[6], double (&L)[6]) {
  L[0] = sqrt(A[0]);
  L[1] = A[1] / L[0];
  const double d1 = A[3] - L[1] * L[1];
  L[2] = sqrt(d1);
  L[3] = A[2] / L[0];
  L[4] = (A[4] - L[3] * L[1]) / L[2];
  const double d2 = A[5] - L[3] * L[3] - L[4] * L[4];
  L[5] = sqrt(d2);
  return A[0] > 0.0 && d1 > 0.0 && d2 > 0.0;
}
// x = L^-1 b and x = L^-T b of that L.
__device__ __forceinline__ void lsolve3(const double (&L)[6], const double (&b)[3], double (&x)[3]) {
  x[0] = b[0] / L[0];
  x[1] = (b[1] - L[1] * x[0]) / L[2];
  x[2] = (b[2] - L[3] * x[0] - L[4] * x[1]) / L[5];
}
__device__ __forceinline__ void ltsolve3(const double (&L)[6], const double (&b)[3], double (&x)[3]) {
  x[2] = b[2] / L[5];
  x[1] = (b[1] - L[4] * x[2]) / L[2];
  x[0] = (b[0] - L[1] * x[1] - L[3] * x[2]) / L[0];
}

// Entry (i, j), j <= i, of a lower triangle packed row by row.
__host__ __device__ __forceinline__ int tri_idx(int i, int j) { return i * (i + 1) / 2 + j; }

// Levenberg-Marquardt schedule: lambda starts at kLmLambda0, times kLmAccept after an accepted trial, times kLmReject after a
// rejected one; an accepted step shorter than kLmStepTol (mm) is convergence, a lambda above kLmLambdaMax gives up.
constexpr double kLmLambda0 = 1e-3, kLmAccept = 0.1, kLmReject = 10.0, kLmLambdaMax = 1e12, kLmStepTol = 1e-5;

// The argument checks that the entry points share, in pieces because each entry point has checks of its own between them and
// reports the first that fails.  `who` names the entry point, `rule` is how it words its bounds on B and K.  0 = passed.
static inline int tri_check_views(const char* who, int V, int vmin) {
  XAS_REQUIRE(V >= vmin && V <= XAS_TRI_MAX_VIEWS, "%s: V=%d views (needs %d <= V <= XAS_TRI_MAX_VIEWS = %d)", who, V, vmin, XAS_TRI_MAX_VIEWS);
  return 0;
}
static inline int tri_check_shape(const char* who, int B, int K, const char* rule) {
  XAS_REQUIRE(B > 0 && K > 0 && (long)B * K <= 0x7fffffffL, "%s: bad shape B=%d K=%d (%s, B*K < 2^31)", who, B, K, rule);
  return 0;
}
static inline int tri_check_iter(const char* who, int max_iter) {
  XAS_REQUIRE(max_iter >= 1 && max_iter <= 64, "%s: max_iter=%d trials (needs 1 <= max_iter <= 64)", who, max_iter);
  return 0;
}
static inline int tri_check_flags(const char* who, int flags) {
  XAS_REQUIRE((flags & ~XAS_REFINE_WEIGHTED) == 0, "%s: unknown flag bits 0x%x (XAS_REFINE_WEIGHTED = %d is the only flag)", who,
              flags & ~XAS_REFINE_WEIGHTED, XAS_REFINE_WEIGHTED);
  return 0;
}
static inline int tri_check_lm(const char* who, int max_iter, int flags) {
  return tri_check_iter(who, max_iter) || tri_check_flags(who, flags);
}

}  // namespace xas
