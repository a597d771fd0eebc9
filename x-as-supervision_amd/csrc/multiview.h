// What evalpath.hip, triangulate.hip, tri_refine.hip and tri_volume.hip share, each piece in its one copy: double reductions over
// a wave, the 4x4 eigenproblem, the projection of a point, which views count, the reprojection term, the Levenberg-Marquardt
// schedule and the entry points' argument checks.  Device-inline and host-inline only: nothing here is a symbol.
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
// The callers form their own cost from rr, e and tail: s^2 rr and e e are not the same number in the last bit.
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
static inline int tri_check_lm(const char* who, int max_iter, int flags) {
  XAS_REQUIRE(max_iter >= 1 && max_iter <= 64, "%s: max_iter=%d trials (needs 1 <= max_iter <= 64)", who, max_iter);
  XAS_REQUIRE((flags & ~XAS_REFINE_WEIGHTED) == 0, "%s: unknown flag bits 0x%x (XAS_REFINE_WEIGHTED = %d is the only flag)", who,
              flags & ~XAS_REFINE_WEIGHTED, XAS_REFINE_WEIGHTED);
  return 0;
}

}  // namespace xas
