// The data term of a frame with a 3-D anchor, and the checks of the anchor arguments: what track_anchor.hip and
// track_skeleton.hip share; anchor_load, anchor_term and ta_check serve smplfit_views.hip too.  include/xas_hip.h states the rules (xas_track_anchor_smooth); track_band.h has the
// reprojection term this one takes as it is.  Device-inline and host-inline only: nothing here is a symbol.
#pragma once
#include "track_band.h"

namespace xas {

// Anchor i of anchor [..][3] and info [..][6] (xx xy xz yy yz zz) in double -> it is USABLE: both arrays given, nine finite
// numbers, no negative diagonal entry of W, trace W > 0.  The one rule of the smoothers and of smplfit_views.hip.
__device__ __forceinline__ bool anchor_load(const float* anchor, const float* info, size_t i, double (&A)[3], double (&W)[6]) {
  if (!anchor) return false;
  bool finite = true;
#pragma unroll
  for (int m = 0; m < 3; ++m) { A[m] = (double)anchor[i * 3 + m]; finite = finite && fabs(A[m]) < INFINITY; }
#pragma unroll
  for (int m = 0; m < 6; ++m) { W[m] = (double)info[i * 6 + m]; finite = finite && fabs(W[m]) < INFINITY; }
  return finite && W[0] >= 0.0 && W[3] >= 0.0 && W[5] >= 0.0 && W[0] + W[3] + W[5] > 0.0;
}

// The anchor term at X, added to f: rho_a(m), m = sqrt(e^T W e), e = X - A: with psi = 1 on the quadratic part and huber / m
// on the linear one (multiview.h's IRLS weight), block psi W and gradient psi W e.  e^T W e is clamped at 0: a rank-deficient
// W rounded to fp32 may be indefinite in its last bit.
__device__ __forceinline__ void anchor_term(const double (&A)[3], const double (&W)[6], double huber, const double (&X)[3], PointFit& f) {
  const double e[3] = {X[0] - A[0], X[1] - A[1], X[2] - A[2]};
  const double We[3] = {W[0] * e[0] + W[1] * e[1] + W[2] * e[2], W[1] * e[0] + W[3] * e[1] + W[4] * e[2],
                        W[2] * e[0] + W[4] * e[1] + W[5] * e[2]};
  const double m = sqrt(fmax(e[0] * We[0] + e[1] * We[1] + e[2] * We[2], 0.0));
  const bool tail = huber > 0.0 && m > huber;
  const double psi = tail ? huber / m : 1.0;
  f.C += tail ? 2.0 * huber * m - huber * huber : m * m;
#pragma unroll
  for (int c = 0; c < 6; ++c) f.H[c] += psi * W[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) f.g[c] += psi * We[c];
}

struct TsAnchored {
  const float *anchor, *info;                                         // [N][K][3] and [N][K][6] (xx xy xz yy yz zz), or both NULL
  double huber;                                                       // the anchor term's Huber delta; 0 = squared

  // The frame's anchor in double -> it is USABLE (anchor_load's rule).
  __device__ __forceinline__ bool load(size_t i, double (&A)[3], double (&W)[6]) const { return anchor_load(anchor, info, i, A, W); }

  // Without a usable anchor the frame is TsReproj's.  With one it is a data frame whatever else holds: it starts at init's
  // point if that is finite, else at the anchor, and its reprojection term runs over the views xas_triangulate_refine would
  // use, however few, unless the start lies behind one of them: then the anchor term stands alone.
  __device__ __forceinline__ int classify(const TsArgs& a, int n, int k, double (&X)[3]) const {
    const size_t i = (size_t)n * a.K + k;
    double A[3], W[6];
    if (!load(i, A, W)) return TsReproj().classify(a, n, k, X);
    const float* in = a.init + i * 4;
    X[0] = (double)in[0]; X[1] = (double)in[1]; X[2] = (double)in[2];
    if (!(fabs(X[0]) < INFINITY && fabs(X[1]) < INFINITY && fabs(X[2]) < INFINITY)) { X[0] = A[0]; X[1] = A[1]; X[2] = A[2]; }
    ViewObs ob;
    load_obs(a.pts, n, a.V, a.K, k, a.flags, ob);
    int used = views_used(ob.valid, a.views ? a.views[i] : 0);
    PointFit f;
    if (used && !point_fit(a.P + (size_t)n * a.V * 12, ob, used, a.huber, X, f)) used = 0;
    return used | kTsAnchored;
  }

  // The reprojection term over the views used, then anchor_term.
  __device__ __forceinline__ bool fit(const TsArgs& a, int n, int k, int used, const double (&X)[3], PointFit& f) const {
    const bool front = TsReproj().fit(a, n, k, used, X, f);
    if (used & kTsAnchored) {
      const size_t i = (size_t)n * a.K + k;
      double A[3], W[6];
      load(i, A, W);
      anchor_term(A, W, huber, X, f);
    }
    return front;
  }
};

// The checks of the anchor arguments, before anything is launched.
static inline int ta_check(const char* who, const float* anchor, const float* info, double anchor_huber) {
  XAS_REQUIRE((anchor != nullptr) == (info != nullptr), "%s: anchor and info come together (both given, or both NULL)", who);
  XAS_REQUIRE(anchor_huber >= 0.0 && anchor_huber < INFINITY, "%s: anchor_huber %f (needs a finite anchor_huber >= 0)", who,
              anchor_huber);
  return 0;
}

}  // namespace xas
