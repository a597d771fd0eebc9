// What the two smoothers over tracks share (track_smooth.hip, track_anchor.hip), each piece in its one copy: the record of a
// wave, the acceleration prior's stencil and matrix, the gap-start rule, the cost / gradient / block pass, the block-
// pentadiagonal factorisation with its two substitutions, the Levenberg-Marquardt loop with every output, and the host's checks.
// include/xas_hip.h states the problem; this file is its schedule.  Device-inline and host-inline only: nothing here is a symbol.
// What differs between the two files is the DATA TERM of a frame, a class each of them passes to ts_run:
//   int  classify(a, n, k, X)         the start X of joint k of sample n and the frame's USED word: 0 = a gap frame, else the mask
//                                     of the views its reprojection term uses, and kTsAnchored if it has a 3-D anchor term
//   bool fit(a, n, k, used, X, f)     f = cost, |r|^2, block and gradient of the frame's data at X -> X lies behind no view used
// One wave per (track, joint), one launch.  Its state lives in the caller's workspace, T * kTsRec doubles per wave:
//   X [2][T][3]   the current point and the trial point; accepting a trial swaps the index, nothing is copied
//   D [2][T][6]   the frame's 3x3 Gauss-Newton block of the data (multiview.h's reproj_block, summed over the views used)
//   G [2][T][3]   the frame's gradient, data and prior
//   R2 [2][T]     the frame's sum of squared pixel residuals
//   A [T][3]      row t of the prior's pentadiagonal matrix: A_tt, A_t,t-1, A_t,t-2 (of `frame` alone, formed once)
//   L [T][24]     the Cholesky factor's block row t: L_tt (lower, 00 10 11 20 21 22), L_t,t-1 and L_t,t-2 (3x3, row-major)
//   DX [T][3]     the forward-substituted right-hand side, then the step
//   USED [T]      the frame's USED word, 0 for a GAP frame
// Division of labour.  Lanes stride the frames where frames are independent: the classification, the gap fill, the cost, the
// gradient, the data blocks, the trial point, the outputs.  Every sum over frames is a lane's partial sum in ascending frame
// order, then wave_sum_d: one order, no atomics.  The factorisation and the two substitutions are recurrences over t with the
// two previous block rows in registers; every lane runs them on the same values (nothing to broadcast, no divergence), lane 0
// stores.  Their operands are loaded one frame ahead of their use: the recurrence would otherwise wait a cache latency per frame.
// Every value a branch depends on is the same on all lanes, so the wave never diverges round a barrier.
#pragma once
#include <math.h>

#include "multiview.h"
#include "track_start.h"
#include "track_stencil.h"                                            // TsStencil, ts_stencil

namespace xas {

// offsets of the arrays of a wave's record, in units of T doubles
constexpr int kTsX = 0, kTsD = 6, kTsG = 18, kTsR2 = 24, kTsA = 26, kTsL = 29, kTsDX = 53, kTsUsed = 56, kTsRec = 57;
// the USED word: the views of the reprojection term in its low bits, and whether the frame has an anchor term
constexpr int kTsViews = (1 << XAS_TRI_MAX_VIEWS) - 1, kTsAnchored = 1 << 30;
enum { TS_SMOOTH, TS_LINEARISE };

struct TsArgs {
  const float *pts, *P, *init;
  const unsigned char* views;
  const int *frame, *start;                                           // start: the workspace's copy of the host array
  double* ws;
  int N, V, K, S, flags, max_iter;
  double huber, acc_w;
};
struct TsOut {
  float *out, *resid;                                                 // smooth
  unsigned char *status, *track_status;
  double* cost;
  int* trials;
  double *band, *g, *C, lambda;                                       // linearise
};

// The reprojection term of a frame, xas_triangulate_refine's: the whole data term of track_smooth.hip, and the part of
// track_anchor.hip's that it takes as it is.  classify is multiview.h's pass-through rule: a frame with data is a free point.
struct TsReproj {
  __device__ __forceinline__ int classify(const TsArgs& a, int n, int k, double (&X)[3]) const {
    const size_t i = (size_t)n * a.K + k;
    ViewObs ob;
    load_obs(a.pts, n, a.V, a.K, k, a.flags, ob);
    const int used = views_used(ob.valid, a.views ? a.views[i] : 0);
    const float* in = a.init + i * 4;
    X[0] = (double)in[0]; X[1] = (double)in[1]; X[2] = (double)in[2];
    PointFit f;
    const bool data = point_startable(__popc(used), X) && point_fit(a.P + (size_t)n * a.V * 12, ob, used, a.huber, X, f);
    return data ? used : 0;
  }
  __device__ __forceinline__ bool fit(const TsArgs& a, int n, int k, int used, const double (&X)[3], PointFit& f) const {
    ViewObs o;
    load_obs(a.pts, n, a.V, a.K, k, a.flags, o);
    return point_fit(a.P + (size_t)n * a.V * 12, o, used & kTsViews, a.huber, X, f);
  }
};

// RMS of the pixel residuals over the views a frame uses; NaN where it uses none.
__device__ __forceinline__ float ts_rms(double r2, int used) {
  const int nv = __popc(used & kTsViews);
  return nv ? (float)sqrt(r2 / (double)nv) : NAN;
}

// Cost, data blocks and gradients of every frame at X[src] -> D[src], G[src], R2[src]; C = the track's cost, bad = a data frame
// lies behind a view it uses.  Starts with a barrier (X[src] was just written) and ends past one.
template <class Data>
__device__ __forceinline__ void ts_eval(const TsArgs& a, const Data& data, double* w, const int* __restrict__ fr, int n0, int T,
                                        int k, int src, int lane, double& C, bool& bad) {
  __syncthreads();
  const double* X = w + (size_t)(kTsX + 3 * src) * T;
  double* D = w + (size_t)(kTsD + 6 * src) * T;
  double* G = w + (size_t)(kTsG + 3 * src) * T;
  double* R2 = w + (size_t)(kTsR2 + src) * T;
  const int* usedw = (const int*)(w + (size_t)kTsUsed * T);
  double Cd = 0.0, Cp = 0.0;
  int behind = 0;
  for (int t = lane; t < T; t += 64) {
    double gp[3] = {0.0, 0.0, 0.0}, cp = 0.0;
    for (int s = t - 1; s <= t + 1; ++s) {
      if (s < 1 || s > T - 2) continue;
      const TsStencil c = ts_stencil(fr, s);
      const double ct = c.at(s, t);
      double qq = 0.0;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const double xm = X[3 * (s - 1) + m], x0 = X[3 * s + m], xp = X[3 * (s + 1) + m];
        const double q = c.cp * (xp - x0) - c.cm * (x0 - xm);
        gp[m] += c.ws * ct * q;
        qq += q * q;
      }
      if (s == t) cp = c.ws * qq;
    }
    const int used = usedw[t];
    PointFit f;
    f.clear();                                                        // a gap frame: no data
    if (used) {
      const double Xt[3] = {X[3 * t], X[3 * t + 1], X[3 * t + 2]};
      if (!data.fit(a, n0 + t, k, used, Xt, f)) behind = 1;
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) D[6 * t + m] = f.H[m];
#pragma unroll
    for (int m = 0; m < 3; ++m) G[3 * t + m] = f.g[m] + a.acc_w * gp[m];
    R2[t] = f.r2;
    Cd += f.C; Cp += cp;
  }
  C = lane0(wave_sum_d(Cd)) + a.acc_w * lane0(wave_sum_d(Cp));
  bad = __any(behind) != 0;
  __syncthreads();
}

// Block-pentadiagonal Cholesky of H + lambda diag H (half-bandwidth 8 in scalar terms), H_tt = D_t + acc_w A_tt I,
// H_t,t-1 = acc_w A_t,t-1 I, H_t,t-2 = acc_w A_t,t-2 I, with the forward substitution L y = -g in the same sweep.
// false at a pivot that is not > 0 (NaN fails too); the same on every lane.
static __device__ bool ts_factor(double* w, int T, int cur, double lambda, double acc_w, int lane) {
  const double* D = w + (size_t)(kTsD + 6 * cur) * T;
  const double* G = w + (size_t)(kTsG + 3 * cur) * T;
  const double* A = w + (size_t)kTsA * T;
  double* L = w + (size_t)kTsL * T;
  double* Y = w + (size_t)kTsDX * T;
  double p1[6] = {1.0, 0.0, 1.0, 0.0, 0.0, 1.0}, p2[6] = {1.0, 0.0, 1.0, 0.0, 0.0, 1.0};   // L_t-1,t-1 and L_t-2,t-2
  double q1[9], y1[3] = {0.0, 0.0, 0.0}, y2[3] = {0.0, 0.0, 0.0};                          // L_t-1,t-2; y_t-1, y_t-2
#pragma unroll
  for (int m = 0; m < 9; ++m) q1[m] = 0.0;
  double nd[6], ng[3], na[3];
#pragma unroll
  for (int m = 0; m < 6; ++m) nd[m] = D[m];
#pragma unroll
  for (int m = 0; m < 3; ++m) { ng[m] = G[m]; na[m] = A[m]; }
  for (int t = 0; t < T; ++t) {
    double d[6], g[3], al[3];
#pragma unroll
    for (int m = 0; m < 6; ++m) d[m] = nd[m];
#pragma unroll
    for (int m = 0; m < 3; ++m) { g[m] = ng[m]; al[m] = na[m]; }
    const int tn = t + 1 < T ? t + 1 : t;                             // the next frame's operands, ahead of their use
#pragma unroll
    for (int m = 0; m < 6; ++m) nd[m] = D[6 * tn + m];
#pragma unroll
    for (int m = 0; m < 3; ++m) { ng[m] = G[3 * tn + m]; na[m] = A[3 * tn + m]; }
    const double b0 = acc_w * al[0], b1 = acc_w * al[1], b2 = acc_w * al[2];
    double l2[9], l1[9];                                              // L_t,t-2 = H_t,t-2 L_t-2,t-2^-T, row by row
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double row[3] = {r == 0 ? b2 : 0.0, r == 1 ? b2 : 0.0, r == 2 ? b2 : 0.0};
      double x[3];
      lsolve3(p2, row, x);
      l2[3 * r] = x[0]; l2[3 * r + 1] = x[1]; l2[3 * r + 2] = x[2];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {                                     // L_t,t-1 = (H_t,t-1 - L_t,t-2 L_t-1,t-2^T) L_t-1,t-1^-T
      double row[3];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        row[c] = (r == c ? b1 : 0.0) - (l2[3 * r] * q1[3 * c] + l2[3 * r + 1] * q1[3 * c + 1] + l2[3 * r + 2] * q1[3 * c + 2]);
      double x[3];
      lsolve3(p1, row, x);
      l1[3 * r] = x[0]; l1[3 * r + 1] = x[1]; l1[3 * r + 2] = x[2];
    }
    auto dot = [&](int r, int c) {
      return l2[3 * r] * l2[3 * c] + l2[3 * r + 1] * l2[3 * c + 1] + l2[3 * r + 2] * l2[3 * c + 2] + l1[3 * r] * l1[3 * c] +
             l1[3 * r + 1] * l1[3 * c + 1] + l1[3 * r + 2] * l1[3 * c + 2];
    };
    const double m00 = (d[0] + b0) * (1.0 + lambda) - dot(0, 0), m10 = d[1] - dot(1, 0), m11 = (d[3] + b0) * (1.0 + lambda) - dot(1, 1);
    const double m20 = d[2] - dot(2, 0), m21 = d[4] - dot(2, 1), m22 = (d[5] + b0) * (1.0 + lambda) - dot(2, 2);
    double l0[6];                                                     // chol3's factor, with a test at every pivot
    if (!(m00 > 0.0)) return false;
    l0[0] = sqrt(m00);
    l0[1] = m10 / l0[0];
    const double v11 = m11 - l0[1] * l0[1];
    if (!(v11 > 0.0)) return false;
    l0[2] = sqrt(v11);
    l0[3] = m20 / l0[0];
    l0[4] = (m21 - l0[3] * l0[1]) / l0[2];
    const double v22 = m22 - l0[3] * l0[3] - l0[4] * l0[4];
    if (!(v22 > 0.0)) return false;
    l0[5] = sqrt(v22);
    double rhs[3], y[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
      rhs[r] = -g[r] - (l1[3 * r] * y1[0] + l1[3 * r + 1] * y1[1] + l1[3 * r + 2] * y1[2]) -
               (l2[3 * r] * y2[0] + l2[3 * r + 1] * y2[1] + l2[3 * r + 2] * y2[2]);
    lsolve3(l0, rhs, y);
    if (lane == 0) {
      double* o = L + (size_t)24 * t;
#pragma unroll
      for (int m = 0; m < 6; ++m) o[m] = l0[m];
#pragma unroll
      for (int m = 0; m < 9; ++m) { o[6 + m] = l1[m]; o[15 + m] = l2[m]; }
      Y[3 * t] = y[0]; Y[3 * t + 1] = y[1]; Y[3 * t + 2] = y[2];
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) { p2[m] = p1[m]; p1[m] = l0[m]; }
#pragma unroll
    for (int m = 0; m < 9; ++m) q1[m] = l1[m];
#pragma unroll
    for (int m = 0; m < 3; ++m) { y2[m] = y1[m]; y1[m] = y[m]; }
  }
  return true;
}

// L^T d = y, from the last frame down: d_t = L_tt^-T (y_t - L_t+1,t^T d_t+1 - L_t+2,t^T d_t+2).  d replaces y in DX.
static __device__ void ts_back(double* w, int T, int lane) {
  __syncthreads();                                                    // lane 0's factor and y are read by every lane
  const double* L = w + (size_t)kTsL * T;
  double* Y = w + (size_t)kTsDX * T;
  double a1[9], a2[9], a2n[9], d1[3] = {0.0, 0.0, 0.0}, d2[3] = {0.0, 0.0, 0.0};            // L_t+1,t; L_t+2,t; L_t+1,t-1
#pragma unroll
  for (int m = 0; m < 9; ++m) { a1[m] = 0.0; a2[m] = 0.0; a2n[m] = 0.0; }
  double nl[24], ny[3];
#pragma unroll
  for (int m = 0; m < 24; ++m) nl[m] = L[(size_t)24 * (T - 1) + m];
#pragma unroll
  for (int m = 0; m < 3; ++m) ny[m] = Y[3 * (T - 1) + m];
  for (int t = T - 1; t >= 0; --t) {
    double l[24], y[3];
#pragma unroll
    for (int m = 0; m < 24; ++m) l[m] = nl[m];
#pragma unroll
    for (int m = 0; m < 3; ++m) y[m] = ny[m];
    const int tn = t > 0 ? t - 1 : 0;                                 // the frame below, ahead of its use
#pragma unroll
    for (int m = 0; m < 24; ++m) nl[m] = L[(size_t)24 * tn + m];
#pragma unroll
    for (int m = 0; m < 3; ++m) ny[m] = Y[3 * tn + m];
    double rhs[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      rhs[c] = y[c] - (a1[c] * d1[0] + a1[3 + c] * d1[1] + a1[6 + c] * d1[2]) - (a2[c] * d2[0] + a2[3 + c] * d2[1] + a2[6 + c] * d2[2]);
    const double l0[6] = {l[0], l[1], l[2], l[3], l[4], l[5]};
    ltsolve3(l0, rhs, d);
    if (lane == 0) { Y[3 * t] = d[0]; Y[3 * t + 1] = d[1]; Y[3 * t + 2] = d[2]; }
#pragma unroll
    for (int m = 0; m < 9; ++m) { a2[m] = a2n[m]; a2n[m] = l[15 + m]; a1[m] = l[6 + m]; }
#pragma unroll
    for (int m = 0; m < 3; ++m) { d2[m] = d1[m]; d1[m] = d[m]; }
  }
  __syncthreads();
}

// The whole of a wave's work: the body of both kernels (launch bounds 64, one block per (track, joint)).
template <class Data>
__device__ __forceinline__ void ts_run(const TsArgs& a, const TsOut& o, int mode, const Data& data) {
  const int p = blockIdx.x, s = p / a.K, k = p - s * a.K, lane = threadIdx.x;
  const int n0 = a.start[s], T = a.start[s + 1] - n0;
  double* w = a.ws + ((size_t)n0 * a.K + (size_t)k * T) * kTsRec;
  const int* fr = a.frame + n0;
  int* usedw = (int*)(w + (size_t)kTsUsed * T);
  double* X0 = w + (size_t)kTsX * T;

  // which frames have data, and their start
  double cnt = 0.0;
  for (int t = lane; t < T; t += 64) {
    double X[3];
    const int used = data.classify(a, n0 + t, k, X);
    usedw[t] = used;
    X0[3 * t] = X[0]; X0[3 * t + 1] = X[1]; X0[3 * t + 2] = X[2];
    cnt += used ? 1.0 : 0.0;
  }
  const double ndata = lane0(wave_sum_d(cnt));
  __syncthreads();
  if (ndata < 2.0) {                                                  // passed through: init bit for bit, NaN stays NaN
    for (int t = lane; t < T; t += 64) {
      const size_t i = (size_t)(n0 + t) * a.K + k;
      if (mode == TS_LINEARISE) {
        for (int m = 0; m < 27; ++m) o.band[i * 27 + m] = 0.0;
        for (int m = 0; m < 3; ++m) o.g[i * 3 + m] = 0.0;
        continue;
      }
      const float* in = a.init + i * 4;
      const float x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3];
      float* q = o.out + i * 4;
      q[0] = x0; q[1] = x1; q[2] = x2; q[3] = x3;
      if (o.status) o.status[i] = 2;
      if (o.resid) { o.resid[i * 2] = NAN; o.resid[i * 2 + 1] = NAN; }
    }
    if (lane == 0) {
      if (mode == TS_LINEARISE) { o.C[p] = 0.0; return; }
      if (o.track_status) o.track_status[p] = 2;
      if (o.cost) { o.cost[(size_t)p * 2] = 0.0; o.cost[(size_t)p * 2 + 1] = 0.0; }
      if (o.trials) o.trials[p] = 0;
    }
    return;
  }
  // gap frames: between data frames the line through them in `frame`, beyond the ends the nearest data frame's point
  for (int t = lane; t < T; t += 64) {
    if (usedw[t]) continue;
    int l = t - 1, r = t + 1;
    while (l >= 0 && !usedw[l]) --l;
    while (r < T && !usedw[r]) ++r;
    double X[3];
    if (l >= 0 && r < T) {
      const double f = ((double)fr[t] - (double)fr[l]) / ((double)fr[r] - (double)fr[l]);
#pragma unroll
      for (int m = 0; m < 3; ++m) X[m] = X0[3 * l + m] + (X0[3 * r + m] - X0[3 * l + m]) * f;
    } else {
      const int e = l >= 0 ? l : r;
#pragma unroll
      for (int m = 0; m < 3; ++m) X[m] = X0[3 * e + m];
    }
    X0[3 * t] = X[0]; X0[3 * t + 1] = X[1]; X0[3 * t + 2] = X[2];
  }
  // the prior's matrix: row t sums the stencils that cover t, in ascending order
  double* A = w + (size_t)kTsA * T;
  for (int t = lane; t < T; t += 64) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int c = t - 1; c <= t + 1; ++c) {
      if (c < 1 || c > T - 2) continue;
      const TsStencil st = ts_stencil(fr, c);
      const double ct = st.at(c, t);
      a0 += st.ws * ct * ct;
      if (c <= t) a1 += st.ws * ct * st.at(c, t - 1);
      if (c == t - 1) a2 += st.ws * st.cp * st.cm;
    }
    A[3 * t] = a0; A[3 * t + 1] = a1; A[3 * t + 2] = a2;
  }
  double C;
  bool bad;
  ts_eval(a, data, w, fr, n0, T, k, 0, lane, C, bad);                 // its first barrier publishes everything above

  if (mode == TS_LINEARISE) {                                         // the band of H + lambda diag H, g and C at the start
    const double* D = w + (size_t)kTsD * T;
    const double* G = w + (size_t)kTsG * T;
    for (int t = lane; t < T; t += 64) {
      const size_t i = (size_t)(n0 + t) * a.K + k;
      const double d[6] = {D[6 * t], D[6 * t + 1], D[6 * t + 2], D[6 * t + 3], D[6 * t + 4], D[6 * t + 5]};
      const double b0 = a.acc_w * A[3 * t], b1 = a.acc_w * A[3 * t + 1], b2 = a.acc_w * A[3 * t + 2];
      const double full[3][3] = {{d[0] + b0, d[1], d[2]}, {d[1], d[3] + b0, d[4]}, {d[2], d[4], d[5] + b0}};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double* q = o.band + i * 27 + c * 9;
#pragma unroll
        for (int off = 0; off < 9; ++off) {
          double v = 0.0;
          if (off == 0) v = full[c][c] * (1.0 + o.lambda);
          else if (off <= c) v = full[c][c - off];
          else if (off == 3) v = b1;
          else if (off == 6) v = b2;
          q[off] = v;
        }
        o.g[i * 3 + c] = G[3 * t + c];
      }
    }
    if (lane == 0) o.C[p] = C;
    return;
  }

  const double C_init = C;
  if (o.resid) {
    const double* R2 = w + (size_t)kTsR2 * T;
    for (int t = lane; t < T; t += 64) {
      const size_t i = (size_t)(n0 + t) * a.K + k;
      o.resid[i * 2] = ts_rms(R2[t], usedw[t]);
    }
  }
  int cur = 0, st = 1, made = 0;
  double lambda = kLmLambda0;
  for (int it = 0; it < a.max_iter; ++it) {
    ++made;
    bool accept = false;
    double Ct = 0.0, big = 0.0;
    if (ts_factor(w, T, cur, lambda, a.acc_w, lane)) {
      ts_back(w, T, lane);
      const double* Xc = w + (size_t)(kTsX + 3 * cur) * T;
      double* Xt = w + (size_t)(kTsX + 3 * (cur ^ 1)) * T;
      const double* dx = w + (size_t)kTsDX * T;
      for (int t = lane; t < T; t += 64) {
        const double d0 = dx[3 * t], d1 = dx[3 * t + 1], d2 = dx[3 * t + 2];
        Xt[3 * t] = Xc[3 * t] + d0; Xt[3 * t + 1] = Xc[3 * t + 1] + d1; Xt[3 * t + 2] = Xc[3 * t + 2] + d2;
        big = fmax(big, sqrt(d0 * d0 + d1 * d1 + d2 * d2));
      }
      big = lane0(wave_max_d(big));
      bool behind;
      ts_eval(a, data, w, fr, n0, T, k, cur ^ 1, lane, Ct, behind);
      accept = !behind && Ct < C;                                     // NaN never passes
    }
    if (accept) {
      cur ^= 1; C = Ct;
      lambda *= kLmAccept;
      if (big < kLmStepTol) { st = 0; break; }
    } else {
      lambda *= kLmReject;
      if (lambda > kLmLambdaMax) break;
    }
  }
  const double* Xc = w + (size_t)(kTsX + 3 * cur) * T;
  const double* R2 = w + (size_t)(kTsR2 + cur) * T;
  for (int t = lane; t < T; t += 64) {
    const size_t i = (size_t)(n0 + t) * a.K + k;
    const float x3 = a.init[i * 4 + 3];
    float* q = o.out + i * 4;
    q[0] = (float)Xc[3 * t]; q[1] = (float)Xc[3 * t + 1]; q[2] = (float)Xc[3 * t + 2]; q[3] = x3;
    if (o.status) o.status[i] = usedw[t] ? 0 : 1;
    if (o.resid) o.resid[i * 2 + 1] = ts_rms(R2[t], usedw[t]);
  }
  if (lane == 0) {
    if (o.track_status) o.track_status[p] = (unsigned char)st;
    if (o.cost) { o.cost[(size_t)p * 2] = C_init; o.cost[(size_t)p * 2 + 1] = C; }
    if (o.trials) o.trials[p] = made;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static inline size_t ts_workspace_bytes(int N, int K) {
  if (!(N > 0 && K > 0 && (long)N * K <= 0x7fffffffL)) return 0;
  return track_table_bytes(N) + (size_t)N * K * kTsRec * sizeof(double);
}

// The checks the entry points share (vmin: the fewest views the entry point takes), the copy of `start` into the workspace and
// the kernel's arguments.  The launches of the copy come last: an entry point's own checks stand before its call of this.
static inline int ts_plan(const char* who, int vmin, const float* points, const float* P, const float* init,
                          const unsigned char* views, const int* start, const int* frame, int N, int V, int K, int S, int flags,
                          float huber, double acc_w, void* workspace, hipStream_t s, TsArgs& a) {
  XAS_REQUIRE(points && P && init && start && frame && workspace,
              "%s: null buffer (points, P, init, start, frame and workspace are required)", who);
  if (tri_check_views(who, V, vmin) || tri_check_shape(who, N, K, "N > 0, K >= 1")) return 1;
  if (track_check_start(who, start, N, K, S)) return 1;
  if (tri_check_flags(who, flags)) return 1;
  XAS_REQUIRE(acc_w >= 0.0 && acc_w < INFINITY, "%s: acc_w %f (needs a finite acc_w >= 0)", who, acc_w);
  XAS_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", who);
  int* table = (int*)workspace;
  if (int e = track_copy_start(start, S, table, s)) return e;
  a = TsArgs{points, P, init, views, frame, table, (double*)((char*)workspace + track_table_bytes(N)), N, V, K, S, flags, 1,
             (double)huber, acc_w};
  return 0;
}

// What the two linearise entry points check of their own outputs, and the two smooth entry points of theirs.
static inline int ts_check_linearise(const char* who, double lambda, const double* band, const double* g, const double* C) {
  XAS_REQUIRE(band && g && C, "%s: null buffer (band, g and C are required)", who);
  XAS_REQUIRE(lambda >= 0.0 && lambda < INFINITY, "%s: lambda %f (needs a finite lambda >= 0)", who, lambda);
  return 0;
}
static inline int ts_check_smooth(const char* who, const float* init, int N, int K, int max_iter, const float* out) {
  XAS_REQUIRE(out, "%s: null buffer (out is required)", who);
  if (tri_check_iter(who, max_iter)) return 1;
  if (init && N > 0 && K > 0) {
    const size_t nout = (size_t)N * K * 4;
    XAS_REQUIRE(out + nout <= init || init + nout <= out, "%s: out must not overlap init (a passed-through frame is copied from it)", who);
  }
  return 0;
}

}  // namespace xas
