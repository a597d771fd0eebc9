// Bundle adjustment of the camera extrinsics on the device (gfx950; eval.py --calibrate, no reference counterpart): per rig one
// Levenberg-Marquardt problem over a 6-vector (omega, tau) per free camera and every free point of the rig's samples, the points
// eliminated by a Schur complement.  include/xas_hip.h states the problem; this file is its schedule.
// State in the workspace, per rig: lambda, the running cost, which of two copies of (points, corrections) is current, a
// "stopped" word, counters.  One TRIAL is four launches, all enqueued up front; a stopped rig's blocks return at once:
//   calib_assemble  point blocks (256 points each, a rig's blocks start at its first point).  32 points at a time: a thread per
//                   point writes its rows to LDS (per free camera it uses: sqrt(w) (du, dv) / d delta, W = B chol(A)^-T, the
//                   scaled residual; y = chol(A)^-1 g_p), then a thread per ENTRY of (H_cc - sum W W^T, g_c - sum W y, diag
//                   H_cc) adds the 32 points in point order; only the camera pairs a point uses are visited.  One partial per
//                   block and entry.
//   calib_solve     a block per rig: the partials added in block order, prior and damping on the diagonal, Cholesky of S packed
//                   in LDS, d_c, the trial corrections.
//   calib_cost      point blocks, a thread per point: d_p by back-substitution (its 3x3 system formed again, not stored), the
//                   trial point, and the trial cost: per block one partial (cost, |r|^2, views, behind, largest step).
//   calib_decide    a thread per rig: the partials added in block order, the prior, accept or reject, lambda, the stop rules.
// calib_cost and calib_decide also run once before the first trial (which points are free, the start cost).  Nothing is an
// atomic and every sum has one order: lanes by a butterfly, waves and blocks ascending.  All arithmetic is double.
#include <math.h>

#include "multiview.h"

namespace xas {

constexpr int kCalV = XAS_TRI_MAX_VIEWS, kCalN = 6 * kCalV, kCalTri = kCalN * (kCalN + 1) / 2, kCalE = kCalTri + 2 * kCalN;
constexpr int kCalBlock = 256, kCalChunk = 32, kCalCam = 21, kCalR = XAS_CALIB_MAX_RIGS;
constexpr int kCalRs = 8, kCalRi = 8, kCalCp = 8;                      // doubles / ints of a rig's state, doubles of a cost partial
static_assert(kCalE <= 3 * kCalBlock, "calib_assemble: three entries per thread");
enum { RS_LAMBDA, RS_C, RS_C0, RS_R2_0, RS_R2, RS_CNT, RS_ROT, RS_TRANS };
enum { RI_CUR, RI_STOPPED, RI_STATUS, RI_ACCEPTED, RI_TRIALS, RI_SOLVED };
enum { CAL_SOLVE, CAL_EXPORT, CAL_COV };

struct CalRigs {
  int start[kCalR + 1], blk[kCalR + 1];                               // first sample and first point block of every rig
};
struct CalArgs {
  const float *pts, *P, *init;
  const unsigned char* views;
  int N, V, K, R, free_mask, nfree, flags;
  double huber, prior_rot, prior_trans;
};
struct CalWs {
  double *X, *part, *cpart, *rs, *delta, *dc;                         // X [2][N K][3], delta [2][R][6][6], dc [R][36]
  int *free, *ri;
};

__device__ __forceinline__ int cal_rig(const CalRigs& g, int R, int blk) {
  int r = 0;
  while (r + 1 < R && blk >= g.blk[r + 1]) ++r;
  return r;
}
__device__ __forceinline__ int cal_slot(int free_mask, int v) { return __popc(free_mask & ((1 << v) - 1)); }
__device__ __forceinline__ int cal_view_of(int free_mask, int slot) {
  int v = 0;
  for (int m = free_mask; m; m &= m - 1, --slot)
    if (slot == 0) { v = __ffs(m) - 1; break; }
  return v;
}

// c [21] of a correction d = (omega, tau): R = exp([omega]x) row-major, tau, and the left Jacobian Jl of the exponential map,
// d (R X) / d omega = -[R X]x Jl.  th^2 < 1e-16: the series R = I + K + K^2 / 2, Jl = I + K / 2 + K^2 / 6.
__device__ __forceinline__ void cal_camera(const double* d, double* c) {
  const double w0 = d[0], w1 = d[1], w2 = d[2], th2 = w0 * w0 + w1 * w1 + w2 * w2;
  double a = 1.0, b = 0.5, cc = 1.0 / 6.0;
  if (!(th2 < 1e-16)) {
    const double th = sqrt(th2);
    a = sin(th) / th; b = (1.0 - cos(th)) / th2; cc = (th - sin(th)) / (th2 * th);
  }
  const double Km[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
  const double K2[9] = {w0 * w0 - th2, w0 * w1, w0 * w2, w1 * w0, w1 * w1 - th2, w1 * w2, w2 * w0, w2 * w1, w2 * w2 - th2};
#pragma unroll
  for (int n = 0; n < 9; ++n) {
    const double e = (n % 4 == 0) ? 1.0 : 0.0;
    c[n] = e + a * Km[n] + b * K2[n];
    c[12 + n] = e + b * Km[n] + cc * K2[n];
  }
  c[9] = d[3]; c[10] = d[4]; c[11] = d[5];
}

// One view's term at the world point X under the camera constants c: X' = R X + tau, multiview.h's term at X', then ju / jv
// turned into the derivative by X (R^T ju); with `cam` also cu / cv = d (u, v) / d (omega, tau) = (Jl^T (R X x ju), ju).
struct CalView {
  ReprojTerm t;
  double cu[6], cv[6];
};
__device__ __forceinline__ void cal_view(const float* __restrict__ Pm, const double* c, const double (&X)[3], double u, double v,
                                         double s, double huber, bool cam, CalView& o) {
  double a[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) a[r] = c[3 * r] * X[0] + c[3 * r + 1] * X[1] + c[3 * r + 2] * X[2];
  const double Xh[4] = {a[0] + c[9], a[1] + c[10], a[2] + c[11], 1.0};
  o.t = reproj_term(Pm, Xh, u, v, s, huber);
  const double ju[3] = {o.t.ju[0], o.t.ju[1], o.t.ju[2]}, jv[3] = {o.t.jv[0], o.t.jv[1], o.t.jv[2]};
  if (cam) {
    const double mu[3] = {a[1] * ju[2] - a[2] * ju[1], a[2] * ju[0] - a[0] * ju[2], a[0] * ju[1] - a[1] * ju[0]};
    const double mv[3] = {a[1] * jv[2] - a[2] * jv[1], a[2] * jv[0] - a[0] * jv[2], a[0] * jv[1] - a[1] * jv[0]};
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      o.cu[n] = c[12 + n] * mu[0] + c[15 + n] * mu[1] + c[18 + n] * mu[2];
      o.cv[n] = c[12 + n] * mv[0] + c[15 + n] * mv[1] + c[18 + n] * mv[2];
      o.cu[3 + n] = ju[n]; o.cv[3 + n] = jv[n];
    }
  }
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    o.t.ju[n] = c[n] * ju[0] + c[3 + n] * ju[1] + c[6 + n] * ju[2];
    o.t.jv[n] = c[n] * jv[0] + c[3 + n] * jv[1] + c[6 + n] * jv[2];
  }
}

// The fit (multiview.h's PointFit) of the point X under the cameras cam [V][21]: cal_view's terms, summed as everywhere else.
__device__ __forceinline__ bool cal_fit(const CalArgs& a, const float* Pb, const double (*cam)[kCalCam], const ViewObs& o, int used,
                                        const double (&X)[3], PointFit& f) {
  return fit_views(used, a.huber, [&](int v) {
    CalView w;
    cal_view(Pb + v * 12, cam[v], X, (double)o.pu[v], (double)o.pv[v], (double)o.ps[v], a.huber, false, w);
    return w.t;
  }, f);
}

// The point's own 3x3 system at X: A = H_pp + lambda diag H_pp factored, L L^T = A (chol3: a pivot that is not positive leaves
// NaN, which no later comparison passes), and y = L^-1 g_p.
__device__ __forceinline__ void cal_point_system(const CalArgs& a, const float* Pb, const double (*cam)[kCalCam], const ViewObs& o,
                                                 int used, const double (&X)[3], double lambda, double (&L)[6], double (&y)[3]) {
  PointFit f;
  cal_fit(a, Pb, cam, o, used, X, f);
  f.H[0] *= 1.0 + lambda; f.H[3] *= 1.0 + lambda; f.H[5] *= 1.0 + lambda;
  chol3(f.H, L);
  lsolve3(L, f.g, y);
}

struct CalRec {
  double cu[kCalV][6], cv[kCalV][6], W[kCalV][6][3], r[kCalV][2], y[3];
  int cams, pad;                                                      // mask of the camera SLOTS the point has rows for
};
static_assert(sizeof(CalRec) * kCalChunk <= 56 * 1024, "calib_assemble: static LDS of one block");

__global__ __launch_bounds__(kCalBlock) void calib_assemble_kernel(CalArgs a, CalRigs g, CalWs w, double lambda_arg, int force) {
  __shared__ CalRec rec[kCalChunk];
  __shared__ double cam[kCalV][kCalCam];
  const int tid = threadIdx.x, r = cal_rig(g, a.R, blockIdx.x);
  if (!force && w.ri[r * kCalRi + RI_STOPPED]) return;
  const int cur = w.ri[r * kCalRi + RI_CUR], NK = a.N * a.K;
  const double lambda = lambda_arg >= 0.0 ? lambda_arg : w.rs[r * kCalRs + RS_LAMBDA];
  if (tid < a.V) cal_camera(w.delta + ((size_t)(cur * a.R + r) * kCalV + tid) * 6, cam[tid]);
  const int n = 6 * a.nfree, nT = n * (n + 1) / 2, nE = nT + 2 * n;
  int kind[3], ei[3], ej[3];                                          // 0 = entry (i, j) of the matrix, 1 = gradient i, 2 = diagonal i
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const int e = tid + kCalBlock * h;
    kind[h] = -1; ei[h] = 0; ej[h] = 0;
    if (e < nT) {
      int i = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
      while (i * (i + 1) / 2 > e) --i;
      while ((i + 1) * (i + 2) / 2 <= e) ++i;
      kind[h] = 0; ei[h] = i; ej[h] = e - i * (i + 1) / 2;
    } else if (e < nE) {
      kind[h] = e < nT + n ? 1 : 2;
      ei[h] = e < nT + n ? e - nT : e - nT - n;
    }
  }
  double acc[3] = {0.0, 0.0, 0.0};
  const int base = g.start[r] * a.K + (blockIdx.x - g.blk[r]) * kCalBlock, end = g.start[r + 1] * a.K;
  __syncthreads();
  for (int c = 0; c < kCalBlock / kCalChunk; ++c) {
    const int p0 = base + c * kCalChunk;
    if (p0 >= end) break;                                             // the same for every thread
    const int np = min(kCalChunk, end - p0);
    if (tid < np) {
      const int i = p0 + tid, used = w.free[i];
      CalRec& q = rec[tid];
      int cams = 0;
      if (used) {
        const int b = i / a.K, k = i - b * a.K;
        const float* Pb = a.P + (size_t)b * a.V * 12;
        ViewObs o;
        load_obs(a.pts, b, a.V, a.K, k, a.flags, o);
        const double* xp = w.X + ((size_t)cur * NK + i) * 3;
        const double X[3] = {xp[0], xp[1], xp[2]};
        double L[6], y[3];
        cal_point_system(a, Pb, cam, o, used, X, lambda, L, y);
        q.y[0] = y[0]; q.y[1] = y[1]; q.y[2] = y[2];
#pragma unroll
        for (int v = 0; v < kCalV; ++v) {
          if (!((used >> v) & 1) || !((a.free_mask >> v) & 1)) continue;
          const int sl = cal_slot(a.free_mask, v);
          CalView vw;
          cal_view(Pb + v * 12, cam[v], X, (double)o.pu[v], (double)o.pv[v], (double)o.ps[v], a.huber, true, vw);
          const double sw = sqrt(vw.t.w);
          q.r[sl][0] = sw * vw.t.ru; q.r[sl][1] = sw * vw.t.rv;
#pragma unroll
          for (int m = 0; m < 6; ++m) {
            q.cu[sl][m] = sw * vw.cu[m]; q.cv[sl][m] = sw * vw.cv[m];
            const double B[3] = {vw.t.w * (vw.cu[m] * vw.t.ju[0] + vw.cv[m] * vw.t.jv[0]),
                                 vw.t.w * (vw.cu[m] * vw.t.ju[1] + vw.cv[m] * vw.t.jv[1]),
                                 vw.t.w * (vw.cu[m] * vw.t.ju[2] + vw.cv[m] * vw.t.jv[2])};
            double W[3];
            lsolve3(L, B, W);
            q.W[sl][m][0] = W[0]; q.W[sl][m][1] = W[1]; q.W[sl][m][2] = W[2];
          }
          cams |= 1 << sl;
        }
      }
      q.cams = cams;
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      if (kind[h] < 0) continue;
      const int vi = ei[h] / 6, ci = ei[h] - 6 * vi, vj = ej[h] / 6, cj = ej[h] - 6 * vj;
      for (int p = 0; p < np; ++p) {
        const CalRec& q = rec[p];
        if (!((q.cams >> vi) & 1)) continue;
        if (kind[h] == 0) {
          if (!((q.cams >> vj) & 1)) continue;
          double s = -(q.W[vi][ci][0] * q.W[vj][cj][0] + q.W[vi][ci][1] * q.W[vj][cj][1] + q.W[vi][ci][2] * q.W[vj][cj][2]);
          if (vi == vj) s += q.cu[vi][ci] * q.cu[vi][cj] + q.cv[vi][ci] * q.cv[vi][cj];
          acc[h] += s;
        } else if (kind[h] == 1) {
          acc[h] += q.cu[vi][ci] * q.r[vi][0] + q.cv[vi][ci] * q.r[vi][1] -
                    (q.W[vi][ci][0] * q.y[0] + q.W[vi][ci][1] * q.y[1] + q.W[vi][ci][2] * q.y[2]);
        } else {
          acc[h] += q.cu[vi][ci] * q.cu[vi][ci] + q.cv[vi][ci] * q.cv[vi][ci];
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int h = 0; h < 3; ++h)
    if (kind[h] >= 0) w.part[(size_t)blockIdx.x * kCalE + tid + kCalBlock * h] = acc[h];
}

// x (in LDS or registers of one thread) <- (L L^T)^-1 x, L packed lower in Lm.
__device__ __forceinline__ void cal_chol_solve(const double* Lm, int n, double* x) {
  for (int i = 0; i < n; ++i) {
    double s = x[i];
    for (int k = 0; k < i; ++k) s -= Lm[tri_idx(i, k)] * x[k];
    x[i] = s / Lm[tri_idx(i, i)];
  }
  for (int i = n - 1; i >= 0; --i) {
    double s = x[i];
    for (int k = i + 1; k < n; ++k) s -= Lm[tri_idx(k, i)] * x[k];
    x[i] = s / Lm[tri_idx(i, i)];
  }
}

__global__ __launch_bounds__(kCalBlock) void calib_solve_kernel(CalArgs a, CalRigs g, CalWs w, double lambda_arg, int mode,
                                                                double* __restrict__ o0, double* __restrict__ o1,
                                                                double* __restrict__ o2) {
  __shared__ double T[kCalE], gv[kCalN], x[kCalN][kCalN + 1], piv;
  const int tid = threadIdx.x, r = blockIdx.x;
  if (mode == CAL_SOLVE && w.ri[r * kCalRi + RI_STOPPED]) return;
  const int cur = w.ri[r * kCalRi + RI_CUR], n = 6 * a.nfree, nT = n * (n + 1) / 2, nE = nT + 2 * n;
  const double lambda = lambda_arg >= 0.0 ? lambda_arg : w.rs[r * kCalRs + RS_LAMBDA];
  const double* dcur = w.delta + (size_t)(cur * a.R + r) * kCalN;
  for (int e = tid; e < nE; e += kCalBlock) {
    double s = 0.0;
    for (int blk = g.blk[r]; blk < g.blk[r + 1]; ++blk) s += w.part[(size_t)blk * kCalE + e];
    T[e] = s;
  }
  __syncthreads();
  if (tid < n) {
    const int v = cal_view_of(a.free_mask, tid / 6), c = tid % 6;
    const double p = c < 3 ? a.prior_rot : a.prior_trans;
    T[tri_idx(tid, tid)] += p + lambda * (T[nT + n + tid] + p);
    gv[tid] = T[nT + tid] + p * dcur[v * 6 + c];
  }
  __syncthreads();
  if (mode == CAL_EXPORT) {                                           // S [R][n][n] symmetric, b = -g [R][n], C [R]
    for (int e = tid; e < n * n; e += kCalBlock) {
      const int i = e / n, j = e - i * n;
      o0[(size_t)r * n * n + e] = T[i >= j ? tri_idx(i, j) : tri_idx(j, i)];
    }
    if (tid < n) o1[(size_t)r * n + tid] = -gv[tid];
    if (tid == 0) o2[r] = w.rs[r * kCalRs + RS_C];
    return;
  }
  bool ok = true;                                                     // Cholesky in place, left-looking, thread = row
  for (int j = 0; j < n; ++j) {
    if (tid == 0) {
      double d = T[tri_idx(j, j)];
      for (int k = 0; k < j; ++k) d -= T[tri_idx(j, k)] * T[tri_idx(j, k)];
      piv = d;
    }
    __syncthreads();
    const double d = piv;
    if (!(d > 0.0)) { ok = false; break; }                            // the same d on every thread; NaN fails too
    const double sd = sqrt(d);
    if (tid > j && tid < n) {
      double s = T[tri_idx(tid, j)];
      for (int k = 0; k < j; ++k) s -= T[tri_idx(tid, k)] * T[tri_idx(j, k)];
      T[tri_idx(tid, j)] = s / sd;
    }
    __syncthreads();
    if (tid == 0) T[tri_idx(j, j)] = sd;
    __syncthreads();
  }
  if (mode == CAL_COV) {                                              // o0 = cam_cov [R][6V][6V]: the inverse, by view
    const int m = 6 * a.V;
    for (int e = tid; e < m * m; e += kCalBlock) o0[(size_t)r * m * m + e] = 0.0;
    __syncthreads();
    if (tid < n) {
      for (int i = 0; i < n; ++i) x[tid][i] = i == tid ? 1.0 : 0.0;
      if (ok) cal_chol_solve(T, n, x[tid]);
      const int row = cal_view_of(a.free_mask, tid / 6) * 6 + tid % 6;
      for (int i = 0; i < n; ++i)
        o0[(size_t)r * m * m + (size_t)row * m + cal_view_of(a.free_mask, i / 6) * 6 + i % 6] = ok ? x[tid][i] : NAN;
    }
    return;
  }
  if (tid != 0) return;
  if (!ok) { w.ri[r * kCalRi + RI_SOLVED] = 0; return; }
  for (int i = 0; i < n; ++i) x[0][i] = -gv[i];
  cal_chol_solve(T, n, x[0]);
  double* dnew = w.delta + (size_t)((cur ^ 1) * a.R + r) * kCalN;
  double rot = 0.0, trans = 0.0;
  for (int i = 0; i < kCalN; ++i) dnew[i] = dcur[i];
  for (int i = 0; i < n; ++i) {
    const int v = cal_view_of(a.free_mask, i / 6), c = i % 6;
    w.dc[r * kCalN + i] = x[0][i];
    dnew[v * 6 + c] = dcur[v * 6 + c] + x[0][i];
    if (c < 3) rot = fmax(rot, fabs(x[0][i])); else trans = fmax(trans, fabs(x[0][i]));
  }
  w.rs[r * kCalRs + RS_ROT] = rot; w.rs[r * kCalRs + RS_TRANS] = trans;
  w.ri[r * kCalRi + RI_SOLVED] = 1;
}

__global__ __launch_bounds__(kCalBlock) void calib_cost_kernel(CalArgs a, CalRigs g, CalWs w, int init_mode) {
  __shared__ double cam[2][kCalV][kCalCam], dc[kCalN], red[kCalBlock / 64][5];
  const int tid = threadIdx.x, r = cal_rig(g, a.R, blockIdx.x), NK = a.N * a.K;
  if (!init_mode && (w.ri[r * kCalRi + RI_STOPPED] || !w.ri[r * kCalRi + RI_SOLVED])) return;
  const int cur = init_mode ? 0 : w.ri[r * kCalRi + RI_CUR], dst = init_mode ? 0 : cur ^ 1;
  const double lambda = w.rs[r * kCalRs + RS_LAMBDA];
  if (tid < a.V) {
    cal_camera(w.delta + ((size_t)(cur * a.R + r) * kCalV + tid) * 6, cam[0][tid]);
    cal_camera(w.delta + ((size_t)(dst * a.R + r) * kCalV + tid) * 6, cam[1][tid]);
  }
  if (tid >= 64 && tid < 64 + kCalN) dc[tid - 64] = init_mode ? 0.0 : w.dc[r * kCalN + tid - 64];
  __syncthreads();
  const int i = g.start[r] * a.K + (blockIdx.x - g.blk[r]) * kCalBlock + tid;
  double C = 0.0, r2 = 0.0, cnt = 0.0, bad = 0.0, step = 0.0;
  if (i < g.start[r + 1] * a.K) {
    const int b = i / a.K, k = i - b * a.K;
    const float* Pb = a.P + (size_t)b * a.V * 12;
    ViewObs o;
    load_obs(a.pts, b, a.V, a.K, k, a.flags, o);
    if (init_mode) {                                                  // free by multiview.h's pass-through rule
      const int used = views_used(o.valid, a.views ? a.views[i] : 0), nused = __popc(used);
      const float* in = a.init + (size_t)i * 4;
      const double X[3] = {(double)in[0], (double)in[1], (double)in[2]};
      PointFit f;
      const bool isfree = point_startable(nused, X) && cal_fit(a, Pb, cam[0], o, used, X, f);
      if (isfree) { C = f.C; r2 = f.r2; cnt = (double)nused; }
      w.free[i] = isfree ? used : 0;
      double* xp = w.X + (size_t)i * 3;
      xp[0] = X[0]; xp[1] = X[1]; xp[2] = X[2];
    } else {
      const int used = w.free[i];
      if (used) {
        const double* xp = w.X + ((size_t)cur * NK + i) * 3;
        const double X[3] = {xp[0], xp[1], xp[2]};
        double L[6], z[3];
        cal_point_system(a, Pb, cam[0], o, used, X, lambda, L, z);
#pragma unroll
        for (int v = 0; v < kCalV; ++v) {                             // z = y + B^T d_c, B^T d_c = L W^T d_c folded below
          if (!((used >> v) & 1) || !((a.free_mask >> v) & 1)) continue;
          const int sl = cal_slot(a.free_mask, v);
          CalView vw;
          cal_view(Pb + v * 12, cam[0][v], X, (double)o.pu[v], (double)o.pv[v], (double)o.ps[v], a.huber, true, vw);
#pragma unroll
          for (int m = 0; m < 6; ++m) {
            const double B[3] = {vw.t.w * (vw.cu[m] * vw.t.ju[0] + vw.cv[m] * vw.t.jv[0]),
                                 vw.t.w * (vw.cu[m] * vw.t.ju[1] + vw.cv[m] * vw.t.jv[1]),
                                 vw.t.w * (vw.cu[m] * vw.t.ju[2] + vw.cv[m] * vw.t.jv[2])};
            double W[3];
            lsolve3(L, B, W);
            const double d = dc[6 * sl + m];
            z[0] += W[0] * d; z[1] += W[1] * d; z[2] += W[2] * d;
          }
        }
        const double nz[3] = {-z[0], -z[1], -z[2]};
        double d[3];                                                  // d_p = -L^-T z
        ltsolve3(L, nz, d);
        const double Xt[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
        double* xo = w.X + ((size_t)dst * NK + i) * 3;
        xo[0] = Xt[0]; xo[1] = Xt[1]; xo[2] = Xt[2];
        step = fmax(fabs(d[0]), fmax(fabs(d[1]), fabs(d[2])));
        if (!(step == step)) bad = 1.0;                               // a NaN step: fmax would drop it
        PointFit f;
        if (!cal_fit(a, Pb, cam[1], o, used, Xt, f)) bad = 1.0;
        C = f.C; r2 = f.r2;
        cnt = (double)__popc(used);
      }
    }
  }
  C = wave_sum_d(C); r2 = wave_sum_d(r2); cnt = wave_sum_d(cnt); bad = wave_sum_d(bad); step = wave_max_d(step);
  if ((tid & 63) == 0) {
    double* q = red[tid >> 6];
    q[0] = C; q[1] = r2; q[2] = cnt; q[3] = bad; q[4] = step;
  }
  __syncthreads();
  if (tid == 0) {
    for (int wv = 1; wv < kCalBlock / 64; ++wv) {
      C += red[wv][0]; r2 += red[wv][1]; cnt += red[wv][2]; bad += red[wv][3]; step = fmax(step, red[wv][4]);
    }
    double* q = w.cpart + (size_t)blockIdx.x * kCalCp;
    q[0] = C; q[1] = r2; q[2] = cnt; q[3] = bad; q[4] = step;
  }
}

__global__ __launch_bounds__(64) void calib_decide_kernel(CalArgs a, CalRigs g, CalWs w, int init_mode, double lambda0) {
  const int r = threadIdx.x;
  if (r >= a.R) return;
  int* ri = w.ri + r * kCalRi;
  double* rs = w.rs + r * kCalRs;
  if (!init_mode && ri[RI_STOPPED]) return;
  const int cur = ri[RI_CUR], which = init_mode ? cur : cur ^ 1;
  bool accept = false;
  double C = 0.0, r2 = 0.0, cnt = 0.0, bad = 0.0, step = 0.0;
  if (init_mode || ri[RI_SOLVED]) {
    for (int blk = g.blk[r]; blk < g.blk[r + 1]; ++blk) {
      const double* q = w.cpart + (size_t)blk * kCalCp;
      C += q[0]; r2 += q[1]; cnt += q[2]; bad += q[3]; step = fmax(step, q[4]);
    }
    const double* d = w.delta + (size_t)(which * a.R + r) * kCalN;
    double pr = 0.0, pt = 0.0;
    for (int v = 0; v < a.V; ++v)
      if ((a.free_mask >> v) & 1) {
        pr += d[v * 6] * d[v * 6] + d[v * 6 + 1] * d[v * 6 + 1] + d[v * 6 + 2] * d[v * 6 + 2];
        pt += d[v * 6 + 3] * d[v * 6 + 3] + d[v * 6 + 4] * d[v * 6 + 4] + d[v * 6 + 5] * d[v * 6 + 5];
      }
    C += a.prior_rot * pr + a.prior_trans * pt;
    accept = bad == 0.0 && C < rs[RS_C];                              // NaN never passes
  }
  if (init_mode) {
    const bool none = cnt == 0.0;                                      // no free point: everything passes through
    rs[RS_LAMBDA] = lambda0; rs[RS_C] = C; rs[RS_C0] = C; rs[RS_R2_0] = r2; rs[RS_R2] = r2; rs[RS_CNT] = cnt;
    ri[RI_STATUS] = none ? 2 : 1; ri[RI_STOPPED] = none ? 1 : 0;
    return;
  }
  ri[RI_TRIALS] += 1;
  if (accept) {
    ri[RI_CUR] = cur ^ 1; ri[RI_ACCEPTED] += 1;
    rs[RS_C] = C; rs[RS_R2] = r2;
    rs[RS_LAMBDA] *= kLmAccept;
    if (step < kLmStepTol && rs[RS_ROT] < XAS_CALIB_STEP_TOL_ROT && rs[RS_TRANS] < XAS_CALIB_STEP_TOL_TRANS) {
      ri[RI_STATUS] = 0; ri[RI_STOPPED] = 1;
    }
  } else {
    rs[RS_LAMBDA] *= kLmReject;
    if (rs[RS_LAMBDA] > kLmLambdaMax) ri[RI_STOPPED] = 1;
  }
}

// The start: corrections of the free cameras from `delta` (fixed cameras: 0) into both copies, every rig's words cleared.
__global__ __launch_bounds__(kCalBlock) void calib_setup_kernel(CalArgs a, CalWs w, const double* __restrict__ delta) {
  const int tid = threadIdx.x;
  for (int t = tid; t < a.R * kCalN; t += kCalBlock) {
    const int r = t / kCalN, v = (t % kCalN) / 6, c = t % 6;
    const double d = (v < a.V && ((a.free_mask >> v) & 1)) ? delta[((size_t)r * a.V + v) * 6 + c] : 0.0;
    w.delta[t] = d; w.delta[(size_t)a.R * kCalN + t] = d;
    w.dc[t] = 0.0;
  }
  for (int t = tid; t < a.R * kCalRi; t += kCalBlock) w.ri[t] = 0;
  for (int t = tid; t < a.R * kCalRs; t += kCalBlock) w.rs[t] = 0.0;
}

__global__ __launch_bounds__(kCalBlock) void calib_out_kernel(CalArgs a, CalRigs g, CalWs w, float* __restrict__ out) {
  const int i = blockIdx.x * kCalBlock + threadIdx.x, NK = a.N * a.K;
  if (i >= NK) return;
  const int b = i / a.K;
  int r = 0;
  while (r + 1 < a.R && b >= g.start[r + 1]) ++r;
  const float* in = a.init + (size_t)i * 4;
  float* o = out + (size_t)i * 4;
  const float x0 = in[0], x1 = in[1], x2 = in[2];
  o[3] = in[3];
  if (w.free[i]) {
    const double* xp = w.X + ((size_t)w.ri[r * kCalRi + RI_CUR] * NK + i) * 3;
    o[0] = (float)xp[0]; o[1] = (float)xp[1]; o[2] = (float)xp[2];
  } else {                                                            // fixed: init bit for bit, NaN stays NaN
    o[0] = x0; o[1] = x1; o[2] = x2;
  }
}

__global__ __launch_bounds__(kCalBlock) void calib_report_kernel(CalArgs a, CalWs w, double* __restrict__ delta,
                                                                 double* __restrict__ cost, double* __restrict__ rms,
                                                                 unsigned char* __restrict__ status, int* __restrict__ trials) {
  const int tid = threadIdx.x;
  for (int t = tid; t < a.R * a.V * 6; t += kCalBlock) {
    const int r = t / (a.V * 6), q = t % (a.V * 6);
    delta[t] = w.delta[(size_t)(w.ri[r * kCalRi + RI_CUR] * a.R + r) * kCalN + q];
  }
  if (tid >= a.R) return;
  const double* rs = w.rs + tid * kCalRs;
  const int* ri = w.ri + tid * kCalRi;
  if (cost) { cost[tid * 2] = rs[RS_C0]; cost[tid * 2 + 1] = rs[RS_C]; }
  if (rms) {
    rms[tid * 2] = rs[RS_CNT] > 0.0 ? sqrt(rs[RS_R2_0] / rs[RS_CNT]) : NAN;
    rms[tid * 2 + 1] = rs[RS_CNT] > 0.0 ? sqrt(rs[RS_R2] / rs[RS_CNT]) : NAN;
  }
  if (status) status[tid] = (unsigned char)ri[RI_STATUS];
  if (trials) { trials[tid * 2] = ri[RI_TRIALS]; trials[tid * 2 + 1] = ri[RI_ACCEPTED]; }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct CalLayout {
  size_t X, part, cpart, rs, delta, dc, free, ri, total;
};
static inline CalLayout cal_layout(long N, int K, int R) {
  const size_t NK = (size_t)N * K, NB = (NK + kCalBlock - 1) / kCalBlock + R;   // a rig's last block may be partial
  CalLayout l;
  size_t o = 0;
  l.X = o; o += align16(2 * NK * 3 * sizeof(double));
  l.part = o; o += align16(NB * kCalE * sizeof(double));
  l.cpart = o; o += align16(NB * kCalCp * sizeof(double));
  l.rs = o; o += align16((size_t)R * kCalRs * sizeof(double));
  l.delta = o; o += align16((size_t)2 * R * kCalN * sizeof(double));
  l.dc = o; o += align16((size_t)R * kCalN * sizeof(double));
  l.free = o; o += align16(NK * sizeof(int));
  l.ri = o; o += align16((size_t)R * kCalRi * sizeof(int));
  l.total = o;
  return l;
}
static inline bool cal_shape_ok(int N, int V, int K, int R) {
  return N > 0 && K > 0 && (long)N * K <= 0x7fffffffL && V >= 2 && V <= XAS_TRI_MAX_VIEWS && R >= 1 && R <= XAS_CALIB_MAX_RIGS;
}

struct CalPlan {
  CalArgs a;
  CalRigs g;
  CalWs w;
  unsigned blocks;
};
static int cal_plan(const char* who, const float* points, const float* P, const float* init, const unsigned char* views,
                    const int* rig_start, int N, int V, int K, int R, int free_mask, int flags, float huber, double prior_rot,
                    double prior_trans, void* workspace, CalPlan& p) {
  XAS_REQUIRE(points && P && init && rig_start && workspace, "%s: null buffer (points, P, init, rig_start and workspace are required)",
              who);
  if (tri_check_views(who, V, 2) || tri_check_shape(who, N, K, "N > 0, K >= 1")) return 1;
  XAS_REQUIRE(R >= 1 && R <= XAS_CALIB_MAX_RIGS, "%s: R=%d rigs (needs 1 <= R <= XAS_CALIB_MAX_RIGS = %d)", who, R,
              XAS_CALIB_MAX_RIGS);
  XAS_REQUIRE(rig_start[0] == 0 && rig_start[R] == N, "%s: rig_start runs from %d to %d (needs rig_start[0] = 0 and rig_start[R] = N = %d)",
              who, rig_start[0], rig_start[R], N);
  for (int r = 0; r < R; ++r)
    XAS_REQUIRE(rig_start[r] <= rig_start[r + 1], "%s: rig_start[%d] = %d > rig_start[%d] = %d (needs a non-decreasing rig_start)", who,
                r, rig_start[r], r + 1, rig_start[r + 1]);
  if (tri_check_flags(who, flags)) return 1;
  XAS_REQUIRE(free_mask >= 0, "%s: free_mask=%d (needs a mask of cameras >= 0; bits >= V are ignored)", who, free_mask);
  XAS_REQUIRE(prior_rot >= 0.0 && prior_rot < INFINITY && prior_trans >= 0.0 && prior_trans < INFINITY,
              "%s: priors %f, %f (needs finite prior_rot, prior_trans >= 0)", who, prior_rot, prior_trans);
  XAS_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", who);
  const int fm = free_mask & ((1 << V) - 1);
  int nfree = 0;
  for (int v = 0; v < V; ++v) nfree += (fm >> v) & 1;
  p.a = CalArgs{points, P, init, views, N, V, K, R, fm, nfree, flags, (double)huber, prior_rot, prior_trans};
  int blk = 0;
  for (int r = 0; r <= R; ++r) {
    p.g.start[r] = rig_start[r];
    p.g.blk[r] = blk;
    if (r < R) blk += (int)cdiv((long)(rig_start[r + 1] - rig_start[r]) * K, kCalBlock);
  }
  for (int r = R + 1; r <= kCalR; ++r) { p.g.start[r] = N; p.g.blk[r] = blk; }
  p.blocks = (unsigned)blk;
  const CalLayout l = cal_layout(N, K, R);
  char* base = (char*)workspace;
  p.w = CalWs{(double*)(base + l.X), (double*)(base + l.part), (double*)(base + l.cpart), (double*)(base + l.rs),
              (double*)(base + l.delta), (double*)(base + l.dc), (int*)(base + l.free), (int*)(base + l.ri)};
  return 0;
}

// The launches every entry point starts with: the start state, which points are free, the start cost.
static int cal_begin(const CalPlan& p, const double* delta, double lambda0, hipStream_t s) {
  hipLaunchKernelGGL(calib_setup_kernel, dim3(1), dim3(kCalBlock), 0, s, p.a, p.w, delta);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(calib_cost_kernel, dim3(p.blocks), dim3(kCalBlock), 0, s, p.a, p.g, p.w, 1);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(calib_decide_kernel, dim3(1), dim3(64), 0, s, p.a, p.g, p.w, 1, lambda0);
  XAS_LAUNCH_CHECK();
  return 0;
}

}  // namespace xas

using namespace xas;

extern "C" size_t xas_calibrate_workspace_bytes(int N, int V, int K, int R) {
  if (!cal_shape_ok(N, V, K, R)) return 0;
  return cal_layout(N, K, R).total;
}

extern "C" int xas_calibrate_linearise(const float* points, const float* P, const float* init, const unsigned char* views,
                                       const int* rig_start, int N, int V, int K, int R, int free_mask, int flags, float huber,
                                       double prior_rot, double prior_trans, double lambda, const double* delta, double* S,
                                       double* b, double* C, void* workspace, void* stream) {
  CalPlan p;
  if (cal_plan("calibrate_linearise", points, P, init, views, rig_start, N, V, K, R, free_mask, flags, huber, prior_rot, prior_trans,
               workspace, p))
    return 1;
  XAS_REQUIRE(delta && C && ((S && b) || p.a.nfree == 0),
              "calibrate_linearise: null buffer (delta, S, b and C are required; S and b may be NULL when no camera is free)");
  XAS_REQUIRE(lambda >= 0.0 && lambda < INFINITY, "calibrate_linearise: lambda %f (needs a finite lambda >= 0)", lambda);
  hipStream_t s = as_stream(stream);
  if (int e = cal_begin(p, delta, lambda, s)) return e;
  hipLaunchKernelGGL(calib_assemble_kernel, dim3(p.blocks), dim3(kCalBlock), 0, s, p.a, p.g, p.w, lambda, 1);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(calib_solve_kernel, dim3((unsigned)R), dim3(kCalBlock), 0, s, p.a, p.g, p.w, lambda, (int)CAL_EXPORT, S, b, C);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_calibrate_bundle(const float* points, const float* P, const float* init, const unsigned char* views,
                                    const int* rig_start, int N, int V, int K, int R, int free_mask, int flags, float huber,
                                    double prior_rot, double prior_trans, int max_iter, double* delta, float* out, double* cost,
                                    double* rms, double* cam_cov, unsigned char* status, int* trials, void* workspace,
                                    void* stream) {
  CalPlan p;
  if (cal_plan("calibrate_bundle", points, P, init, views, rig_start, N, V, K, R, free_mask, flags, huber, prior_rot, prior_trans,
               workspace, p))
    return 1;
  XAS_REQUIRE(delta && out, "calibrate_bundle: null buffer (delta and out are required)");
  if (tri_check_iter("calibrate_bundle", max_iter)) return 1;
  const size_t nout = (size_t)N * K * 4;
  XAS_REQUIRE(out + nout <= init || init + nout <= out, "calibrate_bundle: out must not overlap init (a fixed point is copied from it)");
  hipStream_t s = as_stream(stream);
  if (int e = cal_begin(p, delta, kLmLambda0, s)) return e;
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(calib_assemble_kernel, dim3(p.blocks), dim3(kCalBlock), 0, s, p.a, p.g, p.w, -1.0, 0);
    XAS_LAUNCH_CHECK();
    hipLaunchKernelGGL(calib_solve_kernel, dim3((unsigned)R), dim3(kCalBlock), 0, s, p.a, p.g, p.w, -1.0, (int)CAL_SOLVE,
                       (double*)nullptr, (double*)nullptr, (double*)nullptr);
    XAS_LAUNCH_CHECK();
    hipLaunchKernelGGL(calib_cost_kernel, dim3(p.blocks), dim3(kCalBlock), 0, s, p.a, p.g, p.w, 0);
    XAS_LAUNCH_CHECK();
    hipLaunchKernelGGL(calib_decide_kernel, dim3(1), dim3(64), 0, s, p.a, p.g, p.w, 0, 0.0);
    XAS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(calib_out_kernel, dim3((unsigned)cdiv((long)N * K, kCalBlock)), dim3(kCalBlock), 0, s, p.a, p.g, p.w, out);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(calib_report_kernel, dim3(1), dim3(kCalBlock), 0, s, p.a, p.w, delta, cost, rms, status, trials);
  XAS_LAUNCH_CHECK();
  if (cam_cov) {                                                      // the inverse of S at the result, lambda = 0
    hipLaunchKernelGGL(calib_assemble_kernel, dim3(p.blocks), dim3(kCalBlock), 0, s, p.a, p.g, p.w, 0.0, 1);
    XAS_LAUNCH_CHECK();
    hipLaunchKernelGGL(calib_solve_kernel, dim3((unsigned)R), dim3(kCalBlock), 0, s, p.a, p.g, p.w, 0.0, (int)CAL_COV, cam_cov,
                       (double*)nullptr, (double*)nullptr);
    XAS_LAUNCH_CHECK();
  }
  return 0;
}
