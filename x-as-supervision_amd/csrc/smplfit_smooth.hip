// xas_smpl_fit_tracks_smooth / _linearise: xas_smpl_fit_tracks' problem with an acceleration prior on pose and translation over
// the usable frames of a track (include/xas_hip.h states the cost, the unwrapping and the schedule; tests/_smplfit_smooth_oracle.py
// restates them in float64 torch).  The set-up, the per-frame evaluation and assembly and the finish are smplfit_tracks.h's and
// smplfit.h's, unchanged; track_stencil.h's stencil is the smoothers'.
//
// The normal equations of a track of T usable frames are block-pentadiagonal with a border: 75 x 75 blocks H_ii (the frame's data
// block plus the prior's diagonal), H_i,i-1 = hoff[i][0] diag(w) and H_i,i-2 = hoff[i][1] diag(w), a 10 x 75 border B_i per frame
// and the 10 x 10 corner, the sum of the frames' corners.  A TRIAL is four launches on one stream:
//   assemble   frame kernel, bounded grid: after an accepted trial (or at the first) evaluate, tangents, H_i and g_i
//   solve      ONE WORKGROUP PER TRACK, the recurrence over frames in track order:
//                L_i,i-2 = H_i,i-2 L_i-2,i-2^-T                      (upper triangular: a scaled inverse)
//                L_i,i-1 = (H_i,i-1 - L_i,i-2 L_i-1,i-2^T) L_i-1,i-1^-T
//                L_ii    = chol(H_ii + lambda diag - L_i,i-1 L_i,i-1^T - L_i,i-2 L_i,i-2^T)
//                L_b,i   = (B_i - L_b,i-1 L_i,i-1^T - L_b,i-2 L_i,i-2^T) L_ii^-T      and the forward substitution as its 11th row
//              then the corner A - sum_i L_b,i L_b,i^T, its Cholesky, d beta, and the back substitution from the last frame
//   trial      frame kernel: the data cost at the trial point
//   decide     track kernel: the prior's cost at the trial point, the sum in frame order, accept or reject
// LDS of the solve (doubles): two packed diagonal factors 2 x 2850 (L_i-1,i-1; L_i-2,i-2, whose place S_i and then L_ii take),
// L_i,i-2^T packed 2850, L_i,i-1^T dense 5625, three border rows with the forward-substituted vector as row 10, 3 x 825, three
// steps 3 x 75, the corner: 17 035 doubles = 136 280 bytes of the 163 840.  L_i-1,i-2, read once per frame for the fill, comes
// from the workspace (L2), where every frame's factor lives for the back substitution.
// The triangular solves give FOUR lanes to a right-hand side: each sums every fourth term of the row's dot product, two xor
// shuffles add them in one order, no barrier inside a solve.  The Cholesky does the same per row, and every group recomputes
// the pivot, so that a column costs one barrier.  No atomics; every sum has one order.
#include "smplfit_tracks.h"
#include "track_stencil.h"

namespace xas {
namespace {

constexpr int kSmThreads = 320;                         // 80 groups of 4 lanes: 75 rows or right-hand sides at a time
constexpr int kTriY = kY * (kY + 1) / 2;                // 2850
constexpr int kBZ = (kBeta + 1) * kY;                   // border row block with the forward-substituted vector as row 10
// per frame, doubles: the factor's block row, the prior's diagonal, the whole gradient of y, the two off-diagonal scalars
constexpr int fLd = 0, fL1 = fLd + kTriY, fL2 = fL1 + kY * kY, fLb = fL2 + kTriY, fZ = fLb + kBeta * kY, fTd = fZ + kY,
              fG = fTd + kY, fOff = fG + kY, kFacD = fOff + 4;
static_assert(fZ == fLb + kBeta * kY, "the border rows and z are stored as one block");

struct SmW {
  double rot, trans;
  __device__ __forceinline__ double at(int c) const { return (c < 3 || c >= 6) ? rot : trans; }
};

struct SmShared {
  double P[2][kTriY];
  double U[kTriY];
  double E[kY * kY];
  double BZ[3][kBZ];
  double d[3][kY];
  double dg[kY];
  double A[kBeta * kBeta], rb[kBeta], db[kBeta];
  double big[kY];
  int ok;
};
static_assert(sizeof(SmShared) <= 160 * 1024, "LDS of a workgroup");

__device__ __forceinline__ double sum4(double p) {
  p += __shfl_xor(p, 1, 64);
  p += __shfl_xor(p, 2, 64);
  return p;
}

__device__ __forceinline__ const int* ulist_of(const TrackArgs& t, const int* ti) { return t.tmp + ti[iOffset]; }
__device__ __forceinline__ double* fac_of(const TrackArgs& t, int f) { return t.fac + (size_t)f * kFacD; }

__device__ __forceinline__ TsStencil sm_stencil(const TrackArgs& t, const int* ul, int k) {
  const int f3[3] = {t.frame[ul[k - 1]], t.frame[ul[k]], t.frame[ul[k + 1]]};
  return ts_stencil(f3, 1);
}
// the second difference of component c at the stencil centred at k; off = oY or oYt
__device__ __forceinline__ double sm_q(const TrackArgs& t, const int* ul, int k, const TsStencil& s, int off, int c) {
  return (s.cm * frame_of(t, ul[k - 1])[off + c] + s.c0 * frame_of(t, ul[k])[off + c]) + s.cp * frame_of(t, ul[k + 1])[off + c];
}

// The prior's cost of a track at the point `off`: thread c < 75 sums its component over the stencils in ascending order, thread 0
// sums the components in ascending order.  part: 75 doubles of LDS.  The same value on every thread.
__device__ double sm_prior_cost(const TrackArgs& t, const int* ul, int T, SmW w, int off, double* part) {
  const int tid = threadIdx.x;
  if (tid < kY) {
    double v = 0.0;
    for (int k = 1; k + 1 < T; ++k) {
      const TsStencil s = sm_stencil(t, ul, k);
      const double q = sm_q(t, ul, k, s, off, tid);
      v += s.ws * (q * q);
    }
    part[tid] = w.at(tid) * v;
  }
  __syncthreads();
  double C = 0.0;
  for (int c = 0; c < kY; ++c) C += part[c];
  __syncthreads();
  return C;
}

// After the list kernel: the usable frames of a track in its order -> tmp[offset ..) (the list kernel is done with it), and the
// root omega of each after the first replaced by the equivalent vector nearest its unwrapped predecessor.  Serial per track.
__global__ __launch_bounds__(64) void smooth_setup_kernel(TrackArgs t, int unwrap) {
  if (threadIdx.x != 0) return;
  const int* ti = t.ti + (size_t)blockIdx.x * kTrackI;
  const int* list = t.list + ti[iOffset];
  int* ul = t.tmp + ti[iOffset];
  int n = 0;
  double prev[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < ti[iCount]; ++k) {
    const int f = list[k];
    if (!t.usable[f]) continue;
    double* y = frame_of(t, f) + oY;
    if (unwrap && n > 0) {
      const double th = sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
      if (th > 0.0) {
        const double u[3] = {y[0] / th, y[1] / th, y[2] / th};
        const double kk = nearbyint((((u[0] * prev[0] + u[1] * prev[1]) + u[2] * prev[2]) - th) / 6.283185307179586476925286766559);
        if (kk != 0.0)
          for (int c = 0; c < 3; ++c) y[c] = y[c] + (6.283185307179586476925286766559 * kk) * u[c];
      }
    }
    for (int c = 0; c < 3; ++c) prev[c] = y[c];
    ul[n++] = f;
  }
}

// tracks_start_kernel with the prior's cost at the start
__global__ __launch_bounds__(128) void smooth_start_kernel(TrackArgs t, SmW w, double lambda0, int max_iters) {
  __shared__ double part[kY];
  const int trk = blockIdx.x;
  int* ti = t.ti + (size_t)trk * kTrackI;
  double* tk = t.tk + (size_t)trk * kTrackD;
  const int* ul = ulist_of(t, ti);
  const int T = ti[iUsable];
  const double Cp = (T >= 3 && w.rot + w.trans > 0.0) ? sm_prior_cost(t, ul, T, w, oY, part) : 0.0;
  if (threadIdx.x != 0) return;
  double C = 0.0;
  for (int k = 0; k < T; ++k) C += frame_of(t, ul[k])[oC];
  C += Cp;
  tk[tC0] = tk[tC] = C;
  tk[tLambda] = lambda0;
  tk[tBig] = 0.0;
  ti[iTrials] = 0;
  ti[iStatus] = T > 0 ? kStLimit : kStNoFrame;
  ti[iDone] = (T == 0 || max_iters == 0) ? 1 : 0;
  ti[iRelin] = 1;
  ti[iOk] = 0;
  ti[iFramesOk] = 0;
}

__global__ __launch_bounds__(kFitThreads) void smooth_assemble_kernel(FitArgs a, TrackArgs t) {
  __shared__ FitShared s;
  const int tid = threadIdx.x;
  double* wsb = scratch_of(t);
  for (int f = blockIdx.x; f < t.N; f += gridDim.x) {
    if (!t.usable[f]) continue;
    const int trk = t.track[f];
    const int* ti = t.ti + (size_t)trk * kTrackI;
    if (ti[iDone] || !ti[iRelin]) continue;
    double* fr = frame_of(t, f);
    fit_stage(s, a, f);
    load_point(s, t, f, trk);
    fit_evaluate(s, a, wsb, 0, 0);
    fit_tangents(s, a, wsb, 0);
    fit_assemble(s, a, fr + oH, 0);
    if (tid < kN) fr[oG + tid] = s.g[tid];
    __syncthreads();
  }
}

// Columns j < ncol of X (element (c, j) at X[c * cs + j * js], LDS) := L^-1 X, L packed lower (LDS).  Four lanes per column; the
// caller has synchronised before and synchronises after.
__device__ __forceinline__ void lower_solve4(const double* L, double* X, int cs, int js, int ncol) {
  const int j = threadIdx.x >> 2, g = threadIdx.x & 3;
  const bool on = j < ncol;
  double* x = X + (on ? j : 0) * js;
  for (int c = 0; c < kY; ++c) {
    double p = 0.0;
    if (on)
      for (int k = g; k < c; k += 4) p += L[tri(c, k)] * x[k * cs];
    p = sum4(p);
    if (on && g == 0) x[c * cs] = (x[c * cs] - p) / L[tri(c, c)];
  }
}

__global__ __launch_bounds__(kSmThreads) void smooth_solve_kernel(TrackArgs t, SmW w) {
  __shared__ SmShared s;
  const int trk = blockIdx.x, tid = threadIdx.x, row = tid >> 2, g = tid & 3, lane = tid & 63;
  int* ti = t.ti + (size_t)trk * kTrackI;
  if (ti[iDone]) return;
  double* tk = t.tk + (size_t)trk * kTrackD;
  const int* ul = ulist_of(t, ti);
  const int T = ti[iUsable];
  const double lambda = tk[tLambda];
  const bool temporal = T >= 3 && w.rot + w.trans > 0.0;

  // the prior's diagonal and gradient and the off-diagonal scalars of every frame: stencils i-1, i, i+1 in this order
  for (int e = tid; e < T * (kY + 1); e += kSmThreads) {
    const int i = e / (kY + 1), c = e % (kY + 1);
    double* fc = fac_of(t, ul[i]);
    double td = 0.0, gt = 0.0, s1 = 0.0, s2 = 0.0;
    if (temporal) {
      if (i - 1 >= 1) {
        const TsStencil st = sm_stencil(t, ul, i - 1);
        td += st.ws * (st.cp * st.cp);
        if (c < kY) gt += st.ws * (st.cp * sm_q(t, ul, i - 1, st, oY, c));
        s1 += st.ws * (st.c0 * st.cp);
        s2 += st.ws * (st.cm * st.cp);
      }
      if (i >= 1 && i + 1 < T) {
        const TsStencil st = sm_stencil(t, ul, i);
        td += st.ws * (st.c0 * st.c0);
        if (c < kY) gt += st.ws * (st.c0 * sm_q(t, ul, i, st, oY, c));
        s1 += st.ws * (st.cm * st.c0);
      }
      if (i + 2 < T) {
        const TsStencil st = sm_stencil(t, ul, i + 1);
        td += st.ws * (st.cm * st.cm);
        if (c < kY) gt += st.ws * (st.cm * sm_q(t, ul, i + 1, st, oY, c));
      }
    }
    if (c < kY) {
      fc[fTd + c] = w.at(c) * td;
      fc[fG + c] = frame_of(t, ul[i])[oG + c] + w.at(c) * gt;
    } else {
      fc[fOff] = s1;
      fc[fOff + 1] = s2;
    }
  }
  // the corner and its right-hand side, summed over the frames in track order, then damped
  if (tid < kBeta * kBeta) {
    const int a = tid / kBeta, b = tid % kBeta, hi = a > b ? a : b, lo = a > b ? b : a;
    double v = 0.0;
    for (int i = 0; i < T; ++i) v += frame_of(t, ul[i])[oH + tri(kY + hi, kY + lo)];
    if (a == b) v += lambda * v;
    s.A[tid] = v;
    if (a >= b) tk[tA + tri(a, b)] = v;
  } else if (tid >= 128 && tid < 128 + kBeta) {
    double v = 0.0;
    for (int i = 0; i < T; ++i) v += frame_of(t, ul[i])[oG + kY + tid - 128];
    s.rb[tid - 128] = -v;
    tk[tRhs + tid - 128] = v;
  }
  if (tid == 0) {
    ti[iFramesOk] = 1;                                  // the system stands, whatever becomes of the factor
    ti[iOk] = 0;
  }
  if (tid < kY) s.big[tid] = 0.0;
  __syncthreads();

  for (int i = 0; i < T; ++i) {
    const int f = ul[i];
    double* fc = fac_of(t, f);
    const double* fr = frame_of(t, f);
    const bool has1 = temporal && i >= 1, has2 = temporal && i >= 2;
    double* P = s.P[(i + 1) & 1];                       // L_i-1,i-1
    double* Q = s.P[i & 1];                             // L_i-2,i-2, then S_i, then L_ii
    double* cur = s.BZ[i % 3];
    const double* b1 = s.BZ[(i + 2) % 3];
    const double* b2 = s.BZ[(i + 1) % 3];
    const double s1 = fc[fOff], s2 = fc[fOff + 1];

    // U[tri(c, r)] = L_i,i-2[r][c], c >= r: row r of s2 diag(w) Q^-T by forward substitution, four lanes per row
    if (has2) {
      if (row < kY && g == 0) s.U[tri(row, row)] = s2 * w.at(row) / Q[tri(row, row)];
      for (int c = 1; c < kY; ++c) {
        const bool on = row < kY && c > row;
        double p = 0.0;
        if (on)
          for (int k = row + g; k < c; k += 4) p += Q[tri(c, k)] * s.U[tri(k, row)];
        p = sum4(p);
        if (on && g == 0) s.U[tri(c, row)] = -p / Q[tri(c, c)];
      }
    }
    __syncthreads();
    // E[c][r] = L_i,i-1[r][c]: (s1 diag(w) - L_i,i-2 L_i-1,i-2^T)^T, then P^-1 on its columns
    if (has1) {
      const double* lsub = fac_of(t, ul[i - 1]) + fL1;  // [k][c] = L_i-1,i-2[c][k]
      for (int e = tid; e < kY * kY; e += kSmThreads) {
        const int c = e / kY, r = e % kY;
        double v = r == c ? s1 * w.at(r) : 0.0;
        if (has2)
          for (int k = r; k < kY; ++k) v -= s.U[tri(k, r)] * lsub[k * kY + c];
        s.E[e] = v;
      }
      __syncthreads();
      lower_solve4(P, s.E, kY, 1, kY);
    }
    __syncthreads();
    // S_i into Q (L_i-2,i-2 is spent), its diagonal apart
    for (int e = tid; e < kY * kY; e += kSmThreads) {
      const int r = e / kY, c = e % kY;
      if (c > r) continue;
      double v = fr[oH + tri(r, c)];
      if (r == c) {
        v += fc[fTd + c];
        v += lambda * v;
      }
      if (has1)
        for (int k = 0; k < kY; ++k) v -= s.E[k * kY + r] * s.E[k * kY + c];
      if (has2)
        for (int k = r; k < kY; ++k) v -= s.U[tri(k, r)] * s.U[tri(k, c)];
      if (r == c) s.dg[c] = v;
      else Q[tri(r, c)] = v;
    }
    __syncthreads();
    // Cholesky in place, left-looking, four lanes per row; every group forms the pivot itself: one barrier per column
    bool fail = false;
    for (int j = 0; j < kY; ++j) {
      const bool on = row < kY && row >= j;
      double p = 0.0, pp = 0.0;
      for (int k = g; k < j; k += 4) {
        const double ljk = Q[tri(j, k)];
        pp += ljk * ljk;
        if (on) p += Q[tri(row, k)] * ljk;
      }
      p = sum4(p);
      pp = sum4(pp);
      const double piv = s.dg[j] - pp;
      if (!(piv > 0.0)) {
        fail = true;
        break;
      }
      const double sd = sqrt(piv);
      if (on && g == 0) Q[tri(row, j)] = row == j ? sd : (Q[tri(row, j)] - p) / sd;
      __syncthreads();
    }
    if (fail) return;                                   // uniform: iOk stays 0
    // border rows and the right-hand side of the forward substitution as row 10, then Q^-1 on all eleven
    for (int e = tid; e < kBZ; e += kSmThreads) {
      const int q = e / kY, c = e % kY;
      double v = q < kBeta ? fr[oH + tri(kY + q, c)] : -fc[fG + c];
      if (has1)
        for (int k = 0; k < kY; ++k) v -= b1[q * kY + k] * s.E[k * kY + c];
      if (has2)
        for (int k = c; k < kY; ++k) v -= b2[q * kY + k] * s.U[tri(k, c)];
      cur[e] = v;
    }
    __syncthreads();
    lower_solve4(Q, cur, 1, kY, kBeta + 1);
    __syncthreads();
    if (tid < kBeta * kBeta) {
      const int a = tid / kBeta, b = tid % kBeta;
      double v = s.A[tid];
      for (int c = 0; c < kY; ++c) v -= cur[a * kY + c] * cur[b * kY + c];
      s.A[tid] = v;
    } else if (tid >= 128 && tid < 128 + kBeta) {
      double v = s.rb[tid - 128];
      for (int c = 0; c < kY; ++c) v -= cur[(tid - 128) * kY + c] * cur[kBeta * kY + c];
      s.rb[tid - 128] = v;
    }
    for (int e = tid; e < kTriY; e += kSmThreads) {
      fc[fLd + e] = Q[e];
      fc[fL2 + e] = has2 ? s.U[e] : 0.0;
    }
    for (int e = tid; e < kY * kY; e += kSmThreads) fc[fL1 + e] = has1 ? s.E[e] : 0.0;
    for (int e = tid; e < kBZ; e += kSmThreads) fc[fLb + e] = cur[e];
    __syncthreads();
  }

  // the corner: Cholesky and both substitutions, serial
  if (tid == 0) {
    double* A = s.A;
    bool ok = true;
    for (int j = 0; j < kBeta && ok; ++j)
      for (int i = j; i < kBeta; ++i) {
        double v = A[i * kBeta + j];
        for (int k = 0; k < j; ++k) v -= A[i * kBeta + k] * A[j * kBeta + k];
        if (i == j) {
          if (!(v > 0.0)) {
            ok = false;
            break;
          }
          A[j * kBeta + j] = sqrt(v);
        } else {
          A[i * kBeta + j] = v / A[j * kBeta + j];
        }
      }
    if (ok) {
      double* d = s.db;
      for (int q = 0; q < kBeta; ++q) d[q] = s.rb[q];
      for (int j = 0; j < kBeta; ++j) {
        d[j] = d[j] / A[j * kBeta + j];
        for (int i = j + 1; i < kBeta; ++i) d[i] -= A[i * kBeta + j] * d[j];
      }
      for (int j = kBeta - 1; j >= 0; --j) {
        d[j] = d[j] / A[j * kBeta + j];
        for (int i = 0; i < j; ++i) d[i] -= A[j * kBeta + i] * d[j];
      }
    }
    s.ok = ok ? 1 : 0;
  }
  __syncthreads();
  if (!s.ok) return;

  // back substitution from the last frame: d_i = L_ii^-T (z_i - L_i+1,i^T d_i+1 - L_i+2,i^T d_i+2 - L_b,i^T d beta)
  for (int i = T - 1; i >= 0; --i) {
    const int f = ul[i];
    const double* fc = fac_of(t, f);
    double* fr = frame_of(t, f);
    double* dc = s.d[i % 3];
    const double* d1 = s.d[(i + 1) % 3];
    const double* d2 = s.d[(i + 2) % 3];
    double* L = s.P[0];
    for (int e = tid; e < kTriY; e += kSmThreads) L[e] = fc[fLd + e];
    {
      const bool on = row < kY;
      const int c = on ? row : 0;
      double p = 0.0;
      if (on && temporal && i + 1 < T) {
        const double* l1 = fac_of(t, ul[i + 1]) + fL1 + c * kY;
        for (int r = g; r < kY; r += 4) p += l1[r] * d1[r];
      }
      if (on && temporal && i + 2 < T) {
        const double* l2 = fac_of(t, ul[i + 2]) + fL2 + tri(c, 0);
        for (int r = g; r <= c; r += 4) p += l2[r] * d2[r];
      }
      p = sum4(p);
      if (on && g == 0) {
        double pb = 0.0;
        for (int q = 0; q < kBeta; ++q) pb += fc[fLb + q * kY + c] * s.db[q];
        dc[c] = (fc[fZ + c] - p) - pb;
      }
    }
    __syncthreads();
    if (tid < 64) {                                     // one wave: the lanes share the row's dot product, butterflies add it
      for (int c = kY - 1; c >= 0; --c) {
        double p = 0.0;
        for (int k = c + 1 + lane; k < kY; k += 64) p += L[tri(k, c)] * dc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
        if (lane == 0) dc[c] = (dc[c] - p) / L[tri(c, c)];
      }
    }
    __syncthreads();
    if (tid < kY) {
      const double d = dc[tid];
      fr[oZ + tid] = d;
      fr[oYt + tid] = fr[oY + tid] + d;
      s.big[tid] = fmax(s.big[tid], fabs(d));
    }
    __syncthreads();
  }
  if (tid == 0) {
    double big = 0.0;
    for (int c = 0; c < kY; ++c) big = fmax(big, s.big[c]);
    for (int q = 0; q < kBeta; ++q) {
      tk[tDBeta + q] = s.db[q];
      tk[tBetaT + q] = tk[tBeta + q] + s.db[q];
      big = fmax(big, fabs(s.db[q]));
    }
    tk[tBig] = big;
    ti[iOk] = 1;
  }
}

// the data cost and the joints of a frame at the trial point
__global__ __launch_bounds__(kFitThreads) void smooth_trial_kernel(FitArgs a, TrackArgs t) {
  __shared__ FitShared s;
  const int tid = threadIdx.x;
  double* wsb = scratch_of(t);
  for (int f = blockIdx.x; f < t.N; f += gridDim.x) {
    if (!t.usable[f]) continue;
    const int trk = t.track[f];
    const int* ti = t.ti + (size_t)trk * kTrackI;
    if (ti[iDone] || !ti[iOk]) continue;
    double* fr = frame_of(t, f);
    fit_stage(s, a, f);
    if (tid < kY) s.x[1][tid] = fr[oYt + tid];
    else if (tid < kN) s.x[1][tid] = t.tk[(size_t)trk * kTrackD + tBetaT + tid - kY];
    __syncthreads();
    const double Ct = fit_evaluate(s, a, wsb, 1, 1);
    if (tid >= 128 && tid < 128 + kRows) fr[oJt + tid - 128] = s.Y[1][tid - 128];
    if (tid == 255) fr[oC + 2] = Ct;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void smooth_decide_kernel(TrackArgs t, SmW w, int max_iters) {
  __shared__ double part[kY];
  __shared__ int accept;
  const int trk = blockIdx.x, tid = threadIdx.x;
  int* ti = t.ti + (size_t)trk * kTrackI;
  if (ti[iDone]) return;
  double* tk = t.tk + (size_t)trk * kTrackD;
  const int* ul = ulist_of(t, ti);
  const int T = ti[iUsable];
  const bool stepped = ti[iOk] != 0;
  const double Cp = (stepped && T >= 3 && w.rot + w.trans > 0.0) ? sm_prior_cost(t, ul, T, w, oYt, part) : 0.0;
  if (tid == 0) {
    bool acc = false;
    double Ct = 0.0;
    if (stepped) {
      for (int k = 0; k < T; ++k) Ct += frame_of(t, ul[k])[oC + 2];
      Ct += Cp;
      acc = fabs(Ct) < INFINITY && Ct < tk[tC];         // NaN never passes
    }
    accept = acc ? 1 : 0;
    const int it = ti[iTrials] + 1;
    ti[iTrials] = it;
    int done = 0;
    if (acc) {
      tk[tC] = Ct;
      tk[tLambda] *= 0.1;
      if (tk[tBig] < XAS_SMPLFIT_STEP_TOL) {
        ti[iStatus] = kStConverged;
        done = 1;
      }
    } else {
      tk[tLambda] *= 10.0;
      if (tk[tLambda] > 1e12) done = 1;
    }
    if (it >= max_iters) done = 1;
    ti[iDone] = done;
    ti[iRelin] = acc ? 1 : 0;
  }
  __syncthreads();
  if (!accept) return;
  if (tid < kBeta) tk[tBeta + tid] = tk[tBetaT + tid];
  for (int k = 0; k < T; ++k) {
    double* fr = frame_of(t, ul[k]);
    if (tid < kY) fr[oY + tid] = fr[oYt + tid];
    else if (tid >= 128 && tid < 128 + kRows) fr[oJ + tid - 128] = fr[oJt + tid - 128];
    else if (tid == 255) fr[oC + 1] = fr[oC + 2];
  }
}

struct SmExport {
  double *hdiag, *hoff, *corner, *border, *g_y, *g_beta, *d_y, *d_beta, *cost;
};

// What one trial at the given lambda left.  A block per sample, then a block per track.
__global__ __launch_bounds__(256) void smooth_export_kernel(TrackArgs t, SmExport o) {
  const int tid = threadIdx.x;
  for (int b = blockIdx.x; b < t.N + t.S; b += gridDim.x) {
    if (b < t.N) {
      const int f = b, trk = t.track[f];
      const bool in = (unsigned)trk < (unsigned)t.S && t.usable[f];
      const int* ti = t.ti + (size_t)(in ? trk : 0) * kTrackI;
      const bool on = in && ti[iFramesOk], step = in && ti[iOk];
      const double* fr = frame_of(t, f);
      const double* fc = fac_of(t, f);
      const double lambda = in ? t.tk[(size_t)trk * kTrackD + tLambda] : 0.0;
      for (int e = tid; e < kY * kY; e += 256) {
        const int r = e / kY, c = e % kY;
        double v = 0.0;
        if (on) {
          v = fr[oH + (r >= c ? tri(r, c) : tri(c, r))];
          if (r == c) {
            v += fc[fTd + c];
            v += lambda * v;
          }
        }
        o.hdiag[(size_t)f * kY * kY + e] = v;
      }
      for (int e = tid; e < kBeta * kY; e += 256) o.border[(size_t)f * kBeta * kY + e] = on ? fr[oH + tri(kY + e / kY, e % kY)] : 0.0;
      if (tid < kY) {
        o.g_y[(size_t)f * kY + tid] = on ? fc[fG + tid] : 0.0;
        o.d_y[(size_t)f * kY + tid] = step ? fr[oZ + tid] : 0.0;
      } else if (tid >= 128 && tid < 130) {
        o.hoff[(size_t)f * 2 + tid - 128] = on ? fc[fOff + tid - 128] : 0.0;
      }
    } else {
      const int trk = b - t.N;
      const int* ti = t.ti + (size_t)trk * kTrackI;
      const double* tk = t.tk + (size_t)trk * kTrackD;
      const bool on = ti[iUsable] > 0 && ti[iFramesOk];
      if (tid < 100) {
        const int i = tid / 10, j = tid % 10;
        o.corner[(size_t)trk * 100 + tid] = on ? tk[tA + (i >= j ? tri(i, j) : tri(j, i))] : 0.0;
      } else if (tid < 110) {
        o.g_beta[(size_t)trk * 10 + tid - 100] = on ? tk[tRhs + tid - 100] : 0.0;
      } else if (tid < 120) {
        o.d_beta[(size_t)trk * 10 + tid - 110] = ti[iUsable] > 0 && ti[iOk] ? tk[tDBeta + tid - 110] : 0.0;
      } else if (tid == 120) {
        o.cost[trk] = tk[tC0];
      }
    }
  }
}

size_t smooth_workspace_bytes(int N, int V, int S) {
  return tracks_workspace_bytes(N, V, S) + align16((size_t)N * kFacD * sizeof(double));
}

int smooth_check(const char* who, double rot_w, double trans_w) {
  XAS_REQUIRE(rot_w >= 0.0 && rot_w < INFINITY && trans_w >= 0.0 && trans_w < INFINITY,
              "%s: weights %g, %g (need finite weights >= 0)", who, rot_w, trans_w);
  return 0;
}

}  // namespace
}  // namespace xas

using namespace xas;

extern "C" size_t xas_smpl_fit_tracks_smooth_workspace_bytes(int N, int V, int S) {
  if (N < 0 || V < 1 || S < 0) return 0;
  return smooth_workspace_bytes(N, V, S);
}

#define XAS_SMOOTH_ARGS()                                                                                                      \
  XAS_TRACKS_ARGS();                                                                                                           \
  t.smooth = rot_w + trans_w > 0.0 ? 1 : 0;                                                                                    \
  t.fac = reinterpret_cast<double*>(static_cast<char*>(workspace) + tracks_workspace_bytes(N, V, S));                          \
  SmW w;                                                                                                                       \
  w.rot = rot_w; w.trans = trans_w

// the launches up to the start of the first trial (S >= 1, N >= 1)
#define XAS_SMOOTH_START(pose_o, trans_o, joints_o, cost_o, status_o, betas_o, lambda0, iters)                                 \
  XAS_TRACKS_JOINT_TERMS();                                                                                                    \
  hipLaunchKernelGGL(tracks_init_frames_kernel, fgrid, dim3(kFitThreads), 0, st, a, t, pose_o, trans_o, joints_o, cost_o,      \
                     status_o);                                                                                                \
  XAS_LAUNCH_CHECK();                                                                                                          \
  XAS_SMOOTH_START_TRACKS(betas_o, lambda0, iters, 1)

// the track kernels of the start; frames = 0: the tracks have no sample and no frame kernel runs
#define XAS_SMOOTH_START_TRACKS(betas_o, lambda0, iters, frames)                                                               \
  hipLaunchKernelGGL(tracks_count_kernel, tgrid, dim3(256), 0, st, t);                                                         \
  XAS_LAUNCH_CHECK();                                                                                                          \
  hipLaunchKernelGGL(tracks_list_kernel, tgrid, dim3(256), 0, st, t, betas, betas_o);                                          \
  XAS_LAUNCH_CHECK();                                                                                                          \
  hipLaunchKernelGGL(smooth_setup_kernel, tgrid, dim3(64), 0, st, t, rot_w > 0.0 ? 1 : 0);                                     \
  XAS_LAUNCH_CHECK();                                                                                                          \
  if (frames) {                                                                                                                \
    hipLaunchKernelGGL(tracks_start_frames_kernel, fgrid, dim3(kFitThreads), 0, st, a, t);                                     \
    XAS_LAUNCH_CHECK();                                                                                                        \
  }                                                                                                                            \
  hipLaunchKernelGGL(smooth_start_kernel, tgrid, dim3(128), 0, st, t, w, lambda0, iters);                                      \
  XAS_LAUNCH_CHECK()

#define XAS_SMOOTH_TRIAL()                                                                                                     \
  hipLaunchKernelGGL(smooth_assemble_kernel, fgrid, dim3(kFitThreads), 0, st, a, t);                                           \
  XAS_LAUNCH_CHECK();                                                                                                          \
  hipLaunchKernelGGL(smooth_solve_kernel, tgrid, dim3(kSmThreads), 0, st, t, w);                                               \
  XAS_LAUNCH_CHECK();                                                                                                          \
  hipLaunchKernelGGL(smooth_trial_kernel, fgrid, dim3(kFitThreads), 0, st, a, t);                                              \
  XAS_LAUNCH_CHECK()

extern "C" int xas_smpl_fit_tracks_smooth_linearise(
    const float* pose, const float* betas, const float* trans, const float* v_template, const float* shapedirs,
    const float* posedirs, const float* j_regressor, const float* weights, const int* parents, const float* h36m_regressor,
    const int* reg_verts, const int* reg_count, const float* targets, const float* joint_w, const int* track, const int* frame,
    float pose_prior, float shape_prior, double rot_w, double trans_w, int N, int V, int S, int center_idx, double lambda,
    double* hdiag, double* hoff, double* corner, double* border, double* g_y, double* g_beta, double* d_y, double* d_beta,
    double* track_cost, void* workspace, void* stream) {
  if (fit_check("smpl_fit_tracks_smooth_linearise", pose, betas, trans, v_template, shapedirs, posedirs, j_regressor, weights,
                parents, h36m_regressor, reg_verts, reg_count, targets, joint_w, pose_prior, shape_prior, N, V, center_idx, workspace))
    return 1;
  if (tracks_check("smpl_fit_tracks_smooth_linearise", track, frame, N, S)) return 1;
  if (smooth_check("smpl_fit_tracks_smooth_linearise", rot_w, trans_w)) return 1;
  XAS_REQUIRE(lambda >= 0.0 && lambda < INFINITY, "smpl_fit_tracks_smooth_linearise: lambda=%g (needs a finite damping >= 0)", lambda);
  if (N == 0 && S == 0) return 0;
  XAS_REQUIRE((N == 0 || (hdiag && hoff && border && g_y && d_y)) && (S == 0 || (corner && g_beta && d_beta && track_cost)),
              "smpl_fit_tracks_smooth_linearise: null output (the blocks, the off-diagonal scalars, the border, the corner, the "
              "right-hand sides, the steps and the cost are required)");
  XAS_REQUIRE(workspace, "smpl_fit_tracks_smooth_linearise: null buffer (the workspace is required)");
  if (N > 0 && tracks_check_ids("smpl_fit_tracks_smooth_linearise", track, N, S)) return 1;
  XAS_SMOOTH_ARGS();
  if (N > 0 && S > 0) {
    XAS_SMOOTH_START((double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, (unsigned char*)nullptr,
                     (double*)nullptr, lambda, 1);
    XAS_SMOOTH_TRIAL();
  } else if (S > 0) {                                   // tracks without a sample: the model arrays are not read
    XAS_SMOOTH_START_TRACKS((double*)nullptr, lambda, 1, 0);
  } else {                                              // samples without a track: every one is passed through
    const size_t n = (size_t)N * sizeof(double);
    XAS_REQUIRE(hipMemsetAsync(hdiag, 0, n * kY * kY, st) == hipSuccess && hipMemsetAsync(hoff, 0, n * 2, st) == hipSuccess &&
                    hipMemsetAsync(border, 0, n * kBeta * kY, st) == hipSuccess && hipMemsetAsync(g_y, 0, n * kY, st) == hipSuccess &&
                    hipMemsetAsync(d_y, 0, n * kY, st) == hipSuccess,
                "smpl_fit_tracks_smooth_linearise: memset failed");
    return 0;
  }
  SmExport o;
  o.hdiag = hdiag; o.hoff = hoff; o.corner = corner; o.border = border; o.g_y = g_y; o.g_beta = g_beta; o.d_y = d_y;
  o.d_beta = d_beta; o.cost = track_cost;
  hipLaunchKernelGGL(smooth_export_kernel, dim3(ew_grid((long)N + S, 1)), dim3(256), 0, st, t, o);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_smpl_fit_tracks_smooth(
    const float* pose, const float* betas, const float* trans, const float* v_template, const float* shapedirs,
    const float* posedirs, const float* j_regressor, const float* weights, const int* parents, const float* h36m_regressor,
    const int* reg_verts, const int* reg_count, const float* targets, const float* joint_w, const int* track, const int* frame,
    float pose_prior, float shape_prior, double rot_w, double trans_w, int N, int V, int S, int center_idx, int max_iters,
    double* pose_out, double* trans_out, double* joints_out, double* frame_cost, unsigned char* frame_status, double* track_betas,
    double* track_cost, int* track_trials, unsigned char* track_status, void* workspace, void* stream) {
  if (fit_check("smpl_fit_tracks_smooth", pose, betas, trans, v_template, shapedirs, posedirs, j_regressor, weights, parents,
                h36m_regressor, reg_verts, reg_count, targets, joint_w, pose_prior, shape_prior, N, V, center_idx, workspace))
    return 1;
  if (tracks_check("smpl_fit_tracks_smooth", track, frame, N, S)) return 1;
  if (smooth_check("smpl_fit_tracks_smooth", rot_w, trans_w)) return 1;
  XAS_REQUIRE(max_iters >= 0 && max_iters <= XAS_SMPLFIT_MAX_ITERS,
              "smpl_fit_tracks_smooth: max_iters=%d trials (needs 0 <= max_iters <= %d)", max_iters, XAS_SMPLFIT_MAX_ITERS);
  if (N == 0 && S == 0) return 0;
  XAS_REQUIRE((N == 0 || (pose_out && trans_out && joints_out && frame_cost && frame_status)) &&
                  (S == 0 || (track_betas && track_cost && track_trials && track_status)),
              "smpl_fit_tracks_smooth: null output (pose, trans, joints, frame cost and status, track betas, cost, trials and status "
              "are required)");
  XAS_REQUIRE(workspace, "smpl_fit_tracks_smooth: null buffer (the workspace is required)");
  if (N > 0 && tracks_check_ids("smpl_fit_tracks_smooth", track, N, S)) return 1;
  XAS_SMOOTH_ARGS();
  if (N > 0 && S > 0) {
    XAS_SMOOTH_START(pose_out, trans_out, joints_out, frame_cost, frame_status, track_betas, 1e-3, max_iters);
    for (int it = 0; it < max_iters; ++it) {
      XAS_SMOOTH_TRIAL();
      hipLaunchKernelGGL(smooth_decide_kernel, tgrid, dim3(256), 0, st, t, w, max_iters);
      XAS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tracks_finish_frames_kernel, dim3(ew_grid(N, 1)), dim3(128), 0, st, t, pose_out, trans_out, joints_out,
                       frame_cost, frame_status);
    XAS_LAUNCH_CHECK();
  } else if (S > 0) {
    XAS_SMOOTH_START_TRACKS(track_betas, 1e-3, max_iters, 0);
  } else {                                              // S == 0: every sample is passed through
    XAS_TRACKS_JOINT_TERMS();
    hipLaunchKernelGGL(tracks_init_frames_kernel, fgrid, dim3(kFitThreads), 0, st, a, t, pose_out, trans_out, joints_out,
                       frame_cost, frame_status);
    XAS_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(tracks_finish_kernel, tgrid, dim3(64), 0, st, t, track_betas, track_cost, track_trials, track_status);
  XAS_LAUNCH_CHECK();
  return 0;
}
