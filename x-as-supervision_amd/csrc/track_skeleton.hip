// Temporal smoothing of whole skeletons (gfx950; eval.py --smooth --smooth-bones, no reference counterpart): the problem of
// xas_track_anchor_smooth for every joint of a track at once, coupled in every frame by the lengths of the bones.
// include/xas_hip.h states the problem; track_band.h has the stencil and the argument checks, track_anchor.h the data term of
// a frame.  This file is the solver, the kernel and its entry points.
// One workgroup of 256 threads per track, one launch.  Unknown 3K t + 3k + c: the matrix is block-pentadiagonal with blocks of
// side n = 3K <= 72, H_tt dense (data, prior and bones), H_t,t-1 = b1 P and H_t,t-2 = b2 P with P the 0/1 diagonal of the free
// joints.  A fixed joint keeps its rows as identity rows with a zero right-hand side: nothing else feels them.
// Three blocks of 73 x 73 doubles sit in LDS (125 KB).  At frame t of the factorisation:
//   C = L_t,t-2, read back from the workspace (frame t-2 wrote it: it is b2 P L_t-2,t-2^-T)
//   B = L_t-1,t-2, replaced by W = b1 P - C B^T (through registers), then by L_t,t-1 = W L_t-1,t-1^-T (A still holds L_t-1,t-1)
//   A = H_tt + lambda diag H_tt - B B^T - C C^T, then its Cholesky factor L_tt in place (right-looking, two barriers a column)
// Row n of each block is the right-hand side's: y_t-1 in B, y_t-2 in C, -g_t in A, so the factorisation of A leaves y_t = the
// forward substitution in its row n with no step of its own.  L_tt, L_t,t-1 and L_t+2,t go to the workspace, as do g, y / d, X
// and the trial point: T is bounded by N alone.  The back substitution walks the frames down with L_tt in LDS.
// Every sum runs in one fixed order (per thread ascending, then a butterfly over the wave, then the four waves in order), every
// loop is bounded by T, n, Bn or max_iter, and every value a barrier sits under is read from LDS by all threads alike.
#include "track_anchor.h"

namespace xas {

constexpr int kSkN = 3 * XAS_SKEL_MAX_JOINTS, kSkLd = kSkN + 1, kSkThreads = 256;
constexpr int kSkPerThread = (kSkN * kSkN + kSkThreads - 1) / kSkThreads;
constexpr double kSkShort = 1e-9;                                     // a bone shorter than this (mm) has a zero Jacobian row

// The record of a track in the workspace: per array, its offset in units of T doubles.
//   X [2][T][n]  D [2][T][K][6]  G [2][T][n]  R2 [2][T][K]  A [T][3]  Y [T][n] (y, then d)  USED [T][K] (ints)  L [T][3][n][n]
struct SkLayout {
  int X, D, G, R2, A, Y, U, L, rec;
};
__host__ __device__ __forceinline__ SkLayout sk_layout(int K) {
  const int n = 3 * K;
  SkLayout l;
  l.X = 0; l.D = 2 * n; l.G = 6 * n; l.R2 = 8 * n; l.A = 8 * n + 2 * K; l.Y = l.A + 3; l.U = l.Y + n; l.L = l.U + K;
  l.rec = l.L + 3 * n * n;
  return l;
}

struct SkBones {
  int j[XAS_TRACK_MAX_BONES][2];
};
struct SkArgs {
  TsArgs a;
  TsAnchored data;
  const float* length;                                                // [S][Bn]
  int Bn;
  double bone_w;
  SkBones bones;
};
struct SkOut {
  float *out, *resid, *bone;                                          // smooth
  unsigned char *status, *track_status;
  double* cost;
  int* trials;
  double *g, *hdiag, *hoff, *d, *C, lambda;                           // linearise
};

struct SkShared {
  double A[kSkLd][kSkLd], B[kSkLd][kSkLd], C[kSkLd][kSkLd];
  double y1[kSkN], y2[kSkN], r[kSkN], dc[kSkN];
  double U[XAS_TRACK_MAX_BONES][3], len[XAS_TRACK_MAX_BONES], red[4];
  int ja[XAS_TRACK_MAX_BONES], jb[XAS_TRACK_MAX_BONES], act[XAS_TRACK_MAX_BONES], free[XAS_SKEL_MAX_JOINTS];
};

// A track's state: where its arrays lie, and what every step needs of the arguments.
struct SkTrack {
  const SkArgs& p;
  SkShared& s;
  int n0, T, K, n, Bn, tid;
  double *w;
  SkLayout l;
  const int* fr;
  __device__ __forceinline__ double* X(int src) const { return w + (size_t)(l.X + n * src) * T; }
  __device__ __forceinline__ double* D(int src) const { return w + (size_t)(l.D + 6 * K * src) * T; }
  __device__ __forceinline__ double* G(int src) const { return w + (size_t)(l.G + n * src) * T; }
  __device__ __forceinline__ double* R2(int src) const { return w + (size_t)(l.R2 + K * src) * T; }
  __device__ __forceinline__ double* A() const { return w + (size_t)l.A * T; }
  __device__ __forceinline__ double* Y() const { return w + (size_t)l.Y * T; }
  __device__ __forceinline__ int* used() const { return (int*)(w + (size_t)l.U * T); }
  __device__ __forceinline__ double* L(int t, int which) const { return w + (size_t)l.L * T + ((size_t)t * 3 + which) * n * n; }
};

// Sum and maximum over the workgroup, the same on every thread.
__device__ __forceinline__ double sk_sum(SkShared& s, double v, int tid) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((tid & 63) == 0) s.red[tid >> 6] = v;
  __syncthreads();
  return ((s.red[0] + s.red[1]) + s.red[2]) + s.red[3];
}
__device__ __forceinline__ double sk_max(SkShared& s, double v, int tid) {
  v = wave_max_d(v);
  __syncthreads();
  if ((tid & 63) == 0) s.red[tid >> 6] = v;
  __syncthreads();
  return fmax(fmax(s.red[0], s.red[1]), fmax(s.red[2], s.red[3]));
}

// Bone b at frame t of X: its residual e = |d| - length, and u = d / |d| (0 where |d| < kSkShort: the row is zero).
__device__ __forceinline__ double sk_bone(const SkTrack& k, const double* X, int t, int b, double (&u)[3]) {
  const double* xi = X + (size_t)t * k.n + 3 * k.s.ja[b];
  const double* xj = X + (size_t)t * k.n + 3 * k.s.jb[b];
  const double d[3] = {xi[0] - xj[0], xi[1] - xj[1], xi[2] - xj[2]};
  const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const bool row = len >= kSkShort;
#pragma unroll
  for (int m = 0; m < 3; ++m) u[m] = row ? d[m] / len : 0.0;
  return len - k.s.len[b];
}

// Cost, data blocks and gradients of every frame and free joint at X[src] -> D[src], G[src], R2[src]; C = the track's cost,
// bad = a data frame lies behind a view it uses.  Starts with a barrier (X[src] was just written) and ends past one.
static __device__ void sk_eval(const SkTrack& k, int src, double& C, bool& bad) {
  __syncthreads();
  const TsArgs& a = k.p.a;
  const double* X = k.X(src);
  double *D = k.D(src), *G = k.G(src), *R2 = k.R2(src);
  const int* usedw = k.used();
  const int T = k.T, K = k.K, n = k.n;
  double Cd = 0.0, Cp = 0.0, Cb = 0.0;
  int behind = 0;
  for (int idx = k.tid; idx < T * K; idx += kSkThreads) {
    const int t = idx / K, j = idx - t * K;
    PointFit f;
    f.clear();
    double gp[3] = {0.0, 0.0, 0.0}, gb[3] = {0.0, 0.0, 0.0}, cp = 0.0;
    if (k.s.free[j]) {
      for (int s = t - 1; s <= t + 1; ++s) {
        if (s < 1 || s > T - 2) continue;
        const TsStencil c = ts_stencil(k.fr, s);
        const double ct = c.at(s, t);
        double qq = 0.0;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const double xm = X[(size_t)(s - 1) * n + 3 * j + m], x0 = X[(size_t)s * n + 3 * j + m], xp = X[(size_t)(s + 1) * n + 3 * j + m];
          const double q = c.cp * (xp - x0) - c.cm * (x0 - xm);
          gp[m] += c.ws * ct * q;
          qq += q * q;
        }
        if (s == t) cp = c.ws * qq;
      }
      const int used = usedw[idx];
      if (used) {
        const double Xt[3] = {X[(size_t)t * n + 3 * j], X[(size_t)t * n + 3 * j + 1], X[(size_t)t * n + 3 * j + 2]};
        if (!k.p.data.fit(a, k.n0 + t, j, used, Xt, f)) behind = 1;
      }
      for (int b = 0; b < k.Bn; ++b) {                                // the bones at this joint, in ascending order
        if (!k.s.act[b] || (k.s.ja[b] != j && k.s.jb[b] != j)) continue;
        double u[3];
        const double e = sk_bone(k, X, t, b, u), sign = k.s.ja[b] == j ? 1.0 : -1.0;
#pragma unroll
        for (int m = 0; m < 3; ++m) gb[m] += sign * u[m] * e;
      }
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) D[(size_t)idx * 6 + m] = f.H[m];
#pragma unroll
    for (int m = 0; m < 3; ++m) G[(size_t)t * n + 3 * j + m] = f.g[m] + a.acc_w * gp[m] + k.p.bone_w * gb[m];
    R2[idx] = f.r2;
    Cd += f.C; Cp += cp;
  }
  for (int idx = k.tid; idx < T * k.Bn; idx += kSkThreads) {
    const int t = idx / k.Bn, b = idx - t * k.Bn;
    if (!k.s.act[b]) continue;
    double u[3];
    const double e = sk_bone(k, X, t, b, u);
    Cb += e * e;
  }
  const double sd = sk_sum(k.s, Cd, k.tid), sp = sk_sum(k.s, Cp, k.tid), sb = sk_sum(k.s, Cb, k.tid);
  C = sd + a.acc_w * sp + k.p.bone_w * sb;
  bad = __syncthreads_or(behind) != 0;
}

// Entry (r, c), c <= r, of the symmetric 3x3 stored as its upper triangle 00 01 02 11 12 22.
__device__ __forceinline__ int sk_sym(int r, int c) { return c == 0 ? r : (c == 1 ? 2 + r : 5); }

// The lower triangle of H_tt (without lambda) at X[src] -> s.A, rows 0 .. n-1; -g_t -> its row n.  A fixed joint has an
// identity block and a zero right-hand side.  Starts with a barrier and ends past one.
static __device__ void sk_assemble(const SkTrack& k, int src, int t) {
  __syncthreads();
  const int n = k.n, K = k.K;
  const double* D = k.D(src) + (size_t)t * K * 6;
  const double* G = k.G(src) + (size_t)t * n;
  const double b0 = k.p.a.acc_w * k.A()[3 * t];
  if (k.tid < k.Bn) {
    double u[3] = {0.0, 0.0, 0.0};
    if (k.s.act[k.tid]) sk_bone(k, k.X(src), t, k.tid, u);
    k.s.U[k.tid][0] = u[0]; k.s.U[k.tid][1] = u[1]; k.s.U[k.tid][2] = u[2];
  }
  for (int idx = k.tid; idx < n * n; idx += kSkThreads) {
    const int i = idx / n, j = idx - i * n;
    if (j > i) continue;
    const int ki = i / 3, kj = j / 3, ci = i - 3 * ki, cj = j - 3 * kj;
    double v = 0.0;
    if (ki == kj) v = k.s.free[ki] ? D[ki * 6 + sk_sym(ci, cj)] + (i == j ? b0 : 0.0) : (i == j ? 1.0 : 0.0);
    k.s.A[i][j] = v;
  }
  if (k.tid < n) k.s.A[n][k.tid] = k.s.free[k.tid / 3] ? -G[k.tid] : 0.0;
  __syncthreads();
  if (k.tid < 9 * K) {                                                // bone_w J^T J: thread (joint, c, c2) owns its entries
    const int j = k.tid / 9, c = (k.tid - 9 * j) / 3, c2 = k.tid % 3;
    for (int b = 0; b < k.Bn; ++b) {
      if (!k.s.act[b] || (k.s.ja[b] != j && k.s.jb[b] != j)) continue;
      const int o = k.s.ja[b] == j ? k.s.jb[b] : k.s.ja[b];
      const double uu = k.p.bone_w * k.s.U[b][c] * k.s.U[b][c2];
      if (c2 <= c) k.s.A[3 * j + c][3 * j + c2] += uu;
      if (o < j) k.s.A[3 * j + c][3 * o + c2] -= uu;
    }
  }
  __syncthreads();
}

// Block Cholesky of H + lambda diag H at X[cur] with the forward substitution L y = -g in the same sweep -> false at a pivot
// that is not > 0 (NaN fails too); the same on every thread.  L_tt, L_t,t-1, L_t,t-2 and y go to the workspace.
static __device__ bool sk_factor(const SkTrack& k, int cur, double lambda) {
  SkShared& s = k.s;
  const int n = k.n, T = k.T, tid = k.tid;
  const double* Ap = k.A();
  __syncthreads();
  if (tid < n) { s.y1[tid] = 0.0; s.y2[tid] = 0.0; }
  for (int t = 0; t < T; ++t) {
    const double b1 = k.p.a.acc_w * Ap[3 * t + 1];
    __syncthreads();
    const double* E2 = k.L(t, 2);
    for (int idx = tid; idx < n * n; idx += kSkThreads) {
      const int i = idx / n, j = idx - i * n;
      s.C[i][j] = t >= 2 ? E2[idx] : 0.0;
      if (t == 0) s.B[i][j] = 0.0;
    }
    if (t > 0) {
      __syncthreads();
      double acc[kSkPerThread];                                       // W = b1 P - L_t,t-2 L_t-1,t-2^T
#pragma unroll
      for (int q = 0; q < kSkPerThread; ++q) {
        const int idx = tid + q * kSkThreads;
        acc[q] = 0.0;
        if (idx < n * n) {
          const int i = idx / n, j = idx - i * n;
          double v = i == j && s.free[i / 3] ? b1 : 0.0;
          for (int m = 0; m < n; ++m) v -= s.C[i][m] * s.B[j][m];
          acc[q] = v;
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kSkPerThread; ++q) {
        const int idx = tid + q * kSkThreads;
        if (idx < n * n) s.B[idx / n][idx % n] = acc[q];
      }
      __syncthreads();
      if (tid < n) {                                                  // L_t,t-1 = W L_t-1,t-1^-T, a row per thread
        for (int j = 0; j < n; ++j) {
          double v = s.B[tid][j];
          for (int m = 0; m < j; ++m) v -= s.B[tid][m] * s.A[j][m];
          s.B[tid][j] = v / s.A[j][j];
        }
      }
    }
    if (tid < n) { s.B[n][tid] = s.y1[tid]; s.C[n][tid] = s.y2[tid]; }
    sk_assemble(k, cur, t);
    for (int idx = tid; idx < (n + 1) * n; idx += kSkThreads) {
      const int i = idx / n, j = idx - i * n;
      if (j > i) continue;
      double v = s.A[i][j];
      if (i == j) v *= 1.0 + lambda;
      for (int m = 0; m < n; ++m) v -= s.B[i][m] * s.B[j][m] + s.C[i][m] * s.C[j][m];
      s.A[i][j] = v;
    }
    for (int j = 0; j < n; ++j) {                                     // Cholesky in place; the diagonal is rooted afterwards
      __syncthreads();
      const double piv = s.A[j][j];
      if (!(piv > 0.0)) return false;
      const double root = sqrt(piv);
      if (tid < n - j) s.A[j + 1 + tid][j] /= root;
      __syncthreads();
      const int wd = n - 1 - j;
      for (int idx = tid; idx < (n - j) * wd; idx += kSkThreads) {
        const int i = j + 1 + idx / wd, c = j + 1 + idx % wd;
        if (c <= i) s.A[i][c] -= s.A[i][j] * s.A[c][j];
      }
    }
    __syncthreads();
    if (tid < n) s.A[tid][tid] = sqrt(s.A[tid][tid]);
    __syncthreads();
    double *L0 = k.L(t, 0), *L1 = k.L(t, 1);
    for (int idx = tid; idx < n * n; idx += kSkThreads) {
      const int i = idx / n, j = idx - i * n;
      L0[idx] = j <= i ? s.A[i][j] : 0.0;
      L1[idx] = s.B[i][j];
    }
    if (tid < n) {
      const double y = s.A[n][tid];
      k.Y()[(size_t)t * n + tid] = y;
      s.y2[tid] = s.y1[tid]; s.y1[tid] = y;
      if (t + 2 < T) {                                                // L_t+2,t = b2 P L_tt^-T, a row per thread, into C
        const double b2 = k.p.a.acc_w * Ap[3 * (t + 2) + 2];
        const bool fr = s.free[tid / 3] != 0;
        for (int j = 0; j < n; ++j) {
          double v = j == tid && fr ? b2 : 0.0;
          if (fr)
            for (int m = tid; m < j; ++m) v -= s.C[tid][m] * s.A[j][m];
          s.C[tid][j] = j >= tid && fr ? v / s.A[j][j] : 0.0;
        }
      }
    }
    if (t + 2 < T) {
      __syncthreads();
      double* N2 = k.L(t + 2, 2);
      for (int idx = tid; idx < n * n; idx += kSkThreads) N2[idx] = s.C[idx / n][idx % n];
    }
  }
  return true;
}

// L^T d = y, from the last frame down: d_t = L_tt^-T (y_t - L_t+1,t^T d_t+1 - L_t+2,t^T d_t+2).  d replaces y in Y.
static __device__ void sk_back(const SkTrack& k) {
  SkShared& s = k.s;
  const int n = k.n, T = k.T, tid = k.tid;
  double* Y = k.Y();
  __syncthreads();
  if (tid < n) { s.y1[tid] = 0.0; s.y2[tid] = 0.0; }                  // d_t+1 and d_t+2
  for (int t = T - 1; t >= 0; --t) {
    __syncthreads();
    const double* L0 = k.L(t, 0);
    for (int idx = tid; idx < n * n; idx += kSkThreads) s.A[idx / n][idx % n] = L0[idx];
    if (tid < n) {
      double v = Y[(size_t)t * n + tid];
      if (t + 1 < T) {
        const double* E = k.L(t + 1, 1);
        for (int i = 0; i < n; ++i) v -= E[i * n + tid] * s.y1[i];
      }
      if (t + 2 < T) {
        const double* E = k.L(t + 2, 2);
        for (int i = 0; i < n; ++i) v -= E[i * n + tid] * s.y2[i];
      }
      s.r[tid] = v;
    }
    for (int i = n - 1; i >= 0; --i) {
      __syncthreads();
      const double di = s.r[i] / s.A[i][i];
      if (tid < i) s.r[tid] -= s.A[i][tid] * di;
      if (tid == i) s.dc[i] = di;
    }
    __syncthreads();
    if (tid < n) {
      const double d = s.dc[tid];
      Y[(size_t)t * n + tid] = d;
      s.y2[tid] = s.y1[tid]; s.y1[tid] = d;
    }
  }
  __syncthreads();
}

enum { SK_SMOOTH, SK_LINEARISE };

__global__ __launch_bounds__(kSkThreads) void track_skeleton_kernel(SkArgs p, SkOut o, int mode) {
  __shared__ SkShared s;
  const TsArgs& a = p.a;
  const int sidx = blockIdx.x, tid = threadIdx.x, K = a.K, n = 3 * K, Bn = p.Bn;
  const int n0 = a.start[sidx], T = a.start[sidx + 1] - n0;
  const SkLayout l = sk_layout(K);
  SkTrack k = {p, s, n0, T, K, n, Bn, tid, a.ws + (size_t)n0 * l.rec, l, a.frame + n0};
  int* usedw = k.used();
  double* X0 = k.X(0);

  // which frames of which joints have data, and their start
  for (int idx = tid; idx < T * K; idx += kSkThreads) {
    const int t = idx / K, j = idx - t * K;
    double X[3];
    usedw[idx] = p.data.classify(a, n0 + t, j, X);
    X0[(size_t)t * n + 3 * j] = X[0]; X0[(size_t)t * n + 3 * j + 1] = X[1]; X0[(size_t)t * n + 3 * j + 2] = X[2];
  }
  __syncthreads();
  if (tid < K) {                                                      // free: at least two data frames
    int cnt = 0;
    for (int t = 0; t < T && cnt < 2; ++t) cnt += usedw[t * K + tid] ? 1 : 0;
    s.free[tid] = cnt >= 2;
  }
  __syncthreads();
  if (tid < Bn) {
    const int ja = p.bones.j[tid][0], jb = p.bones.j[tid][1];
    const double len = (double)p.length[(size_t)sidx * Bn + tid];
    s.ja[tid] = ja; s.jb[tid] = jb; s.len[tid] = len;
    s.act[tid] = s.free[ja] && s.free[jb] && len > 0.0 && len < INFINITY;
  }
  int nfree = 0;
  for (int j = 0; j < K; ++j) nfree += s.free[j];
  // gap frames: between data frames the line through them in `frame`, beyond the ends the nearest data frame's point
  for (int idx = tid; idx < T * K; idx += kSkThreads) {
    const int t = idx / K, j = idx - t * K;
    if (!s.free[j] || usedw[idx]) continue;
    int lt = t - 1, rt = t + 1;
    while (lt >= 0 && !usedw[lt * K + j]) --lt;
    while (rt < T && !usedw[rt * K + j]) ++rt;
    double X[3];
    if (lt >= 0 && rt < T) {
      const double f = ((double)k.fr[t] - (double)k.fr[lt]) / ((double)k.fr[rt] - (double)k.fr[lt]);
#pragma unroll
      for (int m = 0; m < 3; ++m) X[m] = X0[(size_t)lt * n + 3 * j + m] + (X0[(size_t)rt * n + 3 * j + m] - X0[(size_t)lt * n + 3 * j + m]) * f;
    } else {
      const int e = lt >= 0 ? lt : rt;
#pragma unroll
      for (int m = 0; m < 3; ++m) X[m] = X0[(size_t)e * n + 3 * j + m];
    }
    X0[(size_t)t * n + 3 * j] = X[0]; X0[(size_t)t * n + 3 * j + 1] = X[1]; X0[(size_t)t * n + 3 * j + 2] = X[2];
  }
  // the prior's matrix: row t sums the stencils that cover t, in ascending order
  double* Ap = k.A();
  for (int t = tid; t < T; t += kSkThreads) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int c = t - 1; c <= t + 1; ++c) {
      if (c < 1 || c > T - 2) continue;
      const TsStencil st = ts_stencil(k.fr, c);
      const double ct = st.at(c, t);
      a0 += st.ws * ct * ct;
      if (c <= t) a1 += st.ws * ct * st.at(c, t - 1);
      if (c == t - 1) a2 += st.ws * st.cp * st.cm;
    }
    Ap[3 * t] = a0; Ap[3 * t + 1] = a1; Ap[3 * t + 2] = a2;
  }

  if (nfree == 0) {                                                   // nothing to solve: init bit for bit, NaN stays NaN
    __syncthreads();                                                  // the prior's rows, read below by other threads
    for (int idx = tid; idx < T * K; idx += kSkThreads) {
      const size_t i = (size_t)n0 * K + idx;
      if (mode == SK_LINEARISE) {
        for (int m = 0; m < 3; ++m) { o.g[i * 3 + m] = 0.0; o.d[i * 3 + m] = 0.0; }
        continue;
      }
      const float* in = a.init + i * 4;
      const float x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3];
      float* q = o.out + i * 4;
      q[0] = x0; q[1] = x1; q[2] = x2; q[3] = x3;
      if (o.status) o.status[i] = 2;
      if (o.resid) { o.resid[i * 2] = NAN; o.resid[i * 2 + 1] = NAN; }
    }
    if (mode == SK_LINEARISE) {
      for (size_t idx = tid; idx < (size_t)T * n * n; idx += kSkThreads) o.hdiag[(size_t)n0 * n * n + idx] = 0.0;
      for (int t = tid; t < T; t += kSkThreads) {
        o.hoff[(size_t)(n0 + t) * 2] = t >= 1 ? a.acc_w * Ap[3 * t + 1] : 0.0;
        o.hoff[(size_t)(n0 + t) * 2 + 1] = t >= 2 ? a.acc_w * Ap[3 * t + 2] : 0.0;
      }
      if (tid == 0) o.C[sidx] = 0.0;
      return;
    }
    if (o.bone)
      for (int idx = tid; idx < T * Bn; idx += kSkThreads) {
        o.bone[((size_t)n0 * Bn + idx) * 2] = NAN; o.bone[((size_t)n0 * Bn + idx) * 2 + 1] = NAN;
      }
    if (tid == 0) {
      if (o.track_status) o.track_status[sidx] = 2;
      if (o.cost) { o.cost[(size_t)sidx * 2] = 0.0; o.cost[(size_t)sidx * 2 + 1] = 0.0; }
      if (o.trials) o.trials[sidx] = 0;
    }
    return;
  }

  double C;
  bool bad;
  sk_eval(k, 0, C, bad);                                              // its first barrier publishes everything above

  if (mode == SK_LINEARISE) {                                         // g, H + lambda diag H, the trial step and C at the start
    const double* G = k.G(0);
    for (int idx = tid; idx < T * K; idx += kSkThreads) {
      const int t = idx / K, j = idx - t * K;
      for (int m = 0; m < 3; ++m) o.g[((size_t)n0 * K + idx) * 3 + m] = s.free[j] ? G[(size_t)t * n + 3 * j + m] : 0.0;
    }
    for (int t = tid; t < T; t += kSkThreads) {
      o.hoff[(size_t)(n0 + t) * 2] = t >= 1 ? a.acc_w * Ap[3 * t + 1] : 0.0;
      o.hoff[(size_t)(n0 + t) * 2 + 1] = t >= 2 ? a.acc_w * Ap[3 * t + 2] : 0.0;
    }
    for (int t = 0; t < T; ++t) {
      sk_assemble(k, 0, t);
      double* q = o.hdiag + (size_t)(n0 + t) * n * n;
      for (int idx = tid; idx < n * n; idx += kSkThreads) {
        const int i = idx / n, j = idx - i * n;
        const double v = (i >= j ? s.A[i][j] : s.A[j][i]) * (i == j ? 1.0 + o.lambda : 1.0);
        q[idx] = s.free[i / 3] && s.free[j / 3] ? v : 0.0;
      }
    }
    if (tid == 0) o.C[sidx] = C;
    const bool ok = sk_factor(k, 0, o.lambda);
    if (ok) sk_back(k);
    const double* dx = k.Y();
    for (int idx = tid; idx < T * K; idx += kSkThreads) {
      const int t = idx / K, j = idx - t * K;
      for (int m = 0; m < 3; ++m) o.d[((size_t)n0 * K + idx) * 3 + m] = !ok ? (double)NAN : (s.free[j] ? dx[(size_t)t * n + 3 * j + m] : 0.0);
    }
    return;
  }

  const double C_init = C;
  for (int idx = tid; idx < T * K; idx += kSkThreads) {
    const int j = idx % K;
    if (o.resid) o.resid[((size_t)n0 * K + idx) * 2] = s.free[j] ? ts_rms(k.R2(0)[idx], usedw[idx]) : NAN;
  }
  if (o.bone)
    for (int idx = tid; idx < T * Bn; idx += kSkThreads) {
      const int t = idx / Bn, b = idx - t * Bn;
      double u[3];
      o.bone[((size_t)n0 * Bn + idx) * 2] = s.act[b] ? (float)sk_bone(k, X0, t, b, u) : NAN;
    }
  int cur = 0, st = 1, made = 0;
  double lambda = kLmLambda0;
  for (int it = 0; it < a.max_iter; ++it) {
    ++made;
    bool accept = false;
    double Ct = 0.0, big = 0.0;
    if (sk_factor(k, cur, lambda)) {
      sk_back(k);
      const double* Xc = k.X(cur);
      double* Xt = k.X(cur ^ 1);
      const double* dx = k.Y();
      for (int idx = tid; idx < T * K; idx += kSkThreads) {
        const int t = idx / K, j = idx - t * K;
        const size_t i = (size_t)t * n + 3 * j;
        const bool fr = s.free[j] != 0;
        const double d0 = fr ? dx[i] : 0.0, d1 = fr ? dx[i + 1] : 0.0, d2 = fr ? dx[i + 2] : 0.0;
        Xt[i] = Xc[i] + d0; Xt[i + 1] = Xc[i + 1] + d1; Xt[i + 2] = Xc[i + 2] + d2;
        big = fmax(big, sqrt(d0 * d0 + d1 * d1 + d2 * d2));
      }
      big = sk_max(s, big, tid);
      bool behind;
      sk_eval(k, cur ^ 1, Ct, behind);
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
  const double* Xc = k.X(cur);
  for (int idx = tid; idx < T * K; idx += kSkThreads) {
    const int t = idx / K, j = idx - t * K;
    const size_t i = (size_t)n0 * K + idx;
    const float* in = a.init + i * 4;
    const float x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3];
    float* q = o.out + i * 4;
    if (!s.free[j]) {
      q[0] = x0; q[1] = x1; q[2] = x2; q[3] = x3;
      if (o.status) o.status[i] = 2;
      if (o.resid) o.resid[i * 2 + 1] = NAN;
      continue;
    }
    const size_t x = (size_t)t * n + 3 * j;
    q[0] = (float)Xc[x]; q[1] = (float)Xc[x + 1]; q[2] = (float)Xc[x + 2]; q[3] = x3;
    if (o.status) o.status[i] = usedw[idx] ? 0 : 1;
    if (o.resid) o.resid[i * 2 + 1] = ts_rms(k.R2(cur)[idx], usedw[idx]);
  }
  if (o.bone)
    for (int idx = tid; idx < T * Bn; idx += kSkThreads) {
      const int t = idx / Bn, b = idx - t * Bn;
      double u[3];
      o.bone[((size_t)n0 * Bn + idx) * 2 + 1] = s.act[b] ? (float)sk_bone(k, Xc, t, b, u) : NAN;
    }
  if (tid == 0) {
    if (o.track_status) o.track_status[sidx] = (unsigned char)st;
    if (o.cost) { o.cost[(size_t)sidx * 2] = C_init; o.cost[(size_t)sidx * 2 + 1] = C; }
    if (o.trials) o.trials[sidx] = made;
  }
}

static inline bool sk_shape_ok(int N, int K) { return N > 0 && K >= 1 && K <= XAS_SKEL_MAX_JOINTS && (long)N * K <= 0x7fffffffL; }

// The checks of the skeleton's own arguments, before anything is launched, and the kernel's copy of the bones.
static int sk_check(const char* who, const int* bones, const float* length, int K, int Bn, double bone_w, SkBones& tab) {
  XAS_REQUIRE(K >= 1 && K <= XAS_SKEL_MAX_JOINTS, "%s: K=%d joints (needs 1 <= K <= XAS_SKEL_MAX_JOINTS = %d)", who, K,
              XAS_SKEL_MAX_JOINTS);
  XAS_REQUIRE(Bn >= 0 && Bn <= XAS_TRACK_MAX_BONES, "%s: Bn=%d bones (needs 0 <= Bn <= XAS_TRACK_MAX_BONES = %d)", who, Bn,
              XAS_TRACK_MAX_BONES);
  XAS_REQUIRE(Bn == 0 || (bones && length), "%s: null bones or length with Bn=%d (a host array [Bn][2] and a device array [S][Bn])",
              who, Bn);
  XAS_REQUIRE(bone_w >= 0.0 && bone_w < INFINITY, "%s: bone_w %f (needs a finite bone_w >= 0)", who, bone_w);
  tab = SkBones{};
  for (int b = 0; b < Bn; ++b) {
    const int i = bones[2 * b], j = bones[2 * b + 1];
    XAS_REQUIRE(i >= 0 && i < K && j >= 0 && j < K, "%s: bones[%d] = (%d, %d) is no pair of joints (needs 0 <= index < K = %d)", who,
                b, i, j, K);
    XAS_REQUIRE(i != j, "%s: bones[%d] joins joint %d to itself", who, b, i);
    tab.j[b][0] = i; tab.j[b][1] = j;
  }
  return 0;
}

}  // namespace xas

using namespace xas;

extern "C" size_t xas_track_skeleton_workspace_bytes(int N, int K) {
  if (!sk_shape_ok(N, K)) return 0;
  const size_t rec = (size_t)sk_layout(K).rec * sizeof(double), table = track_table_bytes(N);
  if ((size_t)N > ((size_t)-1 - table - 16) / rec) return 0;
  return align16(table + (size_t)N * rec);
}

extern "C" int xas_track_skeleton_linearise(const float* points, const float* P, const float* init, const unsigned char* views,
                                            const float* anchor, const float* info, const int* bones, const float* length,
                                            const int* start, const int* frame, int N, int V, int K, int S, int Bn, int flags,
                                            float huber, double anchor_huber, double acc_w, double bone_w, double lambda, double* g,
                                            double* hdiag, double* hoff, double* d, double* C, void* workspace, void* stream) {
  const char* who = "track_skeleton_linearise";
  XAS_REQUIRE(g && hdiag && hoff && d && C, "%s: null buffer (g, hdiag, hoff, d and C are required)", who);
  XAS_REQUIRE(lambda >= 0.0 && lambda < INFINITY, "%s: lambda %f (needs a finite lambda >= 0)", who, lambda);
  SkArgs p;
  if (ta_check(who, anchor, info, anchor_huber) || sk_check(who, bones, length, K, Bn, bone_w, p.bones)) return 1;
  if (int e = ts_plan(who, 1, points, P, init, views, start, frame, N, V, K, S, flags, huber, acc_w, workspace, as_stream(stream), p.a))
    return e;
  p.data = TsAnchored{anchor, info, anchor_huber};
  p.length = length; p.Bn = Bn; p.bone_w = bone_w;
  SkOut o = {};
  o.g = g; o.hdiag = hdiag; o.hoff = hoff; o.d = d; o.C = C; o.lambda = lambda;
  hipLaunchKernelGGL(track_skeleton_kernel, dim3((unsigned)S), dim3(kSkThreads), 0, as_stream(stream), p, o, (int)SK_LINEARISE);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_track_skeleton_smooth(const float* points, const float* P, const float* init, const unsigned char* views,
                                         const float* anchor, const float* info, const int* bones, const float* length,
                                         const int* start, const int* frame, int N, int V, int K, int S, int Bn, int flags,
                                         float huber, double anchor_huber, double acc_w, double bone_w, int max_iter, float* out,
                                         unsigned char* status, float* resid, float* bone, unsigned char* track_status, double* cost,
                                         int* trials, void* workspace, void* stream) {
  const char* who = "track_skeleton_smooth";
  if (ts_check_smooth(who, init, N, K, max_iter, out)) return 1;
  SkArgs p;
  if (ta_check(who, anchor, info, anchor_huber) || sk_check(who, bones, length, K, Bn, bone_w, p.bones)) return 1;
  if (int e = ts_plan(who, 1, points, P, init, views, start, frame, N, V, K, S, flags, huber, acc_w, workspace, as_stream(stream), p.a))
    return e;
  p.a.max_iter = max_iter;
  p.data = TsAnchored{anchor, info, anchor_huber};
  p.length = length; p.Bn = Bn; p.bone_w = bone_w;
  SkOut o = {};
  o.out = out; o.status = status; o.resid = resid; o.bone = bone; o.track_status = track_status; o.cost = cost; o.trials = trials;
  hipLaunchKernelGGL(track_skeleton_kernel, dim3((unsigned)S), dim3(kSkThreads), 0, as_stream(stream), p, o, (int)SK_SMOOTH);
  XAS_LAUNCH_CHECK();
  return 0;
}
