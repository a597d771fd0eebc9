// What xas_smpl_fit (smplfit.hip), xas_smpl_fit_tracks (smplfit_tracks.hip) and xas_smpl_fit_views (smplfit_views.hip) share: the dual numbers, the two rotation maps,
// the staging of a sample, the evaluation of a point with its vertex cache, the tangents, the assembly of H and g, the dense
// solve, the joint-term launch and the argument checks.  smplfit.hip states how a point is evaluated and linearised.
#pragma once
#include "common.h"

namespace xas {
namespace {

constexpr int kFitThreads = 256, kFitWaves = kFitThreads / 64;
constexpr int kJ = 24;                                 // SMPL joints
constexpr int kN = XAS_SMPLFIT_UNKNOWNS;               // 85 = omega 3, t 3, body pose 69, betas 10
constexpr int kRes = XAS_SMPLFIT_RESIDUALS;            // 133 = 54 joint, 69 pose prior, 10 shape prior
constexpr int kRows = 54, kT = 79, kReg = 51;          // joint rows; tangents through the body; 17 x 3 regressed sums
constexpr int kChunk = 2;                              // tangents per vertex pass
constexpr int kTri = kN * (kN + 1) / 2;                // packed lower triangle
constexpr int kCache = 15;                             // per vertex: v_posed 3, blended transform 12

static_assert(kN == 85 && kRes == 133, "the header's sizes");

template <int N>
struct Dual {
  double v, d[N];
};
template <int N>
__device__ __forceinline__ Dual<N> dmake(double v) {
  Dual<N> r;
  r.v = v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = 0.0;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator+(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v + b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator-(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v - b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator*(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v * b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator*(const Dual<N>& a, double b) {
  Dual<N> r;
  r.v = a.v * b;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> operator/(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  r.v = a.v / b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v;
  return r;
}
template <int N>
__device__ __forceinline__ Dual<N> dsqrt(const Dual<N>& a) {
  Dual<N> r;
  r.v = sqrt(a.v);
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] / (2.0 * r.v);
  return r;
}
template <int N>
__device__ __forceinline__ void dsincos(const Dual<N>& a, Dual<N>& s, Dual<N>& c) {
  s.v = sin(a.v);
  c.v = cos(a.v);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    s.d[i] = c.v * a.d[i];
    c.d[i] = -s.v * a.d[i];
  }
}

// The layer's rodrigues (rodrigues_layer.py:13-52): unit quaternion of angle |a + 1e-8|.  R row-major.
__device__ __forceinline__ void rodrigues_quat(const double (&a)[3], Dual<3> (&R)[9]) {
  Dual<3> x[3], n2 = dmake<3>(0.0);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    x[c] = dmake<3>(a[c]);
    x[c].d[c] = 1.0;
    const Dual<3> t = x[c] + dmake<3>(1e-8);
    n2 = n2 + t * t;
  }
  const Dual<3> angle = dsqrt(n2), half = angle * 0.5;
  Dual<3> sh, ch;
  dsincos(half, sh, ch);
  Dual<3> q[4] = {ch, sh * (x[0] / angle), sh * (x[1] / angle), sh * (x[2] / angle)};
  const Dual<3> qn = dsqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
  for (int c = 0; c < 4; ++c) q[c] = q[c] / qn;
  const Dual<3> w = q[0], X = q[1], Y = q[2], Z = q[3];
  const Dual<3> ww = w * w, xx = X * X, yy = Y * Y, zz = Z * Z;
  const Dual<3> wx = w * X, wy = w * Y, wz = w * Z, xy = X * Y, xz = X * Z, yz = Y * Z;
  R[0] = ((ww + xx) - yy) - zz; R[1] = xy * 2.0 - wz * 2.0;   R[2] = wy * 2.0 + xz * 2.0;
  R[3] = wz * 2.0 + xy * 2.0;   R[4] = ((ww - xx) + yy) - zz; R[5] = yz * 2.0 - wx * 2.0;
  R[6] = xz * 2.0 - wy * 2.0;   R[7] = wx * 2.0 + yz * 2.0;   R[8] = ((ww - xx) - yy) + zz;
}

// The plain exponential map of the root, R = I + sin(th) K + (1 - cos(th)) K^2 with K the cross matrix of omega / th; for
// th^2 < 1e-16 its series I + K(omega) + K(omega)^2 / 2, so that the derivative exists at omega = 0.
__device__ __forceinline__ void expmap(const double (&a)[3], Dual<3> (&R)[9]) {
  Dual<3> x[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    x[c] = dmake<3>(a[c]);
    x[c].d[c] = 1.0;
  }
  const Dual<3> th2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
  Dual<3> k[3], s, omc;
  if (th2.v < 1e-16) {
    k[0] = x[0]; k[1] = x[1]; k[2] = x[2];
    s = dmake<3>(1.0);
    omc = dmake<3>(0.5);
  } else {
    const Dual<3> th = dsqrt(th2);
    Dual<3> c;
    dsincos(th, s, c);
    omc = dmake<3>(1.0) - c;
#pragma unroll
    for (int i = 0; i < 3; ++i) k[i] = x[i] / th;
  }
  const Dual<3> z = dmake<3>(0.0);
  const Dual<3> K[9] = {z, z - k[2], k[1], k[2], z, z - k[0], z - k[1], k[0], z};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const Dual<3> kk = (K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c]) + K[r * 3 + 2] * K[6 + c];
      R[r * 3 + c] = (dmake<3>(r == c ? 1.0 : 0.0) + s * K[r * 3 + c]) + omc * kk;
    }
}

struct FitArgs {
  const float *pose, *betas, *trans;                    // [B][72], [B][10], [B][3]
  const float *vt, *sd, *pd, *skin;                     // v_template [V][3], shapedirs [V][3][10], posedirs [V][3][207], weights [V][24]
  const int* parents;                                   // [24]
  const float* hreg;                                    // [17][V]
  const int *rverts, *rcount;                           // compacted vertex list [V] and its length (device), or both NULL = all
  const float *tgt, *jw;                                // [B][18][3], [B][18]; both NULL = weight 1 against a zero target
  double wp, wsh;
  int V, center;
  const double* jpre;                                   // j_regressor . v_template [24][3], j_regressor . shapedirs [24][3][10]
  double* ws;                                           // per sample: dG2 [79][288], cache [15][V], H [kTri]
  size_t ws_stride;
};

struct FitShared {
  union {
    double J[kRows * kN];                               // joint rows of the Jacobian
    double L[kTri];                                     // Cholesky factor, packed rows
  } m;
  double g[kN], x[2][kN], d[kN];
  double R[kJ * 9], dR[kJ * 27];                        // rotations and d R / d (their three angles)
  double Gv[kJ * 12], G2v[kJ * 12];                     // chain transforms, and with the rest joint taken out
  double dG2[kChunk][kJ * 12];
  double dcen[kT * 3], cen[3], j0[kJ * 3];
  union {
    double red[kFitWaves][kChunk][kReg];              // per-wave sums of reduce_sums
    double dj[kChunk][kRows];                           // tangent joints between reduce_sums and the next vertex pass
  };
  double jr[kChunk][kReg];
  double j18[kRows], Y[2][kRows], r54[kRows], tgt[kRows], sw[18];
  double Rw[9], dRw[27];
  double scal[4];
  int par[kJ], nv;
};

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // i >= j

// H36M order of the 17 regressed rows (arms exchanged); joint 17 is the mean of joints 11 and 14
__device__ __forceinline__ int h36m_row(int k) { return k < 11 ? k : (k < 14 ? k + 3 : k - 3); }

// sum of acc[c][0..50] over the block -> s.jr[c]; fixed order: xor butterflies in the wave, then waves 0 + 1 + 2 + 3
template <int C>
__device__ __forceinline__ void reduce_sums(FitShared& s, double (&acc)[C][kReg]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int i = 0; i < kReg; ++i) {
      double v = acc[c][i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) s.red[wid][c][i] = v;
    }
  __syncthreads();
  for (int t = threadIdx.x; t < C * kReg; t += kFitThreads) {
    const int c = t / kReg, i = t % kReg;
    s.jr[c][i] = ((s.red[0][c][i] + s.red[1][c][i]) + s.red[2][c][i]) + s.red[3][c][i];
  }
  __syncthreads();
}

// regressed sums -> 1000 x the root-centred H36M joint coordinate t = 3 k + c (linear: serves values and tangents alike)
__device__ __forceinline__ double h36m_mm(const double* jr, int t) {
  const int k = t / 3, c = t % 3;
  const double v = k < 17 ? jr[h36m_row(k) * 3 + c] : (jr[h36m_row(11) * 3 + c] + jr[h36m_row(14) * 3 + c]) / 2.0;
  return 1000.0 * (v - jr[c]);
}

__device__ __forceinline__ int fit_vertex(const FitArgs& a, int kk) {
  const int v = a.rverts ? a.rverts[kk] : kk;
  return (unsigned)v < (unsigned)a.V ? v : -1;
}

// Evaluate the model at s.x[xi]: s.R, s.dR, s.Gv, s.G2v, s.cen, s.j0, s.j18, s.Y[yi], s.r54 and the vertex cache.
// -> the cost (the same on every thread).
__device__ __noinline__ double fit_evaluate(FitShared& s, const FitArgs& a, double* wsb, int xi, int yi) {
  const int tid = threadIdx.x;
  const double* x = s.x[xi];
  __syncthreads();
  if (tid < kJ) {
    double ang[3] = {0.0, 0.0, 0.0};
    if (tid > 0)
      for (int c = 0; c < 3; ++c) ang[c] = x[6 + 3 * (tid - 1) + c];
    Dual<3> R[9];
    rodrigues_quat(ang, R);
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      s.R[tid * 9 + e] = R[e].v;
#pragma unroll
      for (int c = 0; c < 3; ++c) s.dR[tid * 27 + c * 9 + e] = R[e].d[c];
    }
  } else if (tid >= 64 && tid < 64 + kJ * 3) {
    const int e = tid - 64;
    double v = a.jpre[e];
    for (int q = 0; q < 10; ++q) v += a.jpre[kJ * 3 + e * 10 + q] * x[75 + q];
    s.j0[e] = v;
  } else if (tid == 192) {
    const double om[3] = {x[0], x[1], x[2]};
    Dual<3> R[9];
    expmap(om, R);
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      s.Rw[e] = R[e].v;
#pragma unroll
      for (int c = 0; c < 3; ++c) s.dRw[c * 9 + e] = R[e].d[c];
    }
  }
  __syncthreads();
  if (tid == 0) {
    for (int i = 0; i < kJ; ++i) {
      const int p = s.par[i];
      double* G = s.Gv + i * 12;
      const double* Ri = s.R + i * 9;
      if (p < 0) {
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c) G[r * 4 + c] = Ri[r * 3 + c];
          G[r * 4 + 3] = s.j0[i * 3 + r];
        }
      } else {
        const double* Gp = s.Gv + p * 12;
        const double tr[3] = {s.j0[i * 3] - s.j0[p * 3], s.j0[i * 3 + 1] - s.j0[p * 3 + 1], s.j0[i * 3 + 2] - s.j0[p * 3 + 2]};
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c)
            G[r * 4 + c] = (Gp[r * 4] * Ri[c] + Gp[r * 4 + 1] * Ri[3 + c]) + Gp[r * 4 + 2] * Ri[6 + c];
          G[r * 4 + 3] = ((Gp[r * 4] * tr[0] + Gp[r * 4 + 1] * tr[1]) + Gp[r * 4 + 2] * tr[2]) + Gp[r * 4 + 3];
        }
      }
      double* G2 = s.G2v + i * 12;
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) G2[r * 4 + c] = G[r * 4 + c];
        G2[r * 4 + 3] = G[r * 4 + 3] - ((G[r * 4] * s.j0[i * 3] + G[r * 4 + 1] * s.j0[i * 3 + 1]) + G[r * 4 + 2] * s.j0[i * 3 + 2]);
      }
    }
    for (int c = 0; c < 3; ++c) s.cen[c] = a.center >= 0 ? s.Gv[a.center * 12 + c * 4 + 3] : 0.0;
  }
  __syncthreads();
  double acc[1][kReg];
#pragma unroll
  for (int i = 0; i < kReg; ++i) acc[0][i] = 0.0;
  double* cache = wsb + (size_t)kT * kJ * 12;
  const size_t V = (size_t)a.V;
  for (int kk = tid; kk < s.nv; kk += kFitThreads) {
    const int v = fit_vertex(a, kk);
    if (v < 0) continue;
    double vp[3];
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
      double vs = (double)a.vt[(size_t)v * 3 + c];
      const float* sd = a.sd + ((size_t)v * 3 + c) * 10;
      for (int q = 0; q < 10; ++q) vs += (double)sd[q] * x[75 + q];
      const float* pd = a.pd + ((size_t)v * 3 + c) * 207;
      double ps = 0.0;
#pragma unroll 1
      for (int j = 1; j < kJ; ++j)
#pragma unroll
        for (int e = 0; e < 9; ++e) ps += (double)pd[(j - 1) * 9 + e] * (s.R[j * 9 + e] - ((e & 3) == 0 ? 1.0 : 0.0));
      vp[c] = vs + ps;
    }
    double T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.0;
#pragma unroll 1
    for (int j = 0; j < kJ; ++j) {
      const double w = (double)a.skin[(size_t)v * kJ + j];
      if (w != 0.0)
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] += w * s.G2v[j * 12 + e];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) cache[(size_t)c * V + kk] = vp[c];
#pragma unroll
    for (int e = 0; e < 12; ++e) cache[(size_t)(3 + e) * V + kk] = T[e];
    double vert[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) vert[r] = (((T[r * 4] * vp[0] + T[r * 4 + 1] * vp[1]) + T[r * 4 + 2] * vp[2]) + T[r * 4 + 3]) - s.cen[r];
#pragma unroll
    for (int l = 0; l < 17; ++l) {
      const double rg = (double)a.hreg[(size_t)l * V + v];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[0][l * 3 + c] += rg * vert[c];
    }
  }
  reduce_sums<1>(s, acc);
  if (tid < kRows) s.j18[tid] = h36m_mm(s.jr[0], tid);
  __syncthreads();
  if (tid < kRows) {
    const int k = tid / 3, c = tid % 3;
    const double y = ((s.Rw[c * 3] * s.j18[k * 3] + s.Rw[c * 3 + 1] * s.j18[k * 3 + 1]) + s.Rw[c * 3 + 2] * s.j18[k * 3 + 2]) + x[3 + c];
    s.Y[yi][tid] = y;
    s.r54[tid] = s.sw[k] > 0.0 ? s.sw[k] * (y - s.tgt[tid]) : 0.0;    // weight 0: the target is never read into arithmetic
  }
  __syncthreads();
  if (tid == 0) {
    double C = 0.0;
    for (int i = 0; i < kRows; ++i) C += s.r54[i] * s.r54[i];
    for (int i = 0; i < 69; ++i) C += a.wp * (x[6 + i] * x[6 + i]);
    for (int i = 0; i < 10; ++i) C += a.wsh * (x[75 + i] * x[75 + i]);
    s.scal[0] = C;
  }
  __syncthreads();
  return s.scal[0];
}

// s.m.J at the point fit_evaluate saw last (s.x[xi]).
__device__ __noinline__ void fit_tangents(FitShared& s, const FitArgs& a, double* wsb, int xi) {
  const int tid = threadIdx.x;
  double* dGall = wsb;
  if (tid < kT) {                                       // one tangent through the chain
    const int p = tid, jp = p < 69 ? 1 + p / 3 : -1, ax = p % 3, q = p - 69;
    double* dg = dGall + (size_t)p * kJ * 12;
    double dc[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < kJ; ++i) {
      const int pr = s.par[i];
      double dRi[9], dtr[3] = {0.0, 0.0, 0.0}, dG[12];
#pragma unroll
      for (int e = 0; e < 9; ++e) dRi[e] = i == jp ? s.dR[i * 27 + ax * 9 + e] : 0.0;
      if (p >= 69)
        for (int c = 0; c < 3; ++c)
          dtr[c] = a.jpre[kJ * 3 + (i * 3 + c) * 10 + q] - (pr >= 0 ? a.jpre[kJ * 3 + (pr * 3 + c) * 10 + q] : 0.0);
      if (pr < 0) {
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c) dG[r * 4 + c] = dRi[r * 3 + c];
          dG[r * 4 + 3] = dtr[r];
        }
      } else {
        const double *Gp = s.Gv + pr * 12, *Ri = s.R + i * 9, *dGp = dg + pr * 12;
        const double tr[3] = {s.j0[i * 3] - s.j0[pr * 3], s.j0[i * 3 + 1] - s.j0[pr * 3 + 1], s.j0[i * 3 + 2] - s.j0[pr * 3 + 2]};
        for (int r = 0; r < 3; ++r) {
          const double g0 = dGp[r * 4], g1 = dGp[r * 4 + 1], g2 = dGp[r * 4 + 2], g3 = dGp[r * 4 + 3];
          for (int c = 0; c < 3; ++c)
            dG[r * 4 + c] = ((g0 * Ri[c] + g1 * Ri[3 + c]) + g2 * Ri[6 + c]) +
                            ((Gp[r * 4] * dRi[c] + Gp[r * 4 + 1] * dRi[3 + c]) + Gp[r * 4 + 2] * dRi[6 + c]);
          dG[r * 4 + 3] = (((g0 * tr[0] + g1 * tr[1]) + g2 * tr[2]) + g3) +
                          ((Gp[r * 4] * dtr[0] + Gp[r * 4 + 1] * dtr[1]) + Gp[r * 4 + 2] * dtr[2]);
        }
      }
      for (int e = 0; e < 12; ++e) dg[i * 12 + e] = dG[e];
      if (i == a.center)
        for (int c = 0; c < 3; ++c) dc[c] = dG[c * 4 + 3];
    }
    for (int c = 0; c < 3; ++c) s.dcen[p * 3 + c] = dc[c];
    for (int i = 0; i < kJ; ++i) {                      // take the rest joint out: t -= d(G_rot j0)
      const double* G = s.Gv + i * 12;
      for (int r = 0; r < 3; ++r) {
        double t = dg[i * 12 + r * 4 + 3];
        for (int c = 0; c < 3; ++c) {
          t -= dg[i * 12 + r * 4 + c] * s.j0[i * 3 + c];
          if (p >= 69) t -= G[r * 4 + c] * a.jpre[kJ * 3 + (i * 3 + c) * 10 + q];
        }
        dg[i * 12 + r * 4 + 3] = t;
      }
    }
  }
  // omega and t columns
  if (tid >= 64 && tid < 64 + kRows) {
    const int t = tid - 64, k = t / 3, c = t % 3;
    const double sw = s.sw[k];
    for (int ax = 0; ax < 3; ++ax) {
      const double* dRw = s.dRw + ax * 9 + c * 3;
      const double v = (dRw[0] * s.j18[k * 3] + dRw[1] * s.j18[k * 3 + 1]) + dRw[2] * s.j18[k * 3 + 2];
      s.m.J[t * kN + ax] = sw > 0.0 ? sw * v : 0.0;
      s.m.J[t * kN + 3 + ax] = (sw > 0.0 && ax == c) ? sw : 0.0;
    }
  }
  __syncthreads();
  const double* cache = wsb + (size_t)kT * kJ * 12;
  const size_t V = (size_t)a.V;
  for (int p0 = 0; p0 < kT; p0 += kChunk) {
    for (int t = tid; t < kChunk * kJ * 12; t += kFitThreads) {
      const int c = t / (kJ * 12), e = t % (kJ * 12);
      s.dG2[c][e] = p0 + c < kT ? dGall[(size_t)(p0 + c) * kJ * 12 + e] : 0.0;
    }
    __syncthreads();
    double acc[kChunk][kReg];
#pragma unroll
    for (int c = 0; c < kChunk; ++c)
#pragma unroll
      for (int i = 0; i < kReg; ++i) acc[c][i] = 0.0;
    for (int kk = tid; kk < s.nv; kk += kFitThreads) {
      const int v = fit_vertex(a, kk);
      if (v < 0) continue;
      double vp[3], T[12], dT[kChunk][12], dv[kChunk][3];
#pragma unroll
      for (int c = 0; c < 3; ++c) vp[c] = cache[(size_t)c * V + kk];
#pragma unroll
      for (int e = 0; e < 12; ++e) T[e] = cache[(size_t)(3 + e) * V + kk];
#pragma unroll
      for (int c = 0; c < kChunk; ++c)
#pragma unroll
        for (int e = 0; e < 12; ++e) dT[c][e] = 0.0;
#pragma unroll 1
      for (int j = 0; j < kJ; ++j) {
        const double w = (double)a.skin[(size_t)v * kJ + j];
        if (w != 0.0)
#pragma unroll
          for (int c = 0; c < kChunk; ++c)
#pragma unroll
            for (int e = 0; e < 12; ++e) dT[c][e] += w * s.dG2[c][j * 12 + e];
      }
#pragma unroll
      for (int c = 0; c < kChunk; ++c) {
        const int p = p0 + c;
        double dvp[3] = {0.0, 0.0, 0.0};
        if (p < 69) {
          const int jp = 1 + p / 3;
          const double* dR = s.dR + jp * 27 + (p % 3) * 9;
          for (int cc = 0; cc < 3; ++cc) {
            const float* pd = a.pd + ((size_t)v * 3 + cc) * 207 + (jp - 1) * 9;
            double t = 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) t += (double)pd[e] * dR[e];
            dvp[cc] = t;
          }
        } else if (p < kT) {
          for (int cc = 0; cc < 3; ++cc) dvp[cc] = (double)a.sd[((size_t)v * 3 + cc) * 10 + (p - 69)];
        }
        const double* dcn = s.dcen + (p < kT ? p : 0) * 3;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double t0 = ((dT[c][r * 4] * vp[0] + dT[c][r * 4 + 1] * vp[1]) + dT[c][r * 4 + 2] * vp[2]) + dT[c][r * 4 + 3];
          const double t1 = (T[r * 4] * dvp[0] + T[r * 4 + 1] * dvp[1]) + T[r * 4 + 2] * dvp[2];
          dv[c][r] = p < kT ? (t0 + t1) - dcn[r] : 0.0;
        }
      }
#pragma unroll
      for (int l = 0; l < 17; ++l) {
        const double rg = (double)a.hreg[(size_t)l * V + v];
#pragma unroll
        for (int c = 0; c < kChunk; ++c)
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) acc[c][l * 3 + cc] += rg * dv[c][cc];
      }
    }
    reduce_sums<kChunk>(s, acc);
    for (int t = tid; t < kChunk * kRows; t += kFitThreads) s.dj[t / kRows][t % kRows] = h36m_mm(s.jr[t / kRows], t % kRows);
    __syncthreads();
    for (int t = tid; t < kChunk * kRows; t += kFitThreads) {
      const int c = t / kRows, row = t % kRows, k = row / 3, cc = row % 3, p = p0 + c;
      if (p < kT) {
        const double* d = s.dj[c] + k * 3;
        const double v = (s.Rw[cc * 3] * d[0] + s.Rw[cc * 3 + 1] * d[1]) + s.Rw[cc * 3 + 2] * d[2];
        s.m.J[row * kN + 6 + p] = s.sw[k] > 0.0 ? s.sw[k] * v : 0.0;
      }
    }
    __syncthreads();
  }
}

// H = J^T J + priors (workspace, packed lower triangle), g = J^T r + priors, from s.m.J, s.r54 and s.x[xi]
__device__ __noinline__ void fit_assemble(FitShared& s, const FitArgs& a, double* H, int xi) {
  const int tid = threadIdx.x;
  for (int e = tid; e < kN * kN; e += kFitThreads) {
    const int i = e / kN, j = e % kN;
    if (j > i) continue;
    double h = 0.0;
    for (int r = 0; r < kRows; ++r) h += s.m.J[r * kN + i] * s.m.J[r * kN + j];
    if (i == j && i >= 6) h += i < 75 ? a.wp : a.wsh;
    H[tri(i, j)] = h;
  }
  if (tid < kN) {
    double g = 0.0;
    for (int r = 0; r < kRows; ++r) g += s.m.J[r * kN + tid] * s.r54[r];
    if (tid >= 6) g += (tid < 75 ? a.wp : a.wsh) * s.x[xi][tid];
    s.g[tid] = g;
  }
  __syncthreads();
}

// Cholesky of H + lambda diag(H) into s.m.L (left-looking, a thread per row), then L L^T d = -g into s.d.
// false at a pivot that is not > 0 (NaN fails too).  Uniform over the block.
__device__ __noinline__ bool fit_solve(FitShared& s, const double* H, double lambda) {
  const int tid = threadIdx.x;
  double* L = s.m.L;
  for (int j = 0; j < kN; ++j) {
    __syncthreads();
    double v = 0.0;
    if (tid >= j && tid < kN) {
      v = H[tri(tid, j)];
      if (tid == j) v += lambda * v;
      for (int k = 0; k < j; ++k) v -= L[tri(tid, k)] * L[tri(j, k)];
      s.d[tid] = v;
    }
    __syncthreads();
    const double piv = s.d[j];
    if (!(piv > 0.0)) return false;
    const double sd = sqrt(piv);
    if (tid >= j && tid < kN) L[tri(tid, j)] = tid == j ? sd : v / sd;
  }
  __syncthreads();
  if (tid < kN) s.d[tid] = -s.g[tid];
  for (int j = 0; j < kN; ++j) {
    __syncthreads();
    if (tid == j) s.d[j] = s.d[j] / L[tri(j, j)];
    __syncthreads();
    if (tid > j && tid < kN) s.d[tid] -= L[tri(tid, j)] * s.d[j];
  }
  for (int j = kN - 1; j >= 0; --j) {
    __syncthreads();
    if (tid == j) s.d[j] = s.d[j] / L[tri(j, j)];
    __syncthreads();
    if (tid < j) s.d[tid] -= L[tri(j, tid)] * s.d[j];
  }
  __syncthreads();
  return true;
}

// parameters, targets and weights of sample b into LDS -> the number of joints of positive weight
__device__ int fit_stage(FitShared& s, const FitArgs& a, int b) {
  const int tid = threadIdx.x;
  if (tid < kN) {
    double v;
    if (tid < 3) v = (double)a.pose[(size_t)b * 72 + tid];
    else if (tid < 6) v = (double)a.trans[(size_t)b * 3 + tid - 3];
    else if (tid < 75) v = (double)a.pose[(size_t)b * 72 + tid - 3];
    else v = (double)a.betas[(size_t)b * 10 + tid - 75];
    s.x[0][tid] = v;
  }
  if (tid >= 128 && tid < 128 + 18) {
    const int k = tid - 128;
    const float w = a.jw ? a.jw[(size_t)b * 18 + k] : 1.f;   // no weights (smplfit_views.hip): s.sw = 1 and s.tgt = 0, so that
    const bool on = w > 0.f;                            // s.r54 and s.m.J hold Y and dY/dx.  NaN and negative weights count as 0
    s.sw[k] = on ? sqrt((double)w) : 0.0;
    for (int c = 0; c < 3; ++c) s.tgt[k * 3 + c] = on && a.tgt ? (double)a.tgt[((size_t)b * 18 + k) * 3 + c] : 0.0;
  }
  if (tid >= 192 && tid < 192 + kJ) {
    const int i = tid - 192, p = a.parents[i];
    s.par[i] = (p >= 0 && p < i) ? p : -1;
  }
  if (tid == 255) {
    int n = a.rcount ? *a.rcount : a.V;
    s.nv = n < 0 ? 0 : (n > a.V ? a.V : n);
  }
  __syncthreads();
  int usable = 0;
  for (int k = 0; k < 18; ++k) usable += s.sw[k] > 0.0 ? 1 : 0;
  return usable;
}

// j_regressor . v_template [24][3] and j_regressor . shapedirs [24][3][10] in double: one wave per dot product, lanes stride
// the vertices, xor butterflies.  The joint locations are affine in the betas, so the chain never touches the vertices.
__global__ __launch_bounds__(64) void smpl_fit_joint_terms_kernel(const float* __restrict__ jreg, const float* __restrict__ vt,
                                                                  const float* __restrict__ sd, int V, double* __restrict__ out) {
  const int o = blockIdx.x, lane = threadIdx.x;          // o < 72: (j, c) of the template; else 72 + (j, c, q)
  const int jc = o < kJ * 3 ? o : (o - kJ * 3) / 10, q = o < kJ * 3 ? -1 : (o - kJ * 3) % 10;
  const int j = jc / 3, c = jc % 3;
  double v = 0.0;
  for (int k = lane; k < V; k += 64) {
    const double x = q < 0 ? (double)vt[(size_t)k * 3 + c] : (double)sd[((size_t)k * 3 + c) * 10 + q];
    v += (double)jreg[(size_t)j * V + k] * x;
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  if (lane == 0) out[o] = v;
}

constexpr size_t kPreDoubles = kJ * 3 * 11;             // 792, padded below to 1024

size_t fit_sample_doubles(int V) { return (size_t)kT * kJ * 12 + (size_t)kCache * V + kTri; }

int fit_check(const char* who, const float* pose, const float* betas, const float* trans, const float* vt, const float* sd,
              const float* pd, const float* jreg, const float* skin, const int* parents, const float* hreg, const int* rverts,
              const int* rcount, const float* tgt, const float* jw, float wp, float wsh, int B, int V, int center, void* ws,
              bool data = true) {                       // data = false: an entry point without targets and weights
  XAS_REQUIRE(B >= 0 && V >= 1, "%s: bad shape B=%d V=%d (B >= 0, V >= 1)", who, B, V);
  XAS_REQUIRE(B == 0 || (pose && betas && trans && vt && sd && pd && jreg && skin && parents && hreg && (!data || (tgt && jw)) && ws),
              "%s: null buffer (parameters, the SMPL arrays, parents, the regressor%s and workspace are required)", who,
              data ? ", targets, weights" : "");
  XAS_REQUIRE((rverts == nullptr) == (rcount == nullptr), "%s: the vertex list and its length come together (or both NULL)", who);
  XAS_REQUIRE(center >= -1 && center < kJ, "%s: center_idx=%d (needs -1 = none, or a joint < 24)", who, center);
  XAS_REQUIRE(wp >= 0.f && wp < INFINITY && wsh >= 0.f && wsh < INFINITY, "%s: priors %f, %f (need finite weights >= 0)", who,
              (double)wp, (double)wsh);
  return 0;
}

}  // namespace
}  // namespace xas

