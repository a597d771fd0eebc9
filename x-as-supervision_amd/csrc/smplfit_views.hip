// xas_smpl_fit_views / xas_smpl_fit_views_linearise: xas_smpl_fit with the DATA TERM in pixels (eval.py --fit-smpl --fit-data
// reproj; include/xas_hip.h states the cost, which observations count and the schedule; tests/_smplfit_views_oracle.py restates
// them in float64 torch).  A model joint Y_k(x) is held to the detections of the cameras that see it (xas_triangulate_refine's
// reprojection term, multiview.h) and to a 3-D anchor with a 3x3 information matrix (xas_track_anchor_smooth's term,
// track_anchor.h).  Both are functions of Y_k alone, so per joint they reduce to a PointFit: a cost c_k, a 3x3 Gauss-Newton
// block A_k and a 3-gradient b_k, and
//   H = sum_k Jy_k^T A_k Jy_k + priors,   g = sum_k Jy_k^T b_k + priors,   Jy_k = dY_k / dx (3 x 85).
// Y and Jy come from smplfit.h as they are: a sample staged without targets and weights has s.sw = 1 and s.tgt = 0, so
// fit_evaluate leaves Y in s.Y and fit_tangents leaves dY / dx in s.m.J (a factor 1.0 and a subtracted 0.0 change no bit).
// One workgroup of 256 threads per sample and the whole LM in one launch, as smplfit.hip: after every evaluation 18 threads
// form (c_k, A_k, b_k) at Y_k, one thread sums the cost in ascending joint order, and after the tangents the block contracts
// A_k with the two columns of Jy_k inside the (i, j) loop of the assembly: no A J product is stored (it would take another
// 36 KB of LDS), the blocks, costs and masks take 1 592 bytes beside FitShared.  A_k is never factored: it has rank 2 for
// one camera without an anchor.  H lives in the workspace as xas_smpl_fit's does and fit_solve takes it unchanged.  No atomics.
#include "smplfit.h"
#include "track_anchor.h"

namespace xas {
namespace {

constexpr int kK = 18;                                  // joints
constexpr int kViewBits = (1 << XAS_TRI_MAX_VIEWS) - 1, kAnchorBit = 0x80;
static_assert(XAS_TRI_MAX_VIEWS <= 7, "the anchor's bit of `used` lies above the views'");

struct ViewsArgs {
  const float *pts, *P;                                 // [B][C][18][3] = u, v, weight; [B][C][3][4]
  const unsigned char* views;                           // [B][18] or NULL
  const float *anchor, *info;                           // [B][18][3], [B][18][6], or both NULL
  int C, flags;
  double huber, ahuber;
};

struct ViewsShared {
  double A[kK][6], b[kK][3], c[kK];                     // the joints' blocks (upper triangle), gradients and costs at the last evaluation
  int used[kK];                                         // the views a joint uses | kAnchorBit; decided at the init
  int front[kK];
};

// Which observations count, at the init (s.Y[0]): -> vs.used and the number of joints used.
__device__ int views_classify(const FitShared& s, ViewsShared& vs, const ViewsArgs& v, int b) {
  const int k = threadIdx.x;
  if (k < kK) {
    ViewObs o;
    load_obs(v.pts, b, v.C, kK, k, v.flags, o);
    int used = views_used(o.valid, v.views ? v.views[(size_t)b * kK + k] : 0);
    const double Xh[4] = {s.Y[0][k * 3], s.Y[0][k * 3 + 1], s.Y[0][k * 3 + 2], 1.0};
#pragma unroll
    for (int c = 0; c < XAS_TRI_MAX_VIEWS; ++c) {
      if (!((used >> c) & 1)) continue;
      double h[3];
      const bool front = project_view(v.P + ((size_t)b * v.C + c) * 12, Xh, h);
      if (!(front && fabsf(o.pu[c]) < INFINITY && fabsf(o.pv[c]) < INFINITY)) used &= ~(1 << c);
    }
    double A[3], W[6];
    if (anchor_load(v.anchor, v.info, (size_t)b * kK + k, A, W)) used |= kAnchorBit;
    vs.used[k] = used;
  }
  __syncthreads();
  int n = 0;
  for (int j = 0; j < kK; ++j) n += vs.used[j] ? 1 : 0;
  return n;
}

// The data terms at s.Y[yi] (what fit_evaluate just left) -> vs.A, vs.b, vs.c; the cost (joints ascending, then the priors as
// xas_smpl_fit sums them); front = no joint lies behind a view it uses.  The same on every thread.
__device__ double views_terms(FitShared& s, ViewsShared& vs, const FitArgs& a, const ViewsArgs& v, int b, int xi, int yi, bool& front) {
  const int k = threadIdx.x;
  if (k < kK) {
    const int used = vs.used[k];
    const double X[3] = {s.Y[yi][k * 3], s.Y[yi][k * 3 + 1], s.Y[yi][k * 3 + 2]};
    PointFit f;
    f.clear();                                          // a joint that is not used: nothing of it is read
    bool fr = true;
    if (used & kViewBits) {
      ViewObs o;
      load_obs(v.pts, b, v.C, kK, k, v.flags, o);
      fr = point_fit(v.P + (size_t)b * v.C * 12, o, used & kViewBits, v.huber, X, f);
    }
    if (used & kAnchorBit) {
      double A[3], W[6];
      anchor_load(v.anchor, v.info, (size_t)b * kK + k, A, W);
      anchor_term(A, W, v.ahuber, X, f);
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) vs.A[k][m] = f.H[m];
#pragma unroll
    for (int m = 0; m < 3; ++m) vs.b[k][m] = f.g[m];
    vs.c[k] = f.C;
    vs.front[k] = fr ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double* x = s.x[xi];
    double C = 0.0;
    int fr = 1;
    for (int j = 0; j < kK; ++j) {
      C += vs.c[j];
      fr &= vs.front[j];
    }
    for (int i = 0; i < 69; ++i) C += a.wp * (x[6 + i] * x[6 + i]);
    for (int i = 0; i < 10; ++i) C += a.wsh * (x[75 + i] * x[75 + i]);
    s.scal[0] = C;
    s.scal[1] = (double)fr;
  }
  __syncthreads();
  front = s.scal[1] != 0.0;
  return s.scal[0];
}

// H = sum_k Jy_k^T A_k Jy_k + priors (workspace, packed lower triangle), g = sum_k Jy_k^T b_k + priors, from s.m.J (= dY / dx),
// vs.A, vs.b and s.x[xi].  The 3x3 contraction runs inside the (i, j) loop, joints ascending.
__device__ __noinline__ void views_assemble(FitShared& s, const ViewsShared& vs, const FitArgs& a, double* H, int xi) {
  const int tid = threadIdx.x;
  for (int e = tid; e < kN * kN; e += kFitThreads) {
    const int i = e / kN, j = e % kN;
    if (j > i) continue;
    double h = 0.0;
    for (int k = 0; k < kK; ++k) {
      if (!vs.used[k]) continue;
      const double* J = s.m.J + k * 3 * kN;
      const double* A = vs.A[k];
      const double i0 = J[i], i1 = J[kN + i], i2 = J[2 * kN + i], j0 = J[j], j1 = J[kN + j], j2 = J[2 * kN + j];
      const double t0 = (A[0] * j0 + A[1] * j1) + A[2] * j2;
      const double t1 = (A[1] * j0 + A[3] * j1) + A[4] * j2;
      const double t2 = (A[2] * j0 + A[4] * j1) + A[5] * j2;
      h += (i0 * t0 + i1 * t1) + i2 * t2;
    }
    if (i == j && i >= 6) h += i < 75 ? a.wp : a.wsh;
    H[tri(i, j)] = h;
  }
  if (tid < kN) {
    double g = 0.0;
    for (int k = 0; k < kK; ++k) {
      if (!vs.used[k]) continue;
      const double* J = s.m.J + k * 3 * kN;
      g += (J[tid] * vs.b[k][0] + J[kN + tid] * vs.b[k][1]) + J[2 * kN + tid] * vs.b[k][2];
    }
    if (tid >= 6) g += (tid < 75 ? a.wp : a.wsh) * s.x[xi][tid];
    s.g[tid] = g;
  }
  __syncthreads();
}

__device__ __forceinline__ void views_write_used(const ViewsShared& vs, unsigned char* used_o, int b) {
  if (threadIdx.x < kK) used_o[(size_t)b * kK + threadIdx.x] = (unsigned char)vs.used[threadIdx.x];
}

__global__ __launch_bounds__(kFitThreads) void smpl_fit_views_linearise_kernel(FitArgs a, ViewsArgs v, double* __restrict__ H_o,
                                                                               double* __restrict__ g_o, double* __restrict__ cost_o,
                                                                               double* __restrict__ blocks_o,
                                                                               unsigned char* __restrict__ used_o) {
  __shared__ FitShared s;
  __shared__ ViewsShared vs;
  const int b = blockIdx.x, tid = threadIdx.x;
  double* wsb = a.ws + (size_t)b * a.ws_stride;
  double* H = wsb + (size_t)kT * kJ * 12 + (size_t)kCache * a.V;
  fit_stage(s, a, b);
  fit_evaluate(s, a, wsb, 0, 0);
  views_classify(s, vs, v, b);
  views_write_used(vs, used_o, b);
  bool front;
  const double C = views_terms(s, vs, a, v, b, 0, 0, front);
  fit_tangents(s, a, wsb, 0);
  views_assemble(s, vs, a, H, 0);                       // ends past a barrier: the packed triangle is the block's to read
  double* Hb = H_o + (size_t)b * kN * kN;
  for (int e = tid; e < kN * kN; e += kFitThreads) {
    const int i = e / kN, j = e % kN;
    Hb[e] = j <= i ? H[tri(i, j)] : H[tri(j, i)];
  }
  if (tid < kN) g_o[(size_t)b * kN + tid] = s.g[tid];
  for (int t = tid; t < kK * 9; t += kFitThreads) {
    const int k = t / 9, m = t % 9;
    blocks_o[(size_t)b * kK * 9 + t] = m < 6 ? vs.A[k][m] : vs.b[k][m - 6];
  }
  if (tid == 255) cost_o[b] = C;
}

__global__ __launch_bounds__(kFitThreads) void smpl_fit_views_kernel(FitArgs a, ViewsArgs v, int max_iters, double* __restrict__ pose_o,
                                                                     double* __restrict__ betas_o, double* __restrict__ trans_o,
                                                                     double* __restrict__ joints_o, double* __restrict__ cost_o,
                                                                     int* __restrict__ iters_o, unsigned char* __restrict__ status_o,
                                                                     unsigned char* __restrict__ used_o) {
  __shared__ FitShared s;
  __shared__ ViewsShared vs;
  const int b = blockIdx.x, tid = threadIdx.x;
  double* wsb = a.ws + (size_t)b * a.ws_stride;
  double* H = wsb + (size_t)kT * kJ * 12 + (size_t)kCache * a.V;
  fit_stage(s, a, b);
  fit_evaluate(s, a, wsb, 0, 0);
  const int usable = views_classify(s, vs, v, b);
  views_write_used(vs, used_o, b);
  bool front;
  double C = views_terms(s, vs, a, v, b, 0, 0, front);
  const double C0 = C;
  int cur = 0, st = 1, it = 0;
  if (usable < 6 || !(fabs(C) < INFINITY)) {
    st = 2;
  } else if (max_iters > 0) {
    fit_tangents(s, a, wsb, 0);
    views_assemble(s, vs, a, H, 0);
    double lambda = 1e-3;
    while (it < max_iters) {
      ++it;
      bool accept = false;
      double Ct = 0.0, big = 0.0;
      if (fit_solve(s, H, lambda)) {
        if (tid < kN) s.x[cur ^ 1][tid] = s.x[cur][tid] + s.d[tid];
        __syncthreads();
        for (int i = 0; i < kN; ++i) big = fmax(big, fabs(s.d[i]));
        fit_evaluate(s, a, wsb, cur ^ 1, cur ^ 1);
        Ct = views_terms(s, vs, a, v, b, cur ^ 1, cur ^ 1, front);
        accept = front && fabs(Ct) < INFINITY && Ct < C;   // NaN never passes; nor does a joint behind a view it uses
      }
      if (accept) {
        cur ^= 1;
        C = Ct;
        lambda *= 0.1;
        if (big < XAS_SMPLFIT_STEP_TOL) { st = 0; break; }
        fit_tangents(s, a, wsb, cur);
        views_assemble(s, vs, a, H, cur);               // vs holds the blocks of the trial just accepted
      } else {
        lambda *= 10.0;
        if (lambda > 1e12) break;
      }
    }
  }
  __syncthreads();
  const double* x = s.x[cur];
  if (tid < 72) pose_o[(size_t)b * 72 + tid] = tid < 3 ? x[tid] : x[tid + 3];
  if (tid >= 72 && tid < 82) betas_o[(size_t)b * 10 + tid - 72] = x[75 + tid - 72];
  if (tid >= 82 && tid < 85) trans_o[(size_t)b * 3 + tid - 82] = x[3 + tid - 82];
  if (tid >= 128 && tid < 128 + kRows) joints_o[(size_t)b * kRows + tid - 128] = s.Y[cur][tid - 128];
  if (tid == 255) {
    cost_o[(size_t)b * 2] = C0;
    cost_o[(size_t)b * 2 + 1] = C;
    iters_o[b] = it;
    status_o[b] = (unsigned char)st;
  }
}

// The checks of both entry points, then the joint-term launch -> the kernels' arguments.
int views_plan(const char* who, const float* pose, const float* betas, const float* trans, const float* vt, const float* sd,
               const float* pd, const float* jreg, const float* skin, const int* parents, const float* hreg, const int* rverts,
               const int* rcount, const float* points, const float* P, const unsigned char* views, const float* anchor,
               const float* info, int flags, double huber, double anchor_huber, float wp, float wsh, int B, int V, int C,
               int center, void* ws, FitArgs& a, ViewsArgs& v) {
  if (fit_check(who, pose, betas, trans, vt, sd, pd, jreg, skin, parents, hreg, rverts, rcount, nullptr, nullptr, wp, wsh, B, V,
                center, ws, false))
    return 1;
  if (tri_check_views(who, C, 1) || tri_check_flags(who, flags) || ta_check(who, anchor, info, anchor_huber)) return 1;
  XAS_REQUIRE(huber >= 0.0 && huber < INFINITY, "%s: huber %f (needs a finite huber >= 0)", who, huber);
  XAS_REQUIRE(B == 0 || (points && P), "%s: null buffer (points and P are required)", who);
  a.pose = pose; a.betas = betas; a.trans = trans; a.vt = vt; a.sd = sd; a.pd = pd; a.skin = skin; a.parents = parents;
  a.hreg = hreg; a.rverts = rverts; a.rcount = rcount; a.tgt = nullptr; a.jw = nullptr;
  a.wp = (double)wp; a.wsh = (double)wsh; a.V = V; a.center = center;
  a.jpre = static_cast<double*>(ws); a.ws = static_cast<double*>(ws) + 1024; a.ws_stride = fit_sample_doubles(V);
  v = ViewsArgs{points, P, views, anchor, info, C, flags, huber, anchor_huber};
  return 0;
}

int views_joint_terms(const float* jreg, const float* vt, const float* sd, int V, void* ws, void* stream) {
  hipLaunchKernelGGL(smpl_fit_joint_terms_kernel, dim3((unsigned)kPreDoubles), dim3(64), 0, as_stream(stream), jreg, vt, sd, V,
                     static_cast<double*>(ws));
  XAS_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace xas

using namespace xas;

// xas_smpl_fit's layout: H is the one thing the solver keeps there; the joint blocks live in LDS.
extern "C" size_t xas_smpl_fit_views_workspace_bytes(int B, int V) {
  if (B < 0 || V < 1) return 0;
  return ((1024 + (size_t)B * fit_sample_doubles(V)) * sizeof(double) + 15) & ~(size_t)15;
}

extern "C" int xas_smpl_fit_views_linearise(const float* pose, const float* betas, const float* trans, const float* v_template,
                                            const float* shapedirs, const float* posedirs, const float* j_regressor,
                                            const float* weights, const int* parents, const float* h36m_regressor,
                                            const int* reg_verts, const int* reg_count, const float* points, const float* P,
                                            const unsigned char* views, const float* anchor, const float* info, int flags,
                                            double huber, double anchor_huber, float pose_prior, float shape_prior, int B, int V,
                                            int C, int center_idx, double* H, double* g, double* cost, double* joint_blocks,
                                            unsigned char* used, void* workspace, void* stream) {
  FitArgs a;
  ViewsArgs v;
  if (views_plan("smpl_fit_views_linearise", pose, betas, trans, v_template, shapedirs, posedirs, j_regressor, weights, parents,
                 h36m_regressor, reg_verts, reg_count, points, P, views, anchor, info, flags, huber, anchor_huber, pose_prior,
                 shape_prior, B, V, C, center_idx, workspace, a, v))
    return 1;
  if (B == 0) return 0;
  XAS_REQUIRE(H && g && cost && joint_blocks && used,
              "smpl_fit_views_linearise: null output (H, g, cost, joint_blocks and used are required)");
  if (int e = views_joint_terms(j_regressor, v_template, shapedirs, V, workspace, stream)) return e;
  hipLaunchKernelGGL(smpl_fit_views_linearise_kernel, dim3((unsigned)B), dim3(kFitThreads), 0, as_stream(stream), a, v, H, g, cost,
                     joint_blocks, used);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_smpl_fit_views(const float* pose, const float* betas, const float* trans, const float* v_template,
                                  const float* shapedirs, const float* posedirs, const float* j_regressor, const float* weights,
                                  const int* parents, const float* h36m_regressor, const int* reg_verts, const int* reg_count,
                                  const float* points, const float* P, const unsigned char* views, const float* anchor,
                                  const float* info, int flags, double huber, double anchor_huber, float pose_prior,
                                  float shape_prior, int B, int V, int C, int center_idx, int max_iters, double* pose_out,
                                  double* betas_out, double* trans_out, double* joints_out, double* cost, int* iters,
                                  unsigned char* status, unsigned char* used, void* workspace, void* stream) {
  FitArgs a;
  ViewsArgs v;
  if (views_plan("smpl_fit_views", pose, betas, trans, v_template, shapedirs, posedirs, j_regressor, weights, parents,
                 h36m_regressor, reg_verts, reg_count, points, P, views, anchor, info, flags, huber, anchor_huber, pose_prior,
                 shape_prior, B, V, C, center_idx, workspace, a, v))
    return 1;
  XAS_REQUIRE(max_iters >= 0 && max_iters <= XAS_SMPLFIT_MAX_ITERS, "smpl_fit_views: max_iters=%d trials (needs 0 <= max_iters <= %d)",
              max_iters, XAS_SMPLFIT_MAX_ITERS);
  if (B == 0) return 0;
  XAS_REQUIRE(pose_out && betas_out && trans_out && joints_out && cost && iters && status && used,
              "smpl_fit_views: null output (pose, betas, trans, joints, cost, iters, status and used are required)");
  if (int e = views_joint_terms(j_regressor, v_template, shapedirs, V, workspace, stream)) return e;
  hipLaunchKernelGGL(smpl_fit_views_kernel, dim3((unsigned)B), dim3(kFitThreads), 0, as_stream(stream), a, v, max_iters, pose_out,
                     betas_out, trans_out, joints_out, cost, iters, status, used);
  XAS_LAUNCH_CHECK();
  return 0;
}
