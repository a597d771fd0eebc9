// xas_smpl_fit / xas_smpl_fit_linearise: SMPL parameters from the 18 H36M joints of a sample (include/xas_hip.h states the
// model, the residual order and the Levenberg-Marquardt schedule; tests/_smplfit_oracle.py restates them in float64 torch).
//
// One workgroup of 256 threads per sample, the whole LM in one launch.  A point is EVALUATED in three steps: the 24 Rodrigues
// rotations (one thread each, dual numbers with three tangents so that dR / d theta comes with R), the kinematic chain (one
// thread: 24 dependent 3x4 products), and a pass over the compacted vertex list in which every thread keeps partial sums of the
// 17 x 3 regressed joints, reduced by wave butterflies and then across the four waves through LDS in a fixed order.  The pass
// leaves v_posed and the blended transform of every vertex in the workspace.  A point is LINEARISED after it was evaluated: 79
// threads push one tangent each (69 body-pose angles, 10 betas) through the chain (forward mode), then the vertex pass runs
// again per chunk of kChunk tangents, reading what the evaluation left.  The derivative is exact: posedirs enters through
// dR / d theta, the betas through v_shaped AND through the joint locations of the chain.  omega and t are closed-form columns.
// The 54 x 85 Jacobian shares its LDS with the Cholesky factor (never live together); J^T J lives in the workspace, because a
// rejected trial factors it again with another damping.  No atomics; all arithmetic after the fp32 loads is double.
// The device functions live in smplfit.h, which smplfit_tracks.hip shares.
#include "smplfit.h"

namespace xas {
namespace {

__global__ __launch_bounds__(kFitThreads) void smpl_fit_linearise_kernel(FitArgs a, double* __restrict__ r, double* __restrict__ J) {
  __shared__ FitShared s;
  const int b = blockIdx.x, tid = threadIdx.x;
  double* wsb = a.ws + (size_t)b * a.ws_stride;
  fit_stage(s, a, b);
  fit_evaluate(s, a, wsb, 0, 0);
  fit_tangents(s, a, wsb, 0);
  double* rb = r + (size_t)b * kRes;
  double* Jb = J + (size_t)b * kRes * kN;
  for (int t = tid; t < kRes; t += kFitThreads)
    rb[t] = t < kRows ? s.r54[t] : (t < kRows + 69 ? sqrt(a.wp) * s.x[0][6 + t - kRows] : sqrt(a.wsh) * s.x[0][75 + t - kRows - 69]);
  for (int t = tid; t < kRes * kN; t += kFitThreads) {
    const int row = t / kN, col = t % kN;
    double v;
    if (row < kRows) v = s.m.J[t];
    else v = col == row - kRows + 6 ? (col < 75 ? sqrt(a.wp) : sqrt(a.wsh)) : 0.0;
    Jb[t] = v;
  }
}

__global__ __launch_bounds__(kFitThreads) void smpl_fit_kernel(FitArgs a, int max_iters, double* __restrict__ pose_o,
                                                               double* __restrict__ betas_o, double* __restrict__ trans_o,
                                                               double* __restrict__ joints_o, double* __restrict__ cost_o,
                                                               int* __restrict__ iters_o, unsigned char* __restrict__ status_o) {
  __shared__ FitShared s;
  const int b = blockIdx.x, tid = threadIdx.x;
  double* wsb = a.ws + (size_t)b * a.ws_stride;
  double* H = wsb + (size_t)kT * kJ * 12 + (size_t)kCache * a.V;
  const int usable = fit_stage(s, a, b);
  double C = fit_evaluate(s, a, wsb, 0, 0);
  const double C0 = C;
  int cur = 0, st = 1, it = 0;
  if (usable < 6 || !(fabs(C) < INFINITY)) {
    st = 2;
  } else if (max_iters > 0) {
    fit_tangents(s, a, wsb, 0);
    fit_assemble(s, a, H, 0);
    double lambda = 1e-3;
    while (it < max_iters) {
      ++it;
      bool accept = false;
      double Ct = 0.0, big = 0.0;
      if (fit_solve(s, H, lambda)) {
        if (tid < kN) s.x[cur ^ 1][tid] = s.x[cur][tid] + s.d[tid];
        __syncthreads();
        for (int i = 0; i < kN; ++i) big = fmax(big, fabs(s.d[i]));
        Ct = fit_evaluate(s, a, wsb, cur ^ 1, cur ^ 1);
        accept = fabs(Ct) < INFINITY && Ct < C;         // NaN never passes
      }
      if (accept) {
        cur ^= 1;
        C = Ct;
        lambda *= 0.1;
        if (big < XAS_SMPLFIT_STEP_TOL) { st = 0; break; }
        fit_tangents(s, a, wsb, cur);
        fit_assemble(s, a, H, cur);
      } else {
        lambda *= 10.0;
        if (lambda > 1e12) break;
      }
    }
  }
  __syncthreads();
  // a rejected trial left its own joints in s.Y[cur ^ 1]; s.Y[cur] belongs to s.x[cur]
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

}  // namespace
}  // namespace xas

using namespace xas;

extern "C" size_t xas_smpl_fit_workspace_bytes(int B, int V) {
  if (B < 0 || V < 1) return 0;
  return ((1024 + (size_t)B * fit_sample_doubles(V)) * sizeof(double) + 15) & ~(size_t)15;
}

#define XAS_FIT_ARGS()                                                                                                         \
  FitArgs a;                                                                                                                   \
  a.pose = pose; a.betas = betas; a.trans = trans; a.vt = v_template; a.sd = shapedirs; a.pd = posedirs; a.skin = weights;       \
  a.parents = parents; a.hreg = h36m_regressor; a.rverts = reg_verts; a.rcount = reg_count; a.tgt = targets; a.jw = joint_w;     \
  a.wp = (double)pose_prior; a.wsh = (double)shape_prior; a.V = V; a.center = center_idx;                                       \
  a.jpre = static_cast<double*>(workspace); a.ws = static_cast<double*>(workspace) + 1024; a.ws_stride = fit_sample_doubles(V); \
  hipLaunchKernelGGL(smpl_fit_joint_terms_kernel, dim3((unsigned)kPreDoubles), dim3(64), 0, as_stream(stream), j_regressor,     \
                     v_template, shapedirs, V, static_cast<double*>(workspace));                                                \
  XAS_LAUNCH_CHECK()

extern "C" int xas_smpl_fit_linearise(const float* pose, const float* betas, const float* trans, const float* v_template,
                                      const float* shapedirs, const float* posedirs, const float* j_regressor,
                                      const float* weights, const int* parents, const float* h36m_regressor,
                                      const int* reg_verts, const int* reg_count, const float* targets, const float* joint_w,
                                      float pose_prior, float shape_prior, int B, int V, int center_idx, double* r, double* J,
                                      void* workspace, void* stream) {
  if (fit_check("smpl_fit_linearise", pose, betas, trans, v_template, shapedirs, posedirs, j_regressor, weights, parents,
                h36m_regressor, reg_verts, reg_count, targets, joint_w, pose_prior, shape_prior, B, V, center_idx, workspace))
    return 1;
  if (B == 0) return 0;
  XAS_REQUIRE(r && J, "smpl_fit_linearise: null output (r and J are required)");
  XAS_FIT_ARGS();
  hipLaunchKernelGGL(smpl_fit_linearise_kernel, dim3((unsigned)B), dim3(kFitThreads), 0, as_stream(stream), a, r, J);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_smpl_fit(const float* pose, const float* betas, const float* trans, const float* v_template,
                            const float* shapedirs, const float* posedirs, const float* j_regressor, const float* weights,
                            const int* parents, const float* h36m_regressor, const int* reg_verts, const int* reg_count,
                            const float* targets, const float* joint_w, float pose_prior, float shape_prior, int B, int V,
                            int center_idx, int max_iters, double* pose_out, double* betas_out, double* trans_out,
                            double* joints_out, double* cost, int* iters, unsigned char* status, void* workspace, void* stream) {
  if (fit_check("smpl_fit", pose, betas, trans, v_template, shapedirs, posedirs, j_regressor, weights, parents, h36m_regressor,
                reg_verts, reg_count, targets, joint_w, pose_prior, shape_prior, B, V, center_idx, workspace))
    return 1;
  XAS_REQUIRE(max_iters >= 0 && max_iters <= XAS_SMPLFIT_MAX_ITERS, "smpl_fit: max_iters=%d trials (needs 0 <= max_iters <= %d)",
              max_iters, XAS_SMPLFIT_MAX_ITERS);
  if (B == 0) return 0;
  XAS_REQUIRE(pose_out && betas_out && trans_out && joints_out && cost && iters && status,
              "smpl_fit: null output (pose, betas, trans, joints, cost, iters and status are required)");
  XAS_FIT_ARGS();
  hipLaunchKernelGGL(smpl_fit_kernel, dim3((unsigned)B), dim3(kFitThreads), 0, as_stream(stream), a, max_iters, pose_out,
                     betas_out, trans_out, joints_out, cost, iters, status);
  XAS_LAUNCH_CHECK();
  return 0;
}
