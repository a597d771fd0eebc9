// xas_smpl_fit_tracks / xas_smpl_fit_tracks_linearise: the entry points.  smplfit_tracks.h holds the kernels and states the schedule.
#include "smplfit_tracks.h"

using namespace xas;

extern "C" size_t xas_smpl_fit_tracks_workspace_bytes(int N, int V, int S) {
  if (N < 0 || V < 1 || S < 0) return 0;
  return tracks_workspace_bytes(N, V, S);
}

extern "C" int xas_smpl_fit_tracks_linearise(const float* pose, const float* betas, const float* trans, const float* v_template,
                                             const float* shapedirs, const float* posedirs, const float* j_regressor,
                                             const float* weights, const int* parents, const float* h36m_regressor,
                                             const int* reg_verts, const int* reg_count, const float* targets,
                                             const float* joint_w, const int* track, const int* frame, float pose_prior,
                                             float shape_prior, int N, int V, int S, int center_idx, double lambda,
                                             double* reduced, double* rhs, double* d_y, double* d_beta, double* track_cost,
                                             void* workspace, void* stream) {
  if (fit_check("smpl_fit_tracks_linearise", pose, betas, trans, v_template, shapedirs, posedirs, j_regressor, weights, parents,
                h36m_regressor, reg_verts, reg_count, targets, joint_w, pose_prior, shape_prior, N, V, center_idx, workspace))
    return 1;
  if (tracks_check("smpl_fit_tracks_linearise", track, frame, N, S)) return 1;
  XAS_REQUIRE(lambda >= 0.0 && lambda < INFINITY, "smpl_fit_tracks_linearise: lambda=%g (needs a finite damping >= 0)", lambda);
  if (N == 0 && S == 0) return 0;
  XAS_REQUIRE((N == 0 || d_y) && (S == 0 || (reduced && rhs && d_beta && track_cost)),
              "smpl_fit_tracks_linearise: null output (the reduced system, its right-hand side, d_y, d_beta and the cost are required)");
  XAS_REQUIRE(workspace, "smpl_fit_tracks_linearise: null buffer (the workspace is required)");
  if (N > 0 && tracks_check_ids("smpl_fit_tracks_linearise", track, N, S)) return 1;
  XAS_TRACKS_ARGS();
  if (N > 0 && S > 0) {
    XAS_TRACKS_START((double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, (unsigned char*)nullptr,
                     (double*)nullptr, lambda, 1);
    XAS_TRACKS_TRIAL(1);
  } else if (S > 0) {                                   // tracks without a sample: no frame kernel, the model arrays are not read
    hipLaunchKernelGGL(tracks_count_kernel, tgrid, dim3(256), 0, st, t);
    XAS_LAUNCH_CHECK();
    hipLaunchKernelGGL(tracks_list_kernel, tgrid, dim3(256), 0, st, t, betas, (double*)nullptr);
    XAS_LAUNCH_CHECK();
    hipLaunchKernelGGL(tracks_start_kernel, tgrid, dim3(64), 0, st, t, lambda, 1);
    XAS_LAUNCH_CHECK();
  } else {                                              // samples without a track: every one is passed through
    XAS_REQUIRE(hipMemsetAsync(d_y, 0, (size_t)N * kY * sizeof(double), st) == hipSuccess, "smpl_fit_tracks_linearise: memset failed");
    return 0;
  }
  hipLaunchKernelGGL(tracks_export_kernel, dim3(ew_grid((long)N + S, 1)), dim3(128), 0, st, t, reduced, rhs, d_y, d_beta, track_cost);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_smpl_fit_tracks(const float* pose, const float* betas, const float* trans, const float* v_template,
                                   const float* shapedirs, const float* posedirs, const float* j_regressor, const float* weights,
                                   const int* parents, const float* h36m_regressor, const int* reg_verts, const int* reg_count,
                                   const float* targets, const float* joint_w, const int* track, const int* frame,
                                   float pose_prior, float shape_prior, int N, int V, int S, int center_idx, int max_iters,
                                   double* pose_out, double* trans_out, double* joints_out, double* frame_cost,
                                   unsigned char* frame_status, double* track_betas, double* track_cost, int* track_trials,
                                   unsigned char* track_status, void* workspace, void* stream) {
  if (fit_check("smpl_fit_tracks", pose, betas, trans, v_template, shapedirs, posedirs, j_regressor, weights, parents,
                h36m_regressor, reg_verts, reg_count, targets, joint_w, pose_prior, shape_prior, N, V, center_idx, workspace))
    return 1;
  if (tracks_check("smpl_fit_tracks", track, frame, N, S)) return 1;
  XAS_REQUIRE(max_iters >= 0 && max_iters <= XAS_SMPLFIT_MAX_ITERS, "smpl_fit_tracks: max_iters=%d trials (needs 0 <= max_iters <= %d)",
              max_iters, XAS_SMPLFIT_MAX_ITERS);
  if (N == 0 && S == 0) return 0;
  XAS_REQUIRE((N == 0 || (pose_out && trans_out && joints_out && frame_cost && frame_status)) &&
                  (S == 0 || (track_betas && track_cost && track_trials && track_status)),
              "smpl_fit_tracks: null output (pose, trans, joints, frame cost and status, track betas, cost, trials and status are required)");
  XAS_REQUIRE(workspace, "smpl_fit_tracks: null buffer (the workspace is required)");
  if (N > 0 && tracks_check_ids("smpl_fit_tracks", track, N, S)) return 1;
  XAS_TRACKS_ARGS();
  if (N > 0 && S > 0) {
    XAS_TRACKS_START(pose_out, trans_out, joints_out, frame_cost, frame_status, track_betas, 1e-3, max_iters);
    for (int it = 0; it < max_iters; ++it) {
      XAS_TRACKS_TRIAL(max_iters);
      hipLaunchKernelGGL(tracks_decide_kernel, tgrid, dim3(256), 0, st, t, max_iters);
      XAS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tracks_finish_frames_kernel, dim3(ew_grid(N, 1)), dim3(128), 0, st, t, pose_out, trans_out, joints_out,
                       frame_cost, frame_status);
    XAS_LAUNCH_CHECK();
  } else if (S > 0) {
    hipLaunchKernelGGL(tracks_count_kernel, tgrid, dim3(256), 0, st, t);
    XAS_LAUNCH_CHECK();
    hipLaunchKernelGGL(tracks_list_kernel, tgrid, dim3(256), 0, st, t, betas, track_betas);
    XAS_LAUNCH_CHECK();
    hipLaunchKernelGGL(tracks_start_kernel, tgrid, dim3(64), 0, st, t, 1e-3, max_iters);
    XAS_LAUNCH_CHECK();
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
