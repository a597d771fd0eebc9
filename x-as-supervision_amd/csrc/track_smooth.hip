// Temporal smoothing of triangulated joint tracks on the device (gfx950; eval.py --smooth, no reference counterpart): per
// (track, joint) one Levenberg-Marquardt problem over the 3 T coordinates of the joint in the T frames of the track, the
// reprojection cost of xas_triangulate_refine in every frame that has data plus a penalty on the discretised acceleration.
// include/xas_hip.h states the problem; track_band.h is its schedule, shared with track_anchor.hip; this file is the kernel
// whose data term is the reprojection term alone (TsReproj), and its entry points.
#include "track_band.h"

namespace xas {

__global__ __launch_bounds__(64) void track_smooth_kernel(TsArgs a, TsOut o, int mode) { ts_run(a, o, mode, TsReproj()); }

}  // namespace xas

using namespace xas;

extern "C" size_t xas_track_smooth_workspace_bytes(int N, int K) { return ts_workspace_bytes(N, K); }

extern "C" int xas_track_linearise(const float* points, const float* P, const float* init, const unsigned char* views,
                                   const int* start, const int* frame, int N, int V, int K, int S, int flags, float huber,
                                   double acc_w, double lambda, double* band, double* g, double* C, void* workspace, void* stream) {
  if (ts_check_linearise("track_linearise", lambda, band, g, C)) return 1;
  TsArgs a;
  if (int e = ts_plan("track_linearise", 2, points, P, init, views, start, frame, N, V, K, S, flags, huber, acc_w, workspace,
                      as_stream(stream), a))
    return e;
  TsOut o = {};
  o.band = band; o.g = g; o.C = C; o.lambda = lambda;
  hipLaunchKernelGGL(track_smooth_kernel, dim3((unsigned)(S * K)), dim3(64), 0, as_stream(stream), a, o, (int)TS_LINEARISE);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_track_smooth(const float* points, const float* P, const float* init, const unsigned char* views,
                                const int* start, const int* frame, int N, int V, int K, int S, int flags, float huber,
                                double acc_w, int max_iter, float* out, unsigned char* status, float* resid,
                                unsigned char* track_status, double* cost, int* trials, void* workspace, void* stream) {
  if (ts_check_smooth("track_smooth", init, N, K, max_iter, out)) return 1;
  TsArgs a;
  if (int e = ts_plan("track_smooth", 2, points, P, init, views, start, frame, N, V, K, S, flags, huber, acc_w, workspace,
                      as_stream(stream), a))
    return e;
  a.max_iter = max_iter;
  TsOut o = {};
  o.out = out; o.status = status; o.resid = resid; o.track_status = track_status; o.cost = cost; o.trials = trials;
  hipLaunchKernelGGL(track_smooth_kernel, dim3((unsigned)(S * K)), dim3(64), 0, as_stream(stream), a, o, (int)TS_SMOOTH);
  XAS_LAUNCH_CHECK();
  return 0;
}
