// Temporal smoothing of joint tracks on 3-D anchors (gfx950; eval.py --smooth --smooth-data anchor, no reference counterpart):
// xas_track_smooth's problem with one more kind of observation per frame, a 3-D point A with a symmetric 3x3 information
// matrix W: a single camera's point on its ray (well known across the ray, poorly along it), or the point and the inverse
// covariance of a volumetric fusion.  include/xas_hip.h states the problem; track_band.h is its schedule, shared with
// track_smooth.hip; track_anchor.h is the data term (TsAnchored: the reprojection term, taken as it is, plus the anchor
// term); this file is the kernel and its entry points.  Without anchors every frame takes TsReproj's path and the sums are
// those of track_smooth.hip.
#include "track_anchor.h"

namespace xas {

__global__ __launch_bounds__(64) void track_anchor_kernel(TsArgs a, TsOut o, int mode, TsAnchored d) { ts_run(a, o, mode, d); }

}  // namespace xas

using namespace xas;

extern "C" size_t xas_track_anchor_workspace_bytes(int N, int K) { return ts_workspace_bytes(N, K); }

extern "C" int xas_track_anchor_linearise(const float* points, const float* P, const float* init, const unsigned char* views,
                                          const float* anchor, const float* info, const int* start, const int* frame, int N, int V,
                                          int K, int S, int flags, float huber, double anchor_huber, double acc_w, double lambda,
                                          double* band, double* g, double* C, void* workspace, void* stream) {
  if (ts_check_linearise("track_anchor_linearise", lambda, band, g, C)) return 1;
  if (ta_check("track_anchor_linearise", anchor, info, anchor_huber)) return 1;
  TsArgs a;
  if (int e = ts_plan("track_anchor_linearise", 1, points, P, init, views, start, frame, N, V, K, S, flags, huber, acc_w,
                      workspace, as_stream(stream), a))
    return e;
  TsOut o = {};
  o.band = band; o.g = g; o.C = C; o.lambda = lambda;
  hipLaunchKernelGGL(track_anchor_kernel, dim3((unsigned)(S * K)), dim3(64), 0, as_stream(stream), a, o, (int)TS_LINEARISE,
                     TsAnchored{anchor, info, anchor_huber});
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_track_anchor_smooth(const float* points, const float* P, const float* init, const unsigned char* views,
                                       const float* anchor, const float* info, const int* start, const int* frame, int N, int V,
                                       int K, int S, int flags, float huber, double anchor_huber, double acc_w, int max_iter,
                                       float* out, unsigned char* status, float* resid, unsigned char* track_status, double* cost,
                                       int* trials, void* workspace, void* stream) {
  if (ts_check_smooth("track_anchor_smooth", init, N, K, max_iter, out)) return 1;
  if (ta_check("track_anchor_smooth", anchor, info, anchor_huber)) return 1;
  TsArgs a;
  if (int e = ts_plan("track_anchor_smooth", 1, points, P, init, views, start, frame, N, V, K, S, flags, huber, acc_w, workspace,
                      as_stream(stream), a))
    return e;
  a.max_iter = max_iter;
  TsOut o = {};
  o.out = out; o.status = status; o.resid = resid; o.track_status = track_status; o.cost = cost; o.trials = trials;
  hipLaunchKernelGGL(track_anchor_kernel, dim3((unsigned)(S * K)), dim3(64), 0, as_stream(stream), a, o, (int)TS_SMOOTH,
                     TsAnchored{anchor, info, anchor_huber});
  XAS_LAUNCH_CHECK();
  return 0;
}
