// xas_smpl_fit_tracks / xas_smpl_fit_tracks_linearise: xas_smpl_fit's problem over whole tracks, one beta vector per track and
// pose and translation per frame (include/xas_hip.h states the cost and the schedule; tests/_smplfit_tracks_oracle.py restates
// them in float64 torch).  The device functions that evaluate and linearise a frame are smplfit.h's, unchanged.
//
// The normal equations of a track are an arrowhead: a 75 x 75 block per frame, a 75 x 10 border per frame, a 10 x 10 corner.
// The betas are the last 10 unknowns of a frame's 85, so the Cholesky of a frame's damped 85 x 85 matrix, stopped after column
// 75, leaves L11, L21 and the frame's share of the reduced 10 x 10 system (its Schur complement) in place, and the forward
// substitution stopped at row 75 leaves the frame's share of the reduced right-hand side.  A TRIAL is four launches on one stream:
//   eliminate     frame kernel: (after an accepted trial: evaluate, tangents, assemble H and g) factor 75 columns at the
//                 track's lambda -> F (L11, L21, Schur corner), z (forward-substituted -g)
//   shape step    track kernel: sum the corners and the reduced right-hand sides over the track's usable frames in ascending
//                 frame order, finish the Cholesky and both substitutions on the 10 x 10 -> d beta
//   back-subst.   frame kernel: d y from L11, L21, z and d beta; evaluate the cost at the trial point
//   decide        track kernel: sum the trial costs in frame order, accept or reject, lambda, status, trial count, step norm
// All launches of max_iters trials are enqueued up front; a finished track and its frames do nothing in the later ones.
// Every operation of the three solves is the one fit_solve would make on the 85 x 85 matrix, in its order, so a track of one
// frame repeats xas_smpl_fit bit for bit.  The damping lambda diag(H) of the corner is therefore added per frame, before the
// frame's Schur complement is taken (the sum over frames of lambda diag(H_t) is lambda times the diagonal of the sum).
// Frame kernels run a bounded grid that strides over the frames: the vertex cache and the tangent transforms (smplfit.h's
// per-sample scratch, about 1 MB at V = 6890) exist once per WORKGROUP and are refilled by fit_evaluate before every use; only
// the small state below is per frame.  No atomics; every sum has a fixed order that does not depend on where a sample sits in N.
//
// This header holds what smplfit_tracks.hip and smplfit_smooth.hip (the same problem with an acceleration prior over the frames)
// share, each piece once: the state's layout, TrackArgs, the set-up kernels, the trial kernels of the arrowhead, the finish
// kernels, the workspace's carving and the host checks.  TrackArgs::smooth is 0 for xas_smpl_fit_tracks, whose launches and
// arithmetic are what they were.
#pragma once
#include "smplfit.h"

namespace xas {
namespace {

constexpr int kY = 75, kBeta = 10, kCorner = kBeta * (kBeta + 1) / 2;
constexpr int kTrackGrid = 512;                          // workgroups of a frame kernel: two per CU (LDS) on 256 CUs
// per frame, doubles
constexpr int oY = 0, oYt = oY + kY, oH = oYt + kY, oF = oH + kTri, oG = oF + kTri, oZ = oG + kN, oJ = oZ + kN, oJt = oJ + kRows,
              oC = oJt + kRows;                          // oC: cost at the track's start, now, at the trial; largest |d y|
constexpr int kFrameD = oC + 4;
// per track, doubles
constexpr int tBeta = 0, tBetaT = 10, tDBeta = 20, tA = 30, tRhs = tA + kCorner, tC0 = tRhs + kBeta, tC = tC0 + 1, tLambda = tC + 1,
              tBig = tLambda + 1;
constexpr int kTrackD = 104;
static_assert(tBig < kTrackD, "track state");
// per track, ints
enum { iCount, iOffset, iUsable, iTrials, iStatus, iDone, iRelin, iOk, iFramesOk, kTrackI };   // iOk: the trial step exists; iFramesOk: every frame was eliminated
constexpr int kStConverged = 0, kStLimit = 1, kStNoFrame = 2;

struct TrackArgs {
  const int *track, *frame;                             // [N]
  double *fr, *tk;                                      // per-frame and per-track doubles
  int *usable, *fok, *tmp, *list, *ti;                  // [N] x 4, [S][kTrackI]
  double* scratch;                                      // per workgroup: fit_sample_doubles(V) - kTri are used
  size_t scratch_stride;
  int N, S;
  int smooth;                                           // smplfit_smooth.hip: 1 = a frame that repeats a frame number is passed through
  double* fac;                                          // smplfit_smooth.hip: the factor, per frame
};

size_t tracks_grid(int N) { return (size_t)(N < kTrackGrid ? N : kTrackGrid); }
size_t tracks_scratch_doubles(int V) { return (size_t)kT * kJ * 12 + (size_t)kCache * V; }

__device__ __forceinline__ double* frame_of(const TrackArgs& t, int f) { return t.fr + (size_t)f * kFrameD; }
__device__ __forceinline__ double* scratch_of(const TrackArgs& t) { return t.scratch + (size_t)blockIdx.x * t.scratch_stride; }

// s.x[0] = (the frame's y, its track's beta); fit_stage filled the rest of the sample
__device__ __forceinline__ void load_point(FitShared& s, const TrackArgs& t, int f, int trk) {
  const int tid = threadIdx.x;
  if (tid < kY) s.x[0][tid] = frame_of(t, f)[oY + tid];
  else if (tid < kN) s.x[0][tid] = t.tk[(size_t)trk * kTrackD + tBeta + tid - kY];
  __syncthreads();
}

// Every frame at its own init, as xas_smpl_fit sees it: usable or passed through (then its outputs are final here).
__global__ __launch_bounds__(kFitThreads) void tracks_init_frames_kernel(FitArgs a, TrackArgs t, double* __restrict__ pose_o,
                                                                         double* __restrict__ trans_o, double* __restrict__ joints_o,
                                                                         double* __restrict__ cost_o, unsigned char* __restrict__ status_o) {
  __shared__ FitShared s;
  const int tid = threadIdx.x;
  double* wsb = scratch_of(t);
  for (int f = blockIdx.x; f < t.N; f += gridDim.x) {
    const int joints = fit_stage(s, a, f);
    const double C = fit_evaluate(s, a, wsb, 0, 0);
    const bool ok = joints >= 6 && fabs(C) < INFINITY && (unsigned)t.track[f] < (unsigned)t.S;
    double* fr = frame_of(t, f);
    if (tid < kY) fr[oY + tid] = s.x[0][tid];
    if (tid == 255) t.usable[f] = ok ? 1 : 0;
    if ((!ok || t.smooth) && pose_o) {                  // smooth: of every frame, the list kernel may yet pass a usable one through
      const double* x = s.x[0];
      if (tid < 72) pose_o[(size_t)f * 72 + tid] = tid < 3 ? x[tid] : x[tid + 3];
      if (tid >= 82 && tid < 85) trans_o[(size_t)f * 3 + tid - 82] = x[3 + tid - 82];
      if (tid >= 128 && tid < 128 + kRows) joints_o[(size_t)f * kRows + tid - 128] = s.Y[0][tid - 128];
      if (tid == 255) {
        cost_o[(size_t)f * 2] = C;
        cost_o[(size_t)f * 2 + 1] = C;
        status_o[f] = 2;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void tracks_count_kernel(TrackArgs t) {
  __shared__ int part[256];
  const int trk = blockIdx.x, tid = threadIdx.x;
  int n = 0;
  for (int i = tid; i < t.N; i += 256) n += t.track[i] == trk ? 1 : 0;
  part[tid] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) t.ti[(size_t)trk * kTrackI + iCount] = part[0];
}

// The track's samples, sorted by frame (a frame held twice: by sample index) -> list[offset ..); its starting beta.
// One workgroup per track: the members are found in one pass over N and ranked against each other, count^2 / 256 comparisons
// per thread, and the offset is a serial sum over the tracks before.  Sized for tracks of hundreds to a few thousand frames.
__global__ __launch_bounds__(256) void tracks_list_kernel(TrackArgs t, const float* __restrict__ betas, double* __restrict__ betas_o) {
  __shared__ int wcnt[4], base, offset;
  const int trk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int* ti = t.ti + (size_t)trk * kTrackI;
  if (tid == 0) {
    int o = 0;
    for (int k = 0; k < trk; ++k) o += t.ti[(size_t)k * kTrackI + iCount];
    offset = o;
    base = 0;
  }
  __syncthreads();
  const int count = ti[iCount];
  int* tmp = t.tmp + offset;
  int* list = t.list + offset;
  for (int i0 = 0; i0 < t.N; i0 += 256) {                 // ordered compaction, 256 samples at a time
    const int i = i0 + tid;
    const bool m = i < t.N && t.track[i] == trk;
    const unsigned long long bal = __ballot(m);
    if (lane == 0) wcnt[wid] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wid; ++w) off += wcnt[w];
    if (m) tmp[off + __popcll(bal & ((1ull << lane) - 1ull))] = i;
    __syncthreads();
    if (tid == 0) base += ((wcnt[0] + wcnt[1]) + wcnt[2]) + wcnt[3];
    __syncthreads();
  }
  for (int k = tid; k < count; k += 256) {                // rank sort
    const int i = tmp[k], fi = t.frame[i];
    int r = 0;
    for (int q = 0; q < count; ++q) {
      const int j = tmp[q], fj = t.frame[j];
      r += (fj < fi || (fj == fi && j < i)) ? 1 : 0;
    }
    list[r] = i;
  }
  __syncthreads();
  if (t.smooth) {                                         // a usable frame with the number of the usable frame before it: passed through
    if (tid == 0) {
      int last = 0, have = 0;
      for (int k = 0; k < count; ++k) {
        const int i = list[k];
        if (!t.usable[i]) continue;
        if (have && t.frame[i] == last) t.usable[i] = 0;
        else last = t.frame[i], have = 1;
      }
    }
    __syncthreads();
  }
  if (tid < kBeta) {
    double sum = 0.0, all = 0.0;
    int n = 0;
    for (int k = 0; k < count; ++k) {
      const int i = list[k];
      const double b = (double)betas[(size_t)i * 10 + tid];
      all += b;
      if (t.usable[i]) {
        sum += b;
        ++n;
      }
    }
    const double v = n > 0 ? sum / (double)n : (count > 0 ? all / (double)count : 0.0);
    t.tk[(size_t)trk * kTrackD + tBeta + tid] = v;
    if (n == 0 && betas_o) betas_o[(size_t)trk * 10 + tid] = v;
    if (tid == 0) {
      ti[iOffset] = offset;
      ti[iUsable] = n;
    }
  }
}

// The usable frames at (their y, the track's starting beta): the cost and the joints there.
__global__ __launch_bounds__(kFitThreads) void tracks_start_frames_kernel(FitArgs a, TrackArgs t) {
  __shared__ FitShared s;
  const int tid = threadIdx.x;
  double* wsb = scratch_of(t);
  for (int f = blockIdx.x; f < t.N; f += gridDim.x) {
    if (!t.usable[f]) continue;
    fit_stage(s, a, f);
    load_point(s, t, f, t.track[f]);
    const double C = fit_evaluate(s, a, wsb, 0, 0);
    double* fr = frame_of(t, f);
    if (tid < kRows) fr[oJ + tid] = s.Y[0][tid];
    if (tid == 255) fr[oC] = fr[oC + 1] = C;
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void tracks_start_kernel(TrackArgs t, double lambda0, int max_iters) {
  const int trk = blockIdx.x;
  if (threadIdx.x != 0) return;
  int* ti = t.ti + (size_t)trk * kTrackI;
  double* tk = t.tk + (size_t)trk * kTrackD;
  const int* list = t.list + ti[iOffset];
  double C = 0.0;
  for (int k = 0; k < ti[iCount]; ++k)
    if (t.usable[list[k]]) C += frame_of(t, list[k])[oC];
  tk[tC0] = tk[tC] = C;
  tk[tLambda] = lambda0;
  tk[tBig] = 0.0;
  ti[iTrials] = 0;
  ti[iStatus] = ti[iUsable] > 0 ? kStLimit : kStNoFrame;
  ti[iDone] = (ti[iUsable] == 0 || max_iters == 0) ? 1 : 0;
  ti[iRelin] = 1;
  ti[iOk] = 0;
  ti[iFramesOk] = 0;
}

// fit_solve's Cholesky of H + lambda diag(H), stopped after column 75, and its forward substitution stopped at row 75:
// F = L11, L21 and the Schur corner (packed like H), z = the substituted -g (rows 75.. : the reduced right-hand side).
// false at a pivot that is not > 0.  Uniform over the block.
__device__ __noinline__ bool tracks_eliminate(FitShared& s, const double* H, double lambda, double* F, double* z) {
  const int tid = threadIdx.x;
  double* L = s.m.L;
  for (int j = 0; j < kY; ++j) {
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
  if (tid < kCorner) {                                  // what columns 75.. of fit_solve hold after their first 75 terms
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= tid) ++i;
    const int j = tid - i * (i + 1) / 2, r = kY + i, c = kY + j;
    double v = H[tri(r, c)];
    if (r == c) v += lambda * v;
    for (int k = 0; k < kY; ++k) v -= L[tri(r, k)] * L[tri(c, k)];
    F[tri(r, c)] = v;
  }
  for (int e = tid; e < tri(kY, 0); e += kFitThreads) F[e] = L[e];
  if (tid >= kY && tid < kN)
    for (int k = 0; k < kY; ++k) F[tri(tid, k)] = L[tri(tid, k)];
  if (tid < kN) s.d[tid] = -s.g[tid];
  for (int j = 0; j < kY; ++j) {
    __syncthreads();
    if (tid == j) s.d[j] = s.d[j] / L[tri(j, j)];
    __syncthreads();
    if (tid > j && tid < kN) s.d[tid] -= L[tri(tid, j)] * s.d[j];
  }
  __syncthreads();
  if (tid < kN) z[tid] = s.d[tid];
  __syncthreads();
  return true;
}

__global__ __launch_bounds__(kFitThreads) void tracks_eliminate_kernel(FitArgs a, TrackArgs t) {
  __shared__ FitShared s;
  const int tid = threadIdx.x;
  double* wsb = scratch_of(t);
  for (int f = blockIdx.x; f < t.N; f += gridDim.x) {
    if (!t.usable[f]) continue;
    const int trk = t.track[f];
    const int* ti = t.ti + (size_t)trk * kTrackI;
    if (ti[iDone]) continue;
    double* fr = frame_of(t, f);
    if (ti[iRelin]) {                                   // the point moved (or this is the first trial): linearise there
      fit_stage(s, a, f);
      load_point(s, t, f, trk);
      fit_evaluate(s, a, wsb, 0, 0);
      fit_tangents(s, a, wsb, 0);
      fit_assemble(s, a, fr + oH, 0);
      if (tid < kN) fr[oG + tid] = s.g[tid];
    } else {
      if (tid < kN) s.g[tid] = fr[oG + tid];
    }
    __syncthreads();
    const bool ok = tracks_eliminate(s, fr + oH, t.tk[(size_t)trk * kTrackD + tLambda], fr + oF, fr + oZ);
    if (tid == 0) t.fok[f] = ok ? 1 : 0;
    __syncthreads();
  }
}

// The reduced system of a track: corners and right-hand sides summed in frame order, then columns 75.. of fit_solve.
__global__ __launch_bounds__(128) void tracks_shape_step_kernel(TrackArgs t) {
  __shared__ double A[kCorner], L[kCorner], d[kBeta];
  __shared__ int allok;
  const int trk = blockIdx.x, tid = threadIdx.x;
  int* ti = t.ti + (size_t)trk * kTrackI;
  if (ti[iDone]) return;
  double* tk = t.tk + (size_t)trk * kTrackD;
  const int* list = t.list + ti[iOffset];
  const int count = ti[iCount];
  if (tid < kCorner) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= tid) ++i;
    const int j = tid - i * (i + 1) / 2, e = tri(kY + i, kY + j);
    double v = 0.0;
    for (int k = 0; k < count; ++k)
      if (t.usable[list[k]]) v += frame_of(t, list[k])[oF + e];
    A[tid] = v;
    tk[tA + tid] = v;
  } else if (tid >= 64 && tid < 64 + kBeta) {
    double v = 0.0;
    for (int k = 0; k < count; ++k)
      if (t.usable[list[k]]) v += frame_of(t, list[k])[oZ + kY + tid - 64];
    d[tid - 64] = v;
    tk[tRhs + tid - 64] = v;
  } else if (tid == 127) {
    int ok = 1;
    for (int k = 0; k < count; ++k)
      if (t.usable[list[k]] && !t.fok[list[k]]) ok = 0;
    allok = ok;
  }
  __syncthreads();
  if (tid != 0) return;
  bool ok = allok != 0;
  ti[iFramesOk] = allok;                                // 0: a frame left no factor, the sums above hold nothing of meaning
  for (int j = 0; j < kBeta && ok; ++j) {
    for (int i = j; i < kBeta; ++i) {
      double v = A[tri(i, j)];
      for (int k = 0; k < j; ++k) v -= L[tri(i, k)] * L[tri(j, k)];
      if (i == j) {
        if (!(v > 0.0)) {
          ok = false;
          break;
        }
        L[tri(j, j)] = sqrt(v);
      } else {
        L[tri(i, j)] = v / L[tri(j, j)];
      }
    }
  }
  if (ok) {
    for (int j = 0; j < kBeta; ++j) {
      d[j] = d[j] / L[tri(j, j)];
      for (int i = j + 1; i < kBeta; ++i) d[i] -= L[tri(i, j)] * d[j];
    }
    for (int j = kBeta - 1; j >= 0; --j) {
      d[j] = d[j] / L[tri(j, j)];
      for (int i = 0; i < j; ++i) d[i] -= L[tri(j, i)] * d[j];
    }
    double big = 0.0;
    for (int q = 0; q < kBeta; ++q) {
      tk[tDBeta + q] = d[q];
      tk[tBetaT + q] = tk[tBeta + q] + d[q];
      big = fmax(big, fabs(d[q]));
    }
    tk[tBig] = big;
  }
  ti[iOk] = ok ? 1 : 0;
}

// d y of a frame (the rows under 75 of fit_solve's backward substitution), the trial point and its cost.
__global__ __launch_bounds__(kFitThreads) void tracks_backsub_kernel(FitArgs a, TrackArgs t) {
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
    load_point(s, t, f, trk);
    double* L = s.m.L;
    for (int e = tid; e < kTri; e += kFitThreads) L[e] = fr[oF + e];
    if (tid < kY) s.d[tid] = fr[oZ + tid];
    else if (tid < kN) s.d[tid] = t.tk[(size_t)trk * kTrackD + tDBeta + tid - kY];
    __syncthreads();
    if (tid < kY)
      for (int j = kN - 1; j >= kY; --j) s.d[tid] -= L[tri(j, tid)] * s.d[j];
    for (int j = kY - 1; j >= 0; --j) {
      __syncthreads();
      if (tid == j) s.d[j] = s.d[j] / L[tri(j, j)];
      __syncthreads();
      if (tid < j) s.d[tid] -= L[tri(j, tid)] * s.d[j];
    }
    __syncthreads();
    if (tid < kN) s.x[1][tid] = s.x[0][tid] + s.d[tid];
    __syncthreads();
    const double Ct = fit_evaluate(s, a, wsb, 1, 1);
    if (tid < kY) {
      fr[oYt + tid] = s.x[1][tid];
      fr[oZ + tid] = s.d[tid];                          // z is spent: the slot now holds d y (xas_smpl_fit_tracks_linearise)
    }
    if (tid >= 128 && tid < 128 + kRows) fr[oJt + tid - 128] = s.Y[1][tid - 128];
    if (tid == 255) {
      double big = 0.0;
      for (int i = 0; i < kY; ++i) big = fmax(big, fabs(s.d[i]));
      fr[oC + 2] = Ct;
      fr[oC + 3] = big;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void tracks_decide_kernel(TrackArgs t, int max_iters) {
  __shared__ int accept;
  const int trk = blockIdx.x, tid = threadIdx.x;
  int* ti = t.ti + (size_t)trk * kTrackI;
  if (ti[iDone]) return;
  double* tk = t.tk + (size_t)trk * kTrackD;
  const int* list = t.list + ti[iOffset];
  const int count = ti[iCount];
  if (tid == 0) {
    bool acc = false;
    double Ct = 0.0, big = tk[tBig];
    if (ti[iOk]) {
      for (int k = 0; k < count; ++k)
        if (t.usable[list[k]]) {
          const double* fr = frame_of(t, list[k]);
          Ct += fr[oC + 2];
          big = fmax(big, fr[oC + 3]);
        }
      acc = fabs(Ct) < INFINITY && Ct < tk[tC];         // NaN never passes
    }
    accept = acc ? 1 : 0;
    const int it = ti[iTrials] + 1;
    ti[iTrials] = it;
    int done = 0;
    if (acc) {
      tk[tC] = Ct;
      tk[tLambda] *= 0.1;
      if (big < XAS_SMPLFIT_STEP_TOL) {
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
  for (int k = 0; k < count; ++k) {
    if (!t.usable[list[k]]) continue;
    double* fr = frame_of(t, list[k]);
    if (tid < kY) fr[oY + tid] = fr[oYt + tid];
    else if (tid >= 128 && tid < 128 + kRows) fr[oJ + tid - 128] = fr[oJt + tid - 128];
    else if (tid == 255) fr[oC + 1] = fr[oC + 2];
  }
}

__global__ __launch_bounds__(128) void tracks_finish_frames_kernel(TrackArgs t, double* __restrict__ pose_o, double* __restrict__ trans_o,
                                                                   double* __restrict__ joints_o, double* __restrict__ cost_o,
                                                                   unsigned char* __restrict__ status_o) {
  const int tid = threadIdx.x;
  for (int f = blockIdx.x; f < t.N; f += gridDim.x) {
    if (!t.usable[f]) continue;
    const double* fr = frame_of(t, f);
    if (tid < 72) pose_o[(size_t)f * 72 + tid] = fr[oY + (tid < 3 ? tid : tid + 3)];
    else if (tid < 75) trans_o[(size_t)f * 3 + tid - 72] = fr[oY + 3 + tid - 72];
    if (tid >= 64 && tid < 64 + kRows) joints_o[(size_t)f * kRows + tid - 64] = fr[oJ + tid - 64];
    if (tid == 127) {
      cost_o[(size_t)f * 2] = fr[oC];
      cost_o[(size_t)f * 2 + 1] = fr[oC + 1];
      status_o[f] = 0;
    }
  }
}

__global__ __launch_bounds__(64) void tracks_finish_kernel(TrackArgs t, double* __restrict__ betas_o, double* __restrict__ cost_o,
                                                           int* __restrict__ trials_o, unsigned char* __restrict__ status_o) {
  const int trk = blockIdx.x, tid = threadIdx.x;
  const int* ti = t.ti + (size_t)trk * kTrackI;
  const double* tk = t.tk + (size_t)trk * kTrackD;
  if (tid < kBeta && ti[iUsable] > 0) betas_o[(size_t)trk * 10 + tid] = tk[tBeta + tid];
  if (tid == 63) {
    cost_o[(size_t)trk * 2] = tk[tC0];
    cost_o[(size_t)trk * 2 + 1] = tk[tC];
    trials_o[trk] = ti[iTrials];
    status_o[trk] = (unsigned char)ti[iStatus];
  }
}

// What one trial at the given lambda left: the summed, damped reduced system, its right-hand side, the step and C_s.
__global__ __launch_bounds__(128) void tracks_export_kernel(TrackArgs t, double* __restrict__ A_o, double* __restrict__ rhs_o,
                                                            double* __restrict__ dy_o, double* __restrict__ dbeta_o,
                                                            double* __restrict__ cost_o) {
  const int tid = threadIdx.x;
  for (int b = blockIdx.x; b < t.N + t.S; b += gridDim.x) {
    if (b < t.N) {
      const int f = b, trk = t.track[f];
      const bool on = t.usable[f] && t.ti[(size_t)trk * kTrackI + iOk];
      if (tid < kY) dy_o[(size_t)f * kY + tid] = on ? frame_of(t, f)[oZ + tid] : 0.0;
    } else {
      const int trk = b - t.N;
      const int* ti = t.ti + (size_t)trk * kTrackI;
      const double* tk = t.tk + (size_t)trk * kTrackD;
      const bool on = ti[iUsable] > 0 && ti[iFramesOk];
      if (tid < 100) {
        const int i = tid / 10, j = tid % 10;
        A_o[(size_t)trk * 100 + tid] = on ? tk[tA + (i >= j ? tri(i, j) : tri(j, i))] : 0.0;
      } else if (tid < 110) {
        rhs_o[(size_t)trk * 10 + tid - 100] = on ? tk[tRhs + tid - 100] : 0.0;
      } else if (tid < 120) {
        dbeta_o[(size_t)trk * 10 + tid - 110] = ti[iUsable] > 0 && ti[iOk] ? tk[tDBeta + tid - 110] : 0.0;
      } else if (tid == 120) {
        cost_o[trk] = tk[tC0];
      }
    }
  }
}

size_t tracks_workspace_bytes(int N, int V, int S) {
  size_t b = align16(1024 * sizeof(double));
  b += align16(tracks_grid(N) * tracks_scratch_doubles(V) * sizeof(double));
  b += align16((size_t)N * kFrameD * sizeof(double));
  b += align16((size_t)S * kTrackD * sizeof(double));
  b += align16(((size_t)N * 4 + (size_t)S * kTrackI) * sizeof(int));
  return b;
}

// true if the host may read p: not known to the runtime (plain host memory), pinned or managed
bool host_visible(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return true;
  }
  return at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeArray;
}

int tracks_check(const char* who, const int* track, const int* frame, int N, int S) {
  XAS_REQUIRE(S >= 0, "%s: S=%d tracks (needs S >= 0)", who, S);
  XAS_REQUIRE(N == 0 || (track && frame), "%s: null buffer (track and frame are required)", who);
  return 0;
}

// after every other check: the only one that reads an array
int tracks_check_ids(const char* who, const int* track, int N, int S) {
  if (!host_visible(track)) return 0;                   // on the device: a frame of a track outside [0, S) is passed through
  for (int i = 0; i < N; ++i)
    XAS_REQUIRE(track[i] >= 0 && track[i] < S, "%s: track[%d] = %d (needs 0 <= track < S = %d)", who, i, track[i], S);
  return 0;
}

}  // namespace
}  // namespace xas

#define XAS_TRACKS_ARGS()                                                                                                      \
  FitArgs a;                                                                                                                   \
  a.pose = pose; a.betas = betas; a.trans = trans; a.vt = v_template; a.sd = shapedirs; a.pd = posedirs; a.skin = weights;       \
  a.parents = parents; a.hreg = h36m_regressor; a.rverts = reg_verts; a.rcount = reg_count; a.tgt = targets; a.jw = joint_w;     \
  a.wp = (double)pose_prior; a.wsh = (double)shape_prior; a.V = V; a.center = center_idx;                                       \
  a.jpre = static_cast<double*>(workspace); a.ws = nullptr; a.ws_stride = 0;                                                    \
  TrackArgs t;                                                                                                                 \
  {                                                                                                                            \
    char* p = static_cast<char*>(workspace) + align16(1024 * sizeof(double));                                                  \
    t.scratch = reinterpret_cast<double*>(p);                                                                                  \
    t.scratch_stride = tracks_scratch_doubles(V);                                                                              \
    p += align16(tracks_grid(N) * tracks_scratch_doubles(V) * sizeof(double));                                                 \
    t.fr = reinterpret_cast<double*>(p);                                                                                       \
    p += align16((size_t)N * kFrameD * sizeof(double));                                                                        \
    t.tk = reinterpret_cast<double*>(p);                                                                                       \
    p += align16((size_t)S * kTrackD * sizeof(double));                                                                        \
    t.usable = reinterpret_cast<int*>(p);                                                                                      \
    t.fok = t.usable + N; t.tmp = t.fok + N; t.list = t.tmp + N; t.ti = t.list + N;                                            \
  }                                                                                                                            \
  t.track = track; t.frame = frame; t.N = N; t.S = S; t.smooth = 0; t.fac = nullptr;                                           \
  const hipStream_t st = as_stream(stream);                                                                                    \
  const dim3 fgrid((unsigned)tracks_grid(N)), tgrid((unsigned)S)

// j_regressor . v_template and j_regressor . shapedirs, before the first frame kernel (N >= 1: fit_check saw the model arrays)
#define XAS_TRACKS_JOINT_TERMS()                                                                                               \
  hipLaunchKernelGGL(smpl_fit_joint_terms_kernel, dim3((unsigned)kPreDoubles), dim3(64), 0, st, j_regressor, v_template,        \
                     shapedirs, V, static_cast<double*>(workspace));                                                            \
  XAS_LAUNCH_CHECK()

// the launches up to the start of the first trial (S >= 1, N >= 1)
#define XAS_TRACKS_START(pose_o, trans_o, joints_o, cost_o, status_o, betas_o, lambda0, iters)                                 \
  XAS_TRACKS_JOINT_TERMS();                                                                                                    \
  hipLaunchKernelGGL(tracks_init_frames_kernel, fgrid, dim3(kFitThreads), 0, st, a, t, pose_o, trans_o, joints_o, cost_o,      \
                     status_o);                                                                                                \
  XAS_LAUNCH_CHECK();                                                                                                          \
  hipLaunchKernelGGL(tracks_count_kernel, tgrid, dim3(256), 0, st, t);                                                         \
  XAS_LAUNCH_CHECK();                                                                                                          \
  hipLaunchKernelGGL(tracks_list_kernel, tgrid, dim3(256), 0, st, t, betas, betas_o);                                          \
  XAS_LAUNCH_CHECK();                                                                                                          \
  hipLaunchKernelGGL(tracks_start_frames_kernel, fgrid, dim3(kFitThreads), 0, st, a, t);                                       \
  XAS_LAUNCH_CHECK();                                                                                                          \
  hipLaunchKernelGGL(tracks_start_kernel, tgrid, dim3(64), 0, st, t, lambda0, iters);                                          \
  XAS_LAUNCH_CHECK()

#define XAS_TRACKS_TRIAL(iters)                                                                                                \
  hipLaunchKernelGGL(tracks_eliminate_kernel, fgrid, dim3(kFitThreads), 0, st, a, t);                                          \
  XAS_LAUNCH_CHECK();                                                                                                          \
  hipLaunchKernelGGL(tracks_shape_step_kernel, tgrid, dim3(128), 0, st, t);                                                    \
  XAS_LAUNCH_CHECK();                                                                                                          \
  hipLaunchKernelGGL(tracks_backsub_kernel, fgrid, dim3(kFitThreads), 0, st, a, t);                                            \
  XAS_LAUNCH_CHECK()

