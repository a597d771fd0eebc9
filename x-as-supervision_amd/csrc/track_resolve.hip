// Depth hypothesis and left/right exchange chosen over time on the device (gfx950; eval.py --resolve-track, no reference
// counterpart): per (track, unit) an exact Viterbi pass over the frames of the track.  A unit is a left/right pair of joints
// (state = exchange bit and one hypothesis per joint, 2 Hy^2 states) or a joint without a partner (state = hypothesis, Hy
// states).  include/xas_hip.h states the cost and the rules; this file is its schedule.
// One wave per (track, unit), one launch, four passes of the same wave:
//   1 usable   lanes stride the frames: is every candidate of the unit finite?  One byte per frame into PATH; fewer than two
//              usable frames and the unit is passed through.
//   2 forward  serial over the usable frames, lane = destination state.  The candidates of this frame and of the usable frame
//              before it sit in LDS as doubles.  The motion term separates per joint: two (2 Hy) x (2 Hy) tables of
//              vel_w / gap * squared distance are filled once per frame (lanes stride their entries), and a state pair costs
//              two table reads and the previous forward value, an LDS broadcast.  Predecessors are tried in ascending index and
//              replaced on strictly smaller only: ties go to the smallest.  The back-pointer goes to BACK, one byte per
//              frame and state.  The next frame's inputs are loaded before this frame's work: a cache latency per frame hides.
//   3 back     the end state is the smallest forward value (ties to the smallest index), the same on every lane.  Eight frames'
//              rows of BACK are loaded at once, lane = state, before any is needed; the chain itself is one cross-lane read
//              per frame.  Lane 0 writes the frame's state over its byte of PATH.
//   4 outputs  lanes stride the frames again: decode the byte, gather from kps, write.
// Every value a branch depends on is the same on all lanes, so the wave never diverges round a barrier.  A byte of the
// workspace is read only after this launch wrote it (rows of BACK of unusable frames are loaded and never used): the outputs do
// not depend on what the workspace held.
#include <math.h>

#include "track_start.h"

namespace xas {

constexpr int kTrHy = XAS_TRACK_MAX_HYPO, kTrK = XAS_TRACK_MAX_JOINTS, kTrCand = 2 * kTrHy;
constexpr int kTrPassed = 0xff;                                       // PATH: the frame is not usable (a state is < 64)
static_assert(2 * kTrHy * kTrHy <= kWave, "a pair's states must fit the lanes of one wave");

struct TrArgs {
  const float *kps, *world, *unary;
  const int *frame, *start;                                           // start: the workspace's copy of the host array
  unsigned char *back, *path;                                         // workspace: [N][K][2 Hy^2] and [N][K] bytes
  int N, Hy, K, U;
  double vel_w, hyp_w, swap_w;
  unsigned char perm[kTrK], lead[kTrK];                               // lead[u]: the joint k <= perm[k] of unit u
};
struct TrOut {
  float* sel;
  unsigned char *hyp, *swap, *status;
  double* cost;
};

// State j of a unit: exchange bit, hypothesis of the first and of the second joint.
struct TrState {
  int e, h0, h1;
};
__device__ __forceinline__ TrState tr_state(int j, int Hy, bool pair) {
  if (!pair) return TrState{0, j, 0};
  return TrState{j / (Hy * Hy), (j / Hy) % Hy, j % Hy};
}

__global__ __launch_bounds__(64) void track_resolve_kernel(TrArgs a, TrOut o) {
  // [buffer][channel][hypothesis]: the unit's channels are its joints as the detector numbered them, 0 = lead, 1 = partner
  __shared__ double s_pos[2][2][kTrHy][3], s_un[2][2][kTrHy];
  __shared__ double s_alpha[2][kWave];                                // [buffer][state]: the forward values
  __shared__ double s_tab[2][kTrCand * kTrCand];                      // [joint][candidate before][candidate now]
  const int p = blockIdx.x, s = p / a.U, u = p - s * a.U, lane = threadIdx.x;
  const int ja = a.lead[u], jb = a.perm[ja], Hy = a.Hy, K = a.K;
  const bool pair = jb != ja;
  const int nch = pair ? 2 : 1, nc = nch * Hy, ns = pair ? 2 * Hy * Hy : Hy;
  const int n0 = a.start[s], T = a.start[s + 1] - n0;
  unsigned char* back = a.back + ((size_t)n0 * K + (size_t)ja * T) * (size_t)(2 * Hy * Hy);
  unsigned char* path = a.path + (size_t)n0 * K + (size_t)ja * T;
  const auto at = [&](int n, int h, int k) { return ((size_t)n * Hy + h) * K + k; };

  // 1: the usable frames
  int count = 0;
  for (int t = lane; t < T; t += kWave) {
    bool ok = true;
    for (int ch = 0; ch < nch; ++ch)
      for (int h = 0; h < Hy; ++h) {
        const size_t i = at(n0 + t, h, ch ? jb : ja);
        const float* w = a.world + i * 3;
        ok = ok && fabsf(w[0]) < INFINITY && fabsf(w[1]) < INFINITY && fabsf(w[2]) < INFINITY;
        if (a.unary) ok = ok && fabsf(a.unary[i]) < INFINITY;
      }
    path[t] = ok ? 0 : kTrPassed;
    count += ok ? 1 : 0;
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) count += __shfl_xor(count, m, kWave);
  const bool resolved = count >= 2;
  __syncthreads();

  double C = 0.0;
  if (resolved) {
    // 2: forward.  Lane l < nch Hy 3 carries coordinate l % 3 of hypothesis (l / 3) % Hy of channel l / (3 Hy); lane
    // l < nch Hy the unary of hypothesis l % Hy of channel l / Hy.
    const int xch = lane / (3 * Hy), xh = (lane / 3) % Hy, xc = lane % 3, uch = lane / Hy, uh = lane % Hy;
    const bool has_x = lane < nch * Hy * 3, has_u = lane < nch * Hy;
    float nx = 0.f, nu = 0.f;
    int nuse = kTrPassed, nf = 0;
    const auto fetch = [&](int t) {
      if (has_x) nx = a.world[at(n0 + t, xh, xch ? jb : ja) * 3 + xc];
      if (has_u && a.unary) nu = a.unary[at(n0 + t, uh, uch ? jb : ja)];
      nuse = path[t];
      nf = a.frame[n0 + t];
    };
    fetch(0);
    const TrState me = tr_state(lane < ns ? lane : 0, Hy, pair);
    const int ca = me.e * Hy + me.h0, cb = me.e * Hy + me.h1;         // this state's candidate of either joint
    int cur = 0, prev_f = 0;
    bool first = true;
    for (int t = 0; t < T; ++t) {
      const float x = nx, un = nu;
      const int use = nuse, f = nf;
      if (t + 1 < T) fetch(t + 1);
      if (use == kTrPassed) continue;
      if (has_x) s_pos[cur][xch][xh][xc] = (double)x;
      if (has_u) s_un[cur][uch][uh] = (double)un;
      __syncthreads();
      if (!first) {
        // candidate c of joint `j` (0 = lead): exchange bit c / Hy, hypothesis c % Hy, read from channel j ^ bit
        const double w = a.vel_w / ((double)f - (double)prev_f);
        for (int i = lane; i < nch * nc * nc; i += kWave) {
          const int j = i / (nc * nc), r = i - j * nc * nc, cp = r / nc, cc = r - cp * nc;
          const double* P = s_pos[cur ^ 1][j ^ (cp / Hy)][cp % Hy];
          const double* Q = s_pos[cur][j ^ (cc / Hy)][cc % Hy];
          const double d0 = Q[0] - P[0], d1 = Q[1] - P[1], d2 = Q[2] - P[2];
          s_tab[j][cp * nc + cc] = w * (d0 * d0 + d1 * d1 + d2 * d2);
        }
        __syncthreads();
      }
      if (lane < ns) {
        double local = a.hyp_w * (double)(me.h0 + me.h1) + a.swap_w * (double)me.e + s_un[cur][me.e][me.h0];
        if (pair) local += s_un[cur][me.e ^ 1][me.h1];
        double best = 0.0;
        int arg = 0;
        if (!first) {
          const double* al = s_alpha[cur ^ 1];
          best = INFINITY;
          for (int cp = 0; cp < nc; ++cp) {                           // predecessor i = cp Hy + h1 (pair), cp (single): ascending
            const double da = s_tab[0][cp * nc + ca];
            if (pair) {
              const int eb = (cp / Hy) * Hy;
              for (int h = 0; h < Hy; ++h) {
                const double v = al[cp * Hy + h] + (da + s_tab[1][(eb + h) * nc + cb]);
                if (v < best) { best = v; arg = cp * Hy + h; }
              }
            } else {
              const double v = al[cp] + da;
              if (v < best) { best = v; arg = cp; }
            }
          }
        }
        s_alpha[cur][lane] = best + local;
        back[(size_t)t * ns + lane] = (unsigned char)arg;
      }
      first = false;
      prev_f = f;
      cur ^= 1;
    }
    __syncthreads();

    // 3: the end state, then back along the pointers
    const double* al = s_alpha[cur ^ 1];
    int state = 0;
    C = al[0];
    for (int i = 1; i < ns; ++i)
      if (al[i] < C) { C = al[i]; state = i; }
    for (int t1 = T - 1; t1 >= 0; t1 -= 8) {
      int row[8], use[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int t = t1 - c;
        row[c] = (t >= 0 && lane < ns) ? back[(size_t)t * ns + lane] : 0;
        use[c] = t >= 0 ? path[t] : kTrPassed;
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (use[c] == kTrPassed) continue;
        if (lane == 0) path[t1 - c] = (unsigned char)state;
        state = __shfl(row[c], state, kWave);                         // (the first usable frame's pointer is 0: never followed)
      }
    }
    __syncthreads();
  }

  // 4: outputs
  for (int t = lane; t < T; t += kWave) {
    const int st = resolved ? path[t] : kTrPassed, n = n0 + t;
    const bool passed = st == kTrPassed;
    const TrState q = tr_state(passed ? 0 : st, Hy, pair);
    for (int ch = 0; ch < nch; ++ch) {
      const int k = ch ? jb : ja, h = ch ? q.h1 : q.h0, from = (ch ^ q.e) ? jb : ja;
      const float* src = a.kps + at(n, h, from) * 3;
      const float x0 = src[0], x1 = src[1], x2 = src[2];
      const size_t i = (size_t)n * K + k;
      float* dst = o.sel + i * 3;
      dst[0] = x0; dst[1] = x1; dst[2] = x2;
      if (o.hyp) o.hyp[i] = (unsigned char)h;
      if (o.swap) o.swap[i] = (unsigned char)q.e;
      if (o.status) o.status[i] = passed ? 1 : 0;
    }
  }
  if (lane == 0 && o.cost) {
    o.cost[(size_t)s * K + ja] = C;
    if (pair) o.cost[(size_t)s * K + jb] = C;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static inline bool tr_shape_ok(int N, int Hy, int K) {
  return N > 0 && Hy >= 1 && Hy <= kTrHy && K >= 1 && K <= kTrK && (long)N * K <= 0x7fffffffL;
}
static inline size_t tr_back_bytes(int N, int Hy, int K) { return align16((size_t)N * K * 2 * Hy * Hy); }
static inline bool tr_overlap(const void* p, size_t np, const void* q, size_t nq) {
  return p && q && (const char*)p < (const char*)q + nq && (const char*)q < (const char*)p + np;
}

}  // namespace xas

using namespace xas;

extern "C" size_t xas_track_resolve_workspace_bytes(int N, int Hy, int K) {
  if (!tr_shape_ok(N, Hy, K)) return 0;
  return track_table_bytes(N) + tr_back_bytes(N, Hy, K) + align16((size_t)N * K);
}

extern "C" int xas_track_resolve(const float* kps, const float* world, const float* unary, const int* perm, const int* start,
                                 const int* frame, int N, int Hy, int K, int S, double vel_w, double hyp_w, double swap_w,
                                 float* sel, unsigned char* hyp, unsigned char* swap, unsigned char* status, double* cost,
                                 void* workspace, void* stream) {
  const char* who = "track_resolve";
  XAS_REQUIRE(kps && world && perm && start && frame && sel && workspace,
              "%s: null buffer (kps, world, perm, start, frame, sel and workspace are required)", who);
  XAS_REQUIRE(Hy >= 1 && Hy <= kTrHy, "%s: Hy=%d hypotheses (needs 1 <= Hy <= %d: a pair's 2 Hy^2 states are the lanes of one wave)",
              who, Hy, kTrHy);
  XAS_REQUIRE(tr_shape_ok(N, Hy, K), "%s: bad shape N=%d K=%d (needs N > 0, 1 <= K <= %d, N*K < 2^31)", who, N, K, kTrK);
  if (track_check_start(who, start, N, K, S)) return 1;
  TrArgs a = {};
  for (int k = 0; k < K; ++k) {
    XAS_REQUIRE(perm[k] >= 0 && perm[k] < K && perm[perm[k]] == k,
                "%s: perm[%d] = %d is not an involution of 0 .. %d (needs perm[perm[k]] = k: pairs and fixed joints)", who, k,
                perm[k], K - 1);
    a.perm[k] = (unsigned char)perm[k];
    if (k <= perm[k]) a.lead[a.U++] = (unsigned char)k;
  }
  const double wts[3] = {vel_w, hyp_w, swap_w};
  const char* names[3] = {"vel_w", "hyp_w", "swap_w"};
  for (int i = 0; i < 3; ++i)
    XAS_REQUIRE(wts[i] >= 0.0 && wts[i] < INFINITY, "%s: %s %f (needs a finite %s >= 0)", who, names[i], wts[i], names[i]);
  XAS_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", who);
  const size_t nk = (size_t)N * K, nhk = nk * Hy;
  const struct { const void* p; size_t bytes; const char* name; } outs[5] = {{sel, nk * 12, "sel"}, {hyp, nk, "hyp"},
      {swap, nk, "swap"}, {status, nk, "status"}, {cost, (size_t)S * K * 8, "cost"}},
      ins[4] = {{kps, nhk * 12, "kps"}, {world, nhk * 12, "world"}, {unary, nhk * 4, "unary"}, {frame, (size_t)N * 4, "frame"}};
  for (const auto& out : outs)
    for (const auto& in : ins)
      XAS_REQUIRE(!tr_overlap(out.p, out.bytes, in.p, in.bytes), "%s: %s must not overlap %s (the inputs stay as they are)", who,
                  out.name, in.name);
  int* table = (int*)workspace;
  if (int e = track_copy_start(start, S, table, as_stream(stream))) return e;
  a.kps = kps; a.world = world; a.unary = unary; a.frame = frame; a.start = table;
  a.back = (unsigned char*)workspace + track_table_bytes(N);
  a.path = a.back + tr_back_bytes(N, Hy, K);
  a.N = N; a.Hy = Hy; a.K = K;
  a.vel_w = vel_w; a.hyp_w = hyp_w; a.swap_w = swap_w;
  const TrOut o = {sel, hyp, swap, status, cost};
  hipLaunchKernelGGL(track_resolve_kernel, dim3((unsigned)(S * a.U)), dim3(64), 0, as_stream(stream), a, o);
  XAS_LAUNCH_CHECK();
  return 0;
}
