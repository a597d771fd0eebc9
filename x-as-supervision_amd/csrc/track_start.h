// What the entry points over tracks share (track_smooth.hip, track_resolve.hip): the rules for `start`, the HOST array that
// cuts the N sorted samples into S tracks, and its copy to the head of the caller's workspace, where the kernels read it.
#pragma once
#include "common.h"

namespace xas {

constexpr int kTrackChunk = 512;
struct TrackStart {
  int v[kTrackChunk];
};

static __global__ __launch_bounds__(256) void track_start_kernel(TrackStart c, int first, int count, int* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) dst[first + i] = c.v[i];
}

static inline size_t track_table_bytes(long N) { return align16((size_t)(N + 1) * sizeof(int)); }

// 1 <= S <= N, S*K < 2^31, start[0] = 0 < ... < start[S] = N.
static inline int track_check_start(const char* who, const int* start, int N, int K, int S) {
  XAS_REQUIRE(S >= 1 && S <= N && (long)S * K <= 0x7fffffffL, "%s: S=%d tracks (needs 1 <= S <= N = %d, S*K < 2^31)", who, S, N);
  XAS_REQUIRE(start[0] == 0 && start[S] == N, "%s: start runs from %d to %d (needs start[0] = 0 and start[S] = N = %d)", who,
              start[0], start[S], N);
  for (int t = 0; t < S; ++t)
    XAS_REQUIRE(start[t] < start[t + 1], "%s: start[%d] = %d >= start[%d] = %d (needs an increasing start: every track has a sample)",
                who, t, start[t], t + 1, start[t + 1]);
  return 0;
}

// start [S+1] -> table, one small launch per kTrackChunk entries, passed by value: nothing of the host array is read later.
static inline int track_copy_start(const int* start, int S, int* table, hipStream_t s) {
  for (int first = 0; first <= S; first += kTrackChunk) {
    TrackStart c;
    const int count = S + 1 - first < kTrackChunk ? S + 1 - first : kTrackChunk;
    for (int i = 0; i < kTrackChunk; ++i) c.v[i] = i < count ? start[first + i] : 0;
    hipLaunchKernelGGL(track_start_kernel, dim3((unsigned)cdiv(count, 256)), dim3(256), 0, s, c, first, count, table);
    XAS_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace xas
