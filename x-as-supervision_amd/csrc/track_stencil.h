// The acceleration prior's stencil on non-uniform frame numbers, in its one copy: the track smoothers (track_band.h) and the
// smoothed SMPL track fit (smplfit_smooth.hip) weigh second differences with it.
#pragma once

namespace xas {

// The acceleration stencil centred at frame s (1 <= s <= T - 2): q_s = cm X_s-1 + c0 X_s + cp X_s+1 is the difference of the
// two slopes, ws = 2 / (h0 + h1) its weight in the prior.
struct TsStencil {
  double cm, c0, cp, ws;
  __device__ __forceinline__ double at(int s, int j) const { return j == s - 1 ? cm : (j == s ? c0 : cp); }
};
__device__ __forceinline__ TsStencil ts_stencil(const int* __restrict__ fr, int s) {
  const double h0 = (double)fr[s] - (double)fr[s - 1], h1 = (double)fr[s + 1] - (double)fr[s];
  TsStencil c;
  c.cm = 1.0 / h0; c.cp = 1.0 / h1; c.c0 = -(c.cm + c.cp); c.ws = 2.0 / (h0 + h1);
  return c;
}

}  // namespace xas
