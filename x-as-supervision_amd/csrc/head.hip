// Fused D x H x W soft-argmax ("integral") head, forward and backward.  gfx950.
//
// Replaces keypoint_detector_integral_multi.py:69-88 / keypoint_detector_integral.py:48-63.
// HBM-bound: the forward reads the logits exactly once (online softmax, all three
// marginals in one pass), the backward reads them once and writes the gradient once.
//
// Data layout: logits are NHWC, i.e. [B][H*W][K*D]: one pixel holds K*D contiguous
// floats.  A thread owns one float4 of channels (joint k, depth bins 4q..4q+3) and walks
// pixels, so every wave-instruction loads 1 KiB of contiguous memory.
//
// Pass 1 (head_partial): per (b, pixel chunk) -> per joint {max, sum e*w, sum e*h, pz[D]}.
// Pass 2 (head_finalize): one wave per (b,k): merge chunks, normalise, pick the depth
// peaks (value desc, index asc), windowed expectation, write kps / indices / stats.
// Pass 2 of the flip test (head_finalize_flip_kernel): the same, on the average of an image's heat-map and the mirrored,
// left/right-swapped heat-map of its mirror image, formed from the two images' records.
// Heat-map spread (head_spread_partial_kernel, head_spread_finalize_kernel): mean and covariance of every joint's x-y marginal,
// a pass of its own on the same geometry and policies, for the evaluation's triangulation weights.
//
// One kernel family, two policies (template parameter POW2 of the partial and backward kernels):
//   * power of two, D in {4,8,16,32,64} where that block exists for K (pow2_policy): pix -> (h, w) is shift/mask; the
//     G = D/4 lanes of one (slot, joint) sit inside one wave (R is a multiple of 64 / gcd(C4, 64)) and reduce with an
//     xor-shuffle tree; one block holds all K joints;
//   * general, every other D % 4 == 0 up to 128: one division per thread before the loop, then the thread walks (h, w) by
//     its pixel stride (rh rows + rw columns, one carry); the G lanes reduce through LDS in lane order (G = 3, 10, 24 ... have
//     no xor tree), wherever the group falls inside a wave; a block holds the channel quads of KT joints (all K when
//     K*G <= 1024, else the joints are tiled over gridDim.z).
// A power-of-two side that the first policy cannot hold runs on the general one; XAS_TUNE_GENERAL_KERNELS puts every
// power-of-two side there (coverage).  pow2_policy is the one rule.
#include "common.h"

namespace xas {

struct HeadGeom {
  int B, K, D, HW, W, C4, G, rec;   // rec = 3 + D floats per (b,chunk,k)
  int KT, ntile, C4t;               // joints per block, joint tiles (gridDim.z), channel quads per block and pixel
  int R, rh, rw, wshift;            // pixel slots per block; R = rh * W + rw: a thread's step in (h, w); log2(W) (POW2 only)
  int P, nchunk;                    // pixels per block, blocks per image
};

// Pixel slots of the power-of-two policy: its lane groups never straddle a wave, so R is a multiple of 64 / gcd(C4, 64).
static int pow2_slots(long C4) {
  int gcd = 1;
  while (gcd < 64 && (C4 % (gcd * 2)) == 0) gcd *= 2;
  return 64 / gcd;
}

// The dispatch rule: which policy a (cube side, joint count) runs on.  A power-of-two side whose power-of-two geometry does
// not exist (fewer pixels than the slots that keep a lane group inside a wave, or a block wider than 1024 threads: K = 3 at
// D = 4, K = 17 at D = 64) runs on the general policy, which tiles the joints.
static bool pow2_policy(int D, int K) {
  if (!(D >= 4 && D <= 64 && (D & (D - 1)) == 0) || (tune_flags() & XAS_TUNE_GENERAL_KERNELS)) return false;
  if (K <= 0) return true;                        // (make_geom reports it)
  const long C4 = (long)K * (D / 4);
  const int R = pow2_slots(C4);
  return R <= D * D && C4 * R <= 1024;
}

static int make_geom(int B, int K, int D, bool pow2, HeadGeom* g) {
  XAS_REQUIRE(B > 0 && K > 0, "head: need B > 0 and K > 0, got B=%d K=%d D=%d", B, K, D);
  XAS_REQUIRE(D >= 4 && D <= 128 && D % 4 == 0,
              "head: depth_dim must be a multiple of 4 in [4,128] (heat-map cube D == H == W), got B=%d K=%d D=%d", B, K, D);
  g->B = B; g->K = K; g->D = D; g->W = D; g->HW = D * D;
  g->G = D / 4;
  g->C4 = K * g->G;
  g->rec = 3 + D;
  const int ktmax = 1024 / g->G;                  // >= 32 joints
  g->ntile = pow2 ? 1 : (K + ktmax - 1) / ktmax;
  g->KT = (K + g->ntile - 1) / g->ntile;
  g->C4t = g->KT * g->G;
  int R = 1;
  if (pow2) R = pow2_slots(g->C4);
  while ((long)g->C4t * R * 2 <= 640 && R * 2 <= g->HW) R *= 2;
  XAS_REQUIRE((long)g->C4t * R <= 1024, "head: K*D=%d too wide for one workgroup", K * D);
  g->R = R; g->rh = R / g->W; g->rw = R % g->W;
  g->wshift = 0;
  while ((1 << g->wshift) < D) ++g->wshift;
  g->P = R > 128 ? R : 128;       // pixels per workgroup: 128 amortises the block-level merge (64: 3.8 TB/s)
  if (g->P > g->HW) g->P = g->HW;
  g->P = (g->P / R) * R;
  XAS_REQUIRE(g->P >= R, "head: heat-map too small");
  g->nchunk = (g->HW + g->P - 1) / g->P;
  return 0;
}

// ---- what the two policies supply ----------------------------------------------------------------------------------------
// (h, w) of the pixels a thread visits, as floats.  POW2: from the pixel index.  General: the thread starts at `pix` and
// every call steps by g.R pixels, so it must be called once per visited pixel, in order.
template <bool POW2>
struct PixelWalk {
  int h, w;
  __device__ PixelWalk(const HeadGeom& g, int pix) {
    if constexpr (!POW2) { h = pix / g.W; w = pix - h * g.W; }   // the only division
  }
  __device__ void next(const HeadGeom& g, int pix, float* fh, float* fw) {
    if constexpr (POW2) {
      *fw = (float)(pix & (g.W - 1)); *fh = (float)(pix >> g.wshift);
    } else {
      *fw = (float)w; *fh = (float)h;
      w += g.rw; h += g.rh;
      if (w >= g.W) { w -= g.W; ++h; }
    }
  }
};

// Maximum over the G lanes of this thread's (slot, joint); `lead` is the group's first thread.  General: through s[blockDim.x].
template <bool POW2>
__device__ float group_max(float v, int G, float* s, int lead) {
  if constexpr (POW2) {
    for (int o = G >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
  } else {
    s[threadIdx.x] = v;
    __syncthreads();
    float gm = -INFINITY;
    for (int j = 0; j < G; ++j) gm = fmaxf(gm, s[lead + j]);
    return gm;
  }
}
// Sums of x and y over the same lanes (valid in the group's first thread): xor tree, or LDS in lane order.
template <bool POW2>
__device__ void group_sum2(float& x, float& y, int G, float* s_x, float* s_y, int lead) {
  if constexpr (POW2) {
    for (int o = G >> 1; o > 0; o >>= 1) { x += __shfl_xor(x, o, 64); y += __shfl_xor(y, o, 64); }
  } else {
    s_x[threadIdx.x] = x;
    s_y[threadIdx.x] = y;
    __syncthreads();
    if ((int)threadIdx.x == lead) {
      x = 0.f; y = 0.f;
      for (int j = 0; j < G; ++j) { x += s_x[lead + j]; y += s_y[lead + j]; }
    }
  }
}

static size_t partial_lds_bytes(const HeadGeom& g, bool pow2) {
  return ((size_t)g.R * g.KT * g.rec + (pow2 ? 0 : 3 * (size_t)g.C4t * g.R)) * sizeof(float);
}

template <bool POW2>
__global__ void head_partial_kernel(const float4* __restrict__ logits, float* __restrict__ partial, HeadGeom g) {
  extern __shared__ float smem[];            // [R][KT][3 + D] records; general: then per thread max, sx, sy
  const int KT = POW2 ? g.K : g.KT, C4t = POW2 ? g.C4 : g.C4t;
  float* s_m = smem + (size_t)g.R * KT * g.rec;
  float* s_x = s_m + blockDim.x;
  float* s_y = s_x + blockDim.x;
  const int tid = threadIdx.x;
  const int c4t = tid % C4t, slot = tid / C4t;
  const int kt = c4t / g.G, dq = c4t % g.G;
  const int k0 = POW2 ? 0 : blockIdx.z * KT, k = k0 + kt;
  const bool live = POW2 || k < g.K;         // the last joint tile may be ragged
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int pix0 = chunk * g.P;
  const int pend = min(g.P, g.HW - pix0);

  float m = -INFINITY, sx = 0.f, sy = 0.f, z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
  if (live) {
    const float4* base = logits + ((size_t)b * g.HW + pix0) * g.C4 + (k * g.G + dq);
    PixelWalk<POW2> walk(g, pix0 + slot);
    // four pixels per trip: one running-max update (one rescale exp) per 16 values keeps the loop-carried
    // dependency short; the 4 loads are issued back to back
    int p = slot;
    for (; p + 3 * g.R < pend; p += 4 * g.R) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = stream_load(base + (size_t)(p + u * g.R) * g.C4);
      float mn = m;
#pragma unroll
      for (int u = 0; u < 4; ++u) mn = fmaxf(mn, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
      const float sc = __expf(m - mn);          // exp(-inf) = 0 on the first trip
      m = mn;
      z0 *= sc; z1 *= sc; z2 *= sc; z3 *= sc; sx *= sc; sy *= sc;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float fh, fw;
        walk.next(g, pix0 + p + u * g.R, &fh, &fw);
        const float e0 = __expf(v[u].x - mn), e1 = __expf(v[u].y - mn), e2 = __expf(v[u].z - mn), e3 = __expf(v[u].w - mn);
        const float es = (e0 + e1) + (e2 + e3);
        z0 += e0; z1 += e1; z2 += e2; z3 += e3;
        sx = fmaf(es, fw, sx);
        sy = fmaf(es, fh, sy);
      }
    }
    for (; p < pend; p += g.R) {
      const float4 v = stream_load(base + (size_t)p * g.C4);
      float fh, fw;
      walk.next(g, pix0 + p, &fh, &fw);
      const float mn = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
      const float sc = __expf(m - mn);
      m = mn;
      const float e0 = __expf(v.x - mn), e1 = __expf(v.y - mn), e2 = __expf(v.z - mn), e3 = __expf(v.w - mn);
      const float es = (e0 + e1) + (e2 + e3);
      z0 = z0 * sc + e0; z1 = z1 * sc + e1; z2 = z2 * sc + e2; z3 = z3 * sc + e3;
      sx = sx * sc + es * fw;
      sy = sy * sc + es * fh;
    }
  }
  // unify the running max over the G lanes of this (slot, joint), then sum sx / sy
  const int lead = tid - dq;                  // first thread of the group
  const float gm = group_max<POW2>(m, g.G, s_m, lead);
  const float sc = (m == -INFINITY) ? 0.f : __expf(m - gm);
  z0 *= sc; z1 *= sc; z2 *= sc; z3 *= sc; sx *= sc; sy *= sc;
  group_sum2<POW2>(sx, sy, g.G, s_x, s_y, lead);
  float* rec = smem + ((size_t)slot * KT + kt) * g.rec;
  if (dq == 0) { rec[0] = gm; rec[1] = sx; rec[2] = sy; }
  rec[3 + 4 * dq + 0] = z0; rec[3 + 4 * dq + 1] = z1; rec[3 + 4 * dq + 2] = z2; rec[3 + 4 * dq + 3] = z3;
  __syncthreads();
  // merge the R slots; thread t handles entry t of this tile's [joints][rec] record table
  const int kn = POW2 ? g.K : min(KT, g.K - k0);
  float* out = partial + (((size_t)b * g.nchunk + chunk) * g.K + k0) * g.rec;
  for (int e = tid; e < kn * g.rec; e += blockDim.x) {
    const int kk = e / g.rec, f = e % g.rec;
    float M = -INFINITY;
    for (int s = 0; s < g.R; ++s) M = fmaxf(M, smem[((size_t)s * KT + kk) * g.rec]);
    if (f == 0) { out[e] = M; continue; }
    float acc = 0.f;
    for (int s = 0; s < g.R; ++s) {
      const float* r = smem + ((size_t)s * KT + kk) * g.rec;
      const float ms = r[0];
      acc += (ms == -INFINITY) ? 0.f : r[f] * __expf(ms - M);
    }
    out[e] = acc;
  }
}

// ---- second pass: one wave per (b,k); lane l keeps depth bins l and l + 64 (the second one is dead for D <= 64: it holds 0
// and scores -1).  Two kernels share its two halves: head_finalize_kernel (one image) and head_finalize_flip_kernel (an image
// and its mirror).
// The chunks of one (image, joint) merged under their own running maximum: this lane's two depth-bin sums and the moments
// along W and H, all still scaled by exp(-M).
struct ChunkSums { float M, sd0, sd1, SX, SY; };

__device__ __forceinline__ ChunkSums merge_chunks(const float* __restrict__ p0, const HeadGeom& g, int d0, int d1, bool live0, bool live1) {
  const size_t cstride = (size_t)g.K * g.rec;
  ChunkSums a;
  a.M = -INFINITY;
  for (int c = 0; c < g.nchunk; ++c) a.M = fmaxf(a.M, p0[c * cstride]);
  a.sd0 = 0.f; a.sd1 = 0.f; a.SX = 0.f; a.SY = 0.f;
  for (int c = 0; c < g.nchunk; ++c) {
    const float* r = p0 + c * cstride;
    const float sc = __expf(r[0] - a.M);
    if (live0) a.sd0 += r[3 + d0] * sc;
    if (live1) a.sd1 += r[3 + d1] * sc;
    a.SX += r[1] * sc;
    a.SY += r[2] * sc;
  }
  return a;
}

// Everything after the marginals: the depth-probability map, then either the plain expectation (neighbor == 0) or the peak
// scores, the lowest-bin tie rule, the num_hypo picks and their windowed expectations, and the int64 peak bins.  pz0 / pz1:
// this lane's bins of the depth marginal (dead bins 0); X, Y: expectations along W and H in pixels.  st: this joint's
// statistics for the backward, or null (a forward-only caller).
__device__ __forceinline__ void finalize_tail(const HeadGeom& g, int b, int k, float pz0, float pz1, float X, float Y, int num_hypo,
                                              int neighbor, float* __restrict__ kps, int64_t* __restrict__ z_idx,
                                              float* __restrict__ depth_prob_map, int dmap_every, float* __restrict__ st) {
  const int lane = threadIdx.x;
  const int d0 = lane, d1 = lane + 64;
  const bool live0 = d0 < g.D, live1 = d1 < g.D;
  if (b % dmap_every == 0) {
    float* dm = depth_prob_map + ((size_t)(b / dmap_every) * g.K + k) * g.D;
    if (live0) dm[d0] = pz0;
    if (live1) dm[d1] = pz1;
  }
  const float fD = (float)g.D;
  const float xn = X / fD * 2.f - 1.f, yn = Y / fD * 2.f - 1.f;

  if (neighbor == 0) {                        // single hypothesis: plain expectation
    const float Z = wave_sum(pz0 * (float)d0 + pz1 * (float)d1);
    if (lane == 0) {
      float* o = kps + ((size_t)b * g.K + k) * 3;
      o[0] = xn; o[1] = yn; o[2] = Z / fD * 2.f - 1.f;
      if (st) st[3] = Z;
      if (z_idx) z_idx[(size_t)b * g.K + k] = 0;
    }
    return;
  }
  // neighbours: bin 63's right one is bin 64 (lane 0's second bin), bin 64's left one is bin 63 (lane 63's first bin)
  float left0 = __shfl_up(pz0, 1, 64), right0 = __shfl_down(pz0, 1, 64);
  float left1 = __shfl_up(pz1, 1, 64), right1 = __shfl_down(pz1, 1, 64);
  const float bin64 = __shfl(pz1, 0, 64), bin63 = __shfl(pz0, 63, 64);
  if (lane == 63) right0 = bin64;
  if (lane == 0) left1 = bin63;
  const bool inner0 = d0 >= 1 && d0 <= g.D - 2, inner1 = d1 <= g.D - 2;   // (bin 127's right neighbour is never read)
  float score0 = inner0 ? ((pz0 >= left0 && pz0 >= right0) ? pz0 : 0.f) : -1.f;
  float score1 = inner1 ? ((pz1 >= left1 && pz1 >= right1) ? pz1 : 0.f) : -1.f;
  const int r = neighbor / 2;
  for (int h = 0; h < num_hypo; ++h) {
    const float best = wave_max(fmaxf(score0, score1));
    const unsigned long long cand0 = __ballot(score0 == best), cand1 = __ballot(score1 == best);
    // lowest bin among equal scores: every first bin (0..63) sorts before every second bin (64..127)
    const int idx = cand0 ? __ffsll((long long)cand0) - 1 : 64 + __ffsll((long long)cand1) - 1;
    if (d0 == idx) score0 = -2.f;
    if (d1 == idx) score1 = -2.f;
    const bool in0 = live0 && (d0 >= idx - r) && (d0 <= idx + r);
    const bool in1 = live1 && (d1 >= idx - r) && (d1 <= idx + r);
    const float sw = wave_sum((in0 ? pz0 : 0.f) + (in1 ? pz1 : 0.f));
    const float swd = wave_sum((in0 ? pz0 * (float)d0 : 0.f) + (in1 ? pz1 * (float)d1 : 0.f));
    const float Z = swd / sw;
    if (lane == 0) {
      float* o = kps + (((size_t)b * num_hypo + h) * g.K + k) * 3;
      o[0] = xn; o[1] = yn; o[2] = Z / fD * 2.f - 1.f;
      z_idx[((size_t)b * g.K + k) * num_hypo + h] = idx;
      if (st) { st[3 + h] = Z; st[9 + h] = sw; }
    }
  }
}

__global__ void head_finalize_kernel(const float* __restrict__ partial, HeadGeom g, int num_hypo, int neighbor,
                                     float* __restrict__ kps, int64_t* __restrict__ z_idx,
                                     float* __restrict__ depth_prob_map, int dmap_every, float* __restrict__ stats) {
  const int b = blockIdx.x / g.K, k = blockIdx.x % g.K;
  const int lane = threadIdx.x;
  const int d0 = lane, d1 = lane + 64;
  const bool live0 = d0 < g.D, live1 = d1 < g.D;
  const ChunkSums a = merge_chunks(partial + ((size_t)b * g.nchunk * g.K + k) * g.rec, g, d0, d1, live0, live1);
  const float S = wave_sum(a.sd0 + a.sd1);    // dead bins hold 0
  const float pz0 = live0 ? a.sd0 / S : 0.f, pz1 = live1 ? a.sd1 / S : 0.f;
  const float X = a.SX / S, Y = a.SY / S;
  float* st = stats + ((size_t)b * g.K + k) * XAS_HEAD_STATS;
  if (lane == 0) { st[0] = a.M + __logf(S); st[1] = X; st[2] = Y; }
  finalize_tail(g, b, k, pz0, pz1, X, Y, num_hypo, neighbor, kps, z_idx, depth_prob_map, dmap_every, st);
}

// Flip test (the test-time step of integral-regression detectors; keypoint_detector_integral_multi.py:36-88 applied to the
// average of a heat-map and the mirrored, pair-swapped heat-map of the mirrored image).  The records hold g.B = 2B images:
// image b and, at B + b, its horizontal mirror.  A mirror acts linearly on a record - depth sums and the H moment stay, the
// W moment becomes (W - 1) * sum e - sum e*w - so the averaged distribution's marginals come from the records of (b, k) and
// (B + b, perm[k]), each normalised by its own softmax sum; no mirrored logits exist.  Forward only: no statistics.
__global__ void head_finalize_flip_kernel(const float* __restrict__ partial, HeadGeom g, const int* __restrict__ perm,
                                          int num_hypo, int neighbor, float* __restrict__ kps, int64_t* __restrict__ z_idx,
                                          float* __restrict__ depth_prob_map, int dmap_every) {
  const int b = blockIdx.x / g.K, k = blockIdx.x % g.K;      // b < B = g.B / 2
  const int lane = threadIdx.x;
  const int d0 = lane, d1 = lane + 64;
  const bool live0 = d0 < g.D, live1 = d1 < g.D;
  int k2 = perm[k];
  if ((unsigned)k2 >= (unsigned)g.K) k2 = k;  // (the binding refuses such a table; no record outside the buffer is read)
  const size_t image = (size_t)g.nchunk * g.K * g.rec;
  const ChunkSums a = merge_chunks(partial + b * image + (size_t)k * g.rec, g, d0, d1, live0, live1);
  const ChunkSums m = merge_chunks(partial + ((size_t)(g.B / 2) + b) * image + (size_t)k2 * g.rec, g, d0, d1, live0, live1);
  const float S1 = wave_sum(a.sd0 + a.sd1), S2 = wave_sum(m.sd0 + m.sd1);
  const float pz0 = live0 ? 0.5f * (a.sd0 / S1 + m.sd0 / S2) : 0.f, pz1 = live1 ? 0.5f * (a.sd1 / S1 + m.sd1 / S2) : 0.f;
  const float X = 0.5f * (a.SX / S1 + ((float)(g.W - 1) - m.SX / S2)), Y = 0.5f * (a.SY / S1 + m.SY / S2);
  finalize_tail(g, b, k, pz0, pz1, X, Y, num_hypo, neighbor, kps, z_idx, depth_prob_map, dmap_every, nullptr);
}

// per (b,k): {cx, cy, c0, lse, gz[D]}; thread = depth bin (64 threads for D <= 64, else 128; nothing crosses lanes here)
__global__ void head_bwd_coef_kernel(const float* __restrict__ stats, const int64_t* __restrict__ z_idx,
                                     const float* __restrict__ grad_kps, HeadGeom g, int num_hypo, int neighbor,
                                     float* __restrict__ coef) {
  const int b = blockIdx.x / g.K, k = blockIdx.x % g.K;
  const int d = threadIdx.x;
  const float* st = stats + ((size_t)b * g.K + k) * XAS_HEAD_STATS;
  const float fD = (float)g.D;
  float gx = 0.f, gy = 0.f, gz = 0.f, c0 = 0.f;
  const int r = neighbor / 2;
  for (int h = 0; h < num_hypo; ++h) {
    const float* gk = grad_kps + (((size_t)b * num_hypo + h) * g.K + k) * 3;
    gx += gk[0];
    gy += gk[1];
    if (neighbor == 0) {
      const float cz = gk[2] * (2.f / fD);
      gz += cz * (float)d;
      c0 -= cz * st[3];
    } else {
      const int idx = (int)z_idx[((size_t)b * g.K + k) * num_hypo + h];
      if (d >= idx - r && d <= idx + r) gz += gk[2] * (2.f / fD) * ((float)d - st[3 + h]) / st[9 + h];
    }
  }
  const float cx = gx * (2.f / fD), cy = gy * (2.f / fD);
  c0 += -cx * st[1] - cy * st[2];
  float* o = coef + ((size_t)b * g.K + k) * (4 + g.D);
  if (d == 0) { o[0] = cx; o[1] = cy; o[2] = c0; o[3] = st[0]; }
  if (d < g.D) o[4 + d] = gz;
}

template <bool POW2>
__global__ void head_bwd_kernel(const float4* __restrict__ logits, const float* __restrict__ coef, HeadGeom g,
                                float4* __restrict__ grad, float* __restrict__ amax_out) {
  __shared__ unsigned s_amax;                          // amax_out != null: max |grad| of the block (bit pattern), then of the launch
  if (threadIdx.x == 0) s_amax = 0u;
  if (amax_out) __syncthreads();
  float amx = 0.f;
  const int KT = POW2 ? g.K : g.KT, C4t = POW2 ? g.C4 : g.C4t;
  const int tid = threadIdx.x;
  const int c4t = tid % C4t, slot = tid / C4t;
  const int kt = c4t / g.G, dq = c4t % g.G;
  const int bz = POW2 ? 0 : blockIdx.z;
  const int k = bz * KT + kt;
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int pix0 = chunk * g.P;
  const int pend = min(g.P, g.HW - pix0);
  if (POW2 || k < g.K) {
    const float* cf = coef + ((size_t)b * g.K + k) * (4 + g.D);
    const float cx = cf[0], cy = cf[1], c0 = cf[2], lse = cf[3];
    const float4 gz = *reinterpret_cast<const float4*>(cf + 4 + 4 * dq);
    const size_t off = ((size_t)b * g.HW + pix0) * g.C4 + (k * g.G + dq);
    PixelWalk<POW2> walk(g, pix0 + slot);
#pragma unroll 4
    for (int p = slot; p < pend; p += g.R) {
      const float4 v = stream_load(logits + off + (size_t)p * g.C4);
      float fh, fw;
      walk.next(g, pix0 + p, &fh, &fw);
      const float lin = cx * fw + cy * fh + c0;
      float4 o;
      o.x = __expf(v.x - lse) * (lin + gz.x);
      o.y = __expf(v.y - lse) * (lin + gz.y);
      o.z = __expf(v.z - lse) * (lin + gz.z);
      o.w = __expf(v.w - lse) * (lin + gz.w);
      amx = amax4(amx, o);
      stream_store(grad + off + (size_t)p * g.C4, o);
    }
  }
  if (amax_out) {                                      // (the block is not a whole number of waves: reduce through LDS)
    if (amx > 0.f) atomicMax(&s_amax, __float_as_uint(amx));
    __syncthreads();
    // one atomic per block, to the sub-maximum the block index selects (common.h: recorded maxima)
    const unsigned sub = (blockIdx.x + (blockIdx.y + bz * gridDim.y) * gridDim.x) % (unsigned)kAmaxSub;
    if (threadIdx.x == 0 && s_amax) atomicMax(reinterpret_cast<unsigned*>(amax_out + sub * kAmaxStride), s_amax);
  }
}

// ---- heat-map spread: mean and covariance of every joint's x-y marginal, in cells (xas_head_spread) ------------------------
// No counterpart in the reference: the spatial spread of the soft-max heat-map as a per-view confidence.  Self-contained (its
// own online soft-max, the logits read once) on the geometry, thread mapping and two policies of head_partial_kernel.
//
// A record is a weighted sample in mean / centred-second-moment form, its weights scaled by exp(-m):
//   {m, S = sum e, uw, uh = weighted means of w, h, Mw, Mh = sum e (w - uw)^2, sum e (h - uh)^2, C = sum e (w - uw)(h - uh)}.
// Records merge pairwise (Chan et al.): with Sa, Sb the two weights on the common scale exp(-max(ma, mb)), f = Sb / (Sa + Sb)
// and d = ub - ua,
//   u = ua + d f,   M = Ma + Mb + d^2 Sa f,   C = Ca + Cb + dw dh Sa f.
// Every added term of a second moment is a square times a weight, so nothing cancels: E[w^2] - E[w]^2 loses four digits for a
// one-cell peak at w = 127 and can go negative.  A pixel enters as the one-point record {es, w, h, 0, 0, 0}.  The merge order
// is fixed at every level (pixels of a thread, lanes of a group, slots of a block, chunks of an image): no atomics.
// A NaN logit never becomes a maximum (fmaxf) but makes its exponential, hence S and every moment of that joint, NaN.
struct SpreadRec { float m, S, uw, uh, Mw, Mh, C; };
constexpr int kSpreadRec = 7;

__device__ __forceinline__ SpreadRec spread_merge(const SpreadRec& a, const SpreadRec& b) {
  SpreadRec r;
  r.m = fmaxf(a.m, b.m);
  const float sa = (a.m == -INFINITY) ? 0.f : __expf(a.m - r.m), sb = (b.m == -INFINITY) ? 0.f : __expf(b.m - r.m);
  const float Sa = a.S * sa, Sb = b.S * sb;
  r.S = Sa + Sb;
  const float f = (r.S == 0.f) ? 0.f : Sb / r.S;     // (NaN == 0 is false: a NaN weight goes through)
  const float x = Sa * f, dw = b.uw - a.uw, dh = b.uh - a.uh;
  r.uw = a.uw + dw * f;
  r.uh = a.uh + dh * f;
  r.Mw = a.Mw * sa + b.Mw * sb + dw * dw * x;
  r.Mh = a.Mh * sa + b.Mh * sb + dh * dh * x;
  r.C = a.C * sa + b.C * sb + dw * dh * x;
  return r;
}

// One pixel of weight es (already on the record's scale) at cell (fw, fh): spread_merge with a one-point record.
__device__ __forceinline__ void spread_add(SpreadRec& r, float es, float fw, float fh) {
  const float Sn = r.S + es;
  const float f = (Sn == 0.f) ? 0.f : __fdividef(es, Sn);
  const float x = r.S * f, dw = fw - r.uw, dh = fh - r.uh;
  r.S = Sn;
  r.uw += dw * f;
  r.uh += dh * f;
  r.Mw += dw * dw * x;
  r.Mh += dh * dh * x;
  r.C += dw * dh * x;
}

__device__ __forceinline__ void spread_rescale(SpreadRec& r, float mn) {
  const float sc = __expf(r.m - mn);                 // exp(-inf) = 0 before the first pixel
  r.m = mn;
  r.S *= sc; r.Mw *= sc; r.Mh *= sc; r.C *= sc;
}

__device__ __forceinline__ SpreadRec spread_read(const float* p) { return {p[0], p[1], p[2], p[3], p[4], p[5], p[6]}; }
__device__ __forceinline__ void spread_write(float* p, const SpreadRec& r) {
  p[0] = r.m; p[1] = r.S; p[2] = r.uw; p[3] = r.uh; p[4] = r.Mw; p[5] = r.Mh; p[6] = r.C;
}

// The record of the G lanes of this thread's (slot, joint), merged in lane order (valid in the group's first thread, `lead`):
// xor tree whose lower lane is always the left operand, or through s[blockDim.x][7] one lane after the other.
template <bool POW2>
__device__ SpreadRec group_merge(SpreadRec r, int G, int dq, float* s, int lead) {
  if constexpr (POW2) {
    for (int o = 1; o < G; o <<= 1) {
      SpreadRec t;
      t.m = __shfl_xor(r.m, o, 64); t.S = __shfl_xor(r.S, o, 64); t.uw = __shfl_xor(r.uw, o, 64); t.uh = __shfl_xor(r.uh, o, 64);
      t.Mw = __shfl_xor(r.Mw, o, 64); t.Mh = __shfl_xor(r.Mh, o, 64); t.C = __shfl_xor(r.C, o, 64);
      r = (dq & o) ? spread_merge(t, r) : spread_merge(r, t);
    }
    return r;
  } else {
    spread_write(s + (size_t)threadIdx.x * kSpreadRec, r);
    __syncthreads();
    if ((int)threadIdx.x == lead)
      for (int j = 1; j < G; ++j) r = spread_merge(r, spread_read(s + (size_t)(lead + j) * kSpreadRec));
    return r;
  }
}

static size_t spread_lds_bytes(const HeadGeom& g, bool pow2) {
  return ((size_t)g.R * g.KT + (pow2 ? 0 : (size_t)g.C4t * g.R)) * kSpreadRec * sizeof(float);
}

// First pass: per (b, pixel chunk, joint) one record, [B][nchunk][K][7].
template <bool POW2>
__global__ void head_spread_partial_kernel(const float4* __restrict__ logits, float* __restrict__ partial, HeadGeom g) {
  extern __shared__ float smem[];            // [R][KT][7] slot records; general: then [blockDim][7] lane records
  const int KT = POW2 ? g.K : g.KT, C4t = POW2 ? g.C4 : g.C4t;
  float* s_lane = smem + (size_t)g.R * KT * kSpreadRec;
  const int tid = threadIdx.x;
  const int c4t = tid % C4t, slot = tid / C4t;
  const int kt = c4t / g.G, dq = c4t % g.G;
  const int k0 = POW2 ? 0 : blockIdx.z * KT, k = k0 + kt;
  const bool live = POW2 || k < g.K;         // the last joint tile may be ragged
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int pix0 = chunk * g.P;
  const int pend = min(g.P, g.HW - pix0);

  SpreadRec r = {-INFINITY, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float4* base = logits + ((size_t)b * g.HW + pix0) * g.C4 + (k * g.G + dq);
    PixelWalk<POW2> walk(g, pix0 + slot);
    int p = slot;
    for (; p + 3 * g.R < pend; p += 4 * g.R) {       // four loads in flight, one rescale per 16 values (as head_partial_kernel)
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = stream_load(base + (size_t)(p + u * g.R) * g.C4);
      float mn = r.m;
#pragma unroll
      for (int u = 0; u < 4; ++u) mn = fmaxf(mn, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
      spread_rescale(r, mn);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float fh, fw;
        walk.next(g, pix0 + p + u * g.R, &fh, &fw);
        const float es = (__expf(v[u].x - mn) + __expf(v[u].y - mn)) + (__expf(v[u].z - mn) + __expf(v[u].w - mn));
        spread_add(r, es, fw, fh);
      }
    }
    for (; p < pend; p += g.R) {
      const float4 v = stream_load(base + (size_t)p * g.C4);
      float fh, fw;
      walk.next(g, pix0 + p, &fh, &fw);
      const float mn = fmaxf(fmaxf(r.m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
      spread_rescale(r, mn);
      const float es = (__expf(v.x - mn) + __expf(v.y - mn)) + (__expf(v.z - mn) + __expf(v.w - mn));
      spread_add(r, es, fw, fh);
    }
  }
  r = group_merge<POW2>(r, g.G, dq, s_lane, tid - dq);
  if (dq == 0) spread_write(smem + ((size_t)slot * KT + kt) * kSpreadRec, r);
  __syncthreads();
  // merge the R slots in slot order; thread t handles joint t of this tile
  const int kn = POW2 ? g.K : min(KT, g.K - k0);
  if (tid < kn) {
    SpreadRec a = spread_read(smem + (size_t)tid * kSpreadRec);
    for (int s = 1; s < g.R; ++s) a = spread_merge(a, spread_read(smem + ((size_t)s * KT + tid) * kSpreadRec));
    spread_write(partial + (((size_t)b * g.nchunk + chunk) * g.K + k0 + tid) * kSpreadRec, a);
  }
}

// Second pass: one wave per (b, k).  Lane c holds chunk c's record (64 at a time); every lane merges them in ascending chunk
// order, reading lane after lane, so the wave agrees bit for bit; lane 0 normalises and writes {E w, E h, Var w, Var h, Cov}.
__global__ void head_spread_finalize_kernel(const float* __restrict__ partial, HeadGeom g, float* __restrict__ spread) {
  const int b = blockIdx.x / g.K, k = blockIdx.x % g.K;
  const int lane = threadIdx.x;
  const float* p0 = partial + ((size_t)b * g.nchunk * g.K + k) * kSpreadRec;
  const size_t cstride = (size_t)g.K * kSpreadRec;
  SpreadRec a = {-INFINITY, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < g.nchunk; c0 += 64) {
    const int n = min(64, g.nchunk - c0);
    SpreadRec mine = a;                              // (lanes past n: never read)
    if (lane < n) mine = spread_read(p0 + (size_t)(c0 + lane) * cstride);
    for (int j = 0; j < n; ++j) {
      SpreadRec t;
      t.m = __shfl(mine.m, j, 64); t.S = __shfl(mine.S, j, 64); t.uw = __shfl(mine.uw, j, 64); t.uh = __shfl(mine.uh, j, 64);
      t.Mw = __shfl(mine.Mw, j, 64); t.Mh = __shfl(mine.Mh, j, 64); t.C = __shfl(mine.C, j, 64);
      a = spread_merge(a, t);
    }
  }
  if (lane == 0) {
    const float vw = a.Mw / a.S, vh = a.Mh / a.S;
    float* o = spread + ((size_t)b * g.K + k) * XAS_HEAD_SPREAD;
    o[0] = a.uw; o[1] = a.uh;
    o[2] = vw < 0.f ? 0.f : vw;                      // (a comparison, not fmaxf: NaN stays NaN)
    o[3] = vh < 0.f ? 0.f : vh;
    o[4] = a.C / a.S;
  }
}

// ---- argument checks: each one is written once --------------------------------------------------------------------------
static int check_modes(const char* who, int D, int num_hypo, int neighbor, const int64_t* z_idx, int B, int groups) {
  XAS_REQUIRE(num_hypo >= 1 && num_hypo <= 6, "%s: num_hypo %d not in [1,6]", who, num_hypo);
  XAS_REQUIRE(neighbor >= 0 && (neighbor > 0 || num_hypo == 1), "%s: single-hypothesis mode needs num_hypo == 1", who);
  XAS_REQUIRE(neighbor == 0 || (z_idx != nullptr && num_hypo <= D - 2), "%s: z_idx required / too many hypotheses", who);
  XAS_REQUIRE(groups >= 1 && B % groups == 0, "%s: B=%d does not split into %d groups", who, B, groups);
  return 0;
}

static int check_grid(const char* who, const HeadGeom& g) {
  XAS_REQUIRE(g.B <= 65535 && g.ntile <= 65535, "%s: B=%d K=%d exceed the launch grid", who, g.B, g.K);
  return 0;
}

static int launch_finalize(const float* partial, const HeadGeom& g, int num_hypo, int neighbor, float* kps, int64_t* z_idx,
                           float* depth_prob_map, int groups, float* stats, void* stream) {
  hipLaunchKernelGGL(head_finalize_kernel, dim3(g.B * g.K), dim3(64), 0, as_stream(stream), partial, g, num_hypo,
                     neighbor, kps, z_idx, depth_prob_map, g.B / groups, stats);
  XAS_LAUNCH_CHECK();
  return 0;
}

// Records of 2B images -> outputs of B (head_finalize_flip_kernel).  g is the geometry of the 2B-image first pass.
static int launch_finalize_flip(const float* partial, const HeadGeom& g, const int* perm, int num_hypo, int neighbor, float* kps,
                                int64_t* z_idx, float* depth_prob_map, int groups, void* stream) {
  const int B = g.B / 2;
  hipLaunchKernelGGL(head_finalize_flip_kernel, dim3(B * g.K), dim3(64), 0, as_stream(stream), partial, g, perm, num_hypo,
                     neighbor, kps, z_idx, depth_prob_map, B / groups);
  XAS_LAUNCH_CHECK();
  return 0;
}

static int launch_partial(const float* logits, float* partial, const HeadGeom& g, bool pow2, const char* who, void* stream) {
  XAS_REQUIRE(((uintptr_t)logits & 15) == 0, "%s: logits must be 16-byte aligned", who);
  const size_t lds = partial_lds_bytes(g, pow2);
  XAS_REQUIRE(lds <= 64 * 1024, "%s: LDS %zu too large", who, lds);
  if (check_grid(who, g)) return 1;
  hipLaunchKernelGGL(pow2 ? head_partial_kernel<true> : head_partial_kernel<false>, dim3(g.nchunk, g.B, g.ntile),
                     dim3(g.C4t * g.R), lds, as_stream(stream), reinterpret_cast<const float4*>(logits), partial, g);
  XAS_LAUNCH_CHECK();
  return 0;
}

}  // namespace xas

using namespace xas;

extern "C" size_t xas_head_workspace_floats(int B, int K, int D) {
  HeadGeom g;
  if (make_geom(B, K, D, pow2_policy(D, K), &g)) return 0;
  return (size_t)B * g.nchunk * K * g.rec;
}

extern "C" int xas_head_softargmax_fwd(const float* logits, int B, int K, int D, int num_hypo, int neighbor,
                                       float* kps, int64_t* z_idx, float* depth_prob_map, int groups, float* stats,
                                       float* partial, void* stream) {
  const bool pow2 = pow2_policy(D, K);
  HeadGeom g;
  if (make_geom(B, K, D, pow2, &g)) return 1;
  XAS_REQUIRE(logits && kps && depth_prob_map && stats && partial, "head fwd: null buffer");
  if (check_modes("head fwd", D, num_hypo, neighbor, z_idx, B, groups)) return 1;
  if (launch_partial(logits, partial, g, pow2, "head fwd", stream)) return 1;
  return launch_finalize(partial, g, num_hypo, neighbor, kps, z_idx, depth_prob_map, groups, stats, stream);
}

// The second pass alone, over partial records that something else produced: xas_conv_fwd_head (conv.hip) emits them from the
// final convolution's epilogue, `nchunk` records of 64 pixels per image in the layout of head_partial_kernel
// ([image][chunk][joint][3 + D]).  Everything downstream (kps, int64 peak indices, depth maps, statistics for the backward)
// is what xas_head_softargmax_fwd writes.
extern "C" int xas_head_softargmax_from_partials(const float* partial, int B, int K, int D, int nchunk, int num_hypo, int neighbor,
                                                 float* kps, int64_t* z_idx, float* depth_prob_map, int groups, float* stats,
                                                 void* stream) {
  HeadGeom g;
  if (make_geom(B, K, D, pow2_policy(D, K), &g)) return 1;
  XAS_REQUIRE(partial && kps && depth_prob_map && stats && nchunk >= 1, "head from partials: null buffer");
  if (check_modes("head from partials", D, num_hypo, neighbor, z_idx, B, groups)) return 1;
  g.nchunk = nchunk;
  return launch_finalize(partial, g, num_hypo, neighbor, kps, z_idx, depth_prob_map, groups, stats, stream);
}

// Flip test, second pass alone: `partial` holds the records of 2B images (image B + b is the horizontal mirror of image b),
// `perm` (device int32 [K]) the joint each joint takes from the mirrored image (its left/right partner, itself when unpaired).
// Outputs are those of xas_head_softargmax_from_partials for B images of the averaged heat-map, minus the statistics.
extern "C" int xas_head_softargmax_flip_from_partials(const float* partial, int B, int K, int D, int nchunk, int num_hypo,
                                                      int neighbor, const int* perm, float* kps, int64_t* z_idx,
                                                      float* depth_prob_map, int groups, void* stream) {
  XAS_REQUIRE(B > 0 && B <= (1 << 29), "head flip from partials: need 0 < B, got B=%d (the records hold 2B images)", B);
  HeadGeom g;
  if (make_geom(2 * B, K, D, pow2_policy(D, K), &g)) return 1;
  XAS_REQUIRE(partial && perm && kps && depth_prob_map && nchunk >= 1, "head flip from partials: null buffer");
  if (check_modes("head flip from partials", D, num_hypo, neighbor, z_idx, B, groups)) return 1;
  g.nchunk = nchunk;
  return launch_finalize_flip(partial, g, perm, num_hypo, neighbor, kps, z_idx, depth_prob_map, groups, stream);
}

// Flip test from the logits of 2B images: the first pass of xas_head_softargmax_fwd over all of them, then the flip merge.
// partial: xas_head_workspace_floats(2B, K, D) floats.
extern "C" int xas_head_softargmax_fwd_flip(const float* logits, int B, int K, int D, int num_hypo, int neighbor, const int* perm,
                                            float* kps, int64_t* z_idx, float* depth_prob_map, int groups, float* partial,
                                            void* stream) {
  XAS_REQUIRE(B > 0 && B <= (1 << 29), "head fwd flip: need 0 < B, got B=%d (the logits hold 2B images)", B);
  const bool pow2 = pow2_policy(D, K);
  HeadGeom g;
  if (make_geom(2 * B, K, D, pow2, &g)) return 1;
  XAS_REQUIRE(logits && perm && kps && depth_prob_map && partial, "head fwd flip: null buffer");
  if (check_modes("head fwd flip", D, num_hypo, neighbor, z_idx, B, groups)) return 1;
  if (launch_partial(logits, partial, g, pow2, "head fwd flip", stream)) return 1;
  return launch_finalize_flip(partial, g, perm, num_hypo, neighbor, kps, z_idx, depth_prob_map, groups, stream);
}

extern "C" size_t xas_head_spread_workspace_floats(int B, int K, int D) {
  HeadGeom g;
  if (make_geom(B, K, D, pow2_policy(D, K), &g)) return 0;
  return (size_t)B * g.nchunk * K * kSpreadRec;
}

// Mean and covariance of every joint's x-y soft-max marginal, in heat-map cells: spread [B][K][5] = {E w, E h, Var w, Var h,
// Cov(w, h)}.  Two launches on the caller's stream; workspace: xas_head_spread_workspace_floats(B, K, D) floats.
extern "C" int xas_head_spread(const float* logits, int B, int K, int D, float* spread, float* workspace, void* stream) {
  const bool pow2 = pow2_policy(D, K);
  HeadGeom g;
  if (make_geom(B, K, D, pow2, &g)) return 1;
  XAS_REQUIRE(logits && spread && workspace, "head spread: null buffer");
  XAS_REQUIRE(((uintptr_t)logits & 15) == 0, "head spread: logits must be 16-byte aligned");
  const size_t lds = spread_lds_bytes(g, pow2);
  XAS_REQUIRE(lds <= 64 * 1024, "head spread: LDS %zu too large", lds);
  XAS_REQUIRE((long)B * K < (1L << 31), "head spread: B=%d K=%d exceed the launch grid", B, K);
  if (check_grid("head spread", g)) return 1;
  hipLaunchKernelGGL(pow2 ? head_spread_partial_kernel<true> : head_spread_partial_kernel<false>, dim3(g.nchunk, g.B, g.ntile),
                     dim3(g.C4t * g.R), lds, as_stream(stream), reinterpret_cast<const float4*>(logits), workspace, g);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_spread_finalize_kernel, dim3(B * K), dim3(64), 0, as_stream(stream), workspace, g, spread);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_head_softargmax_bwd(const float* logits, const float* stats, const int64_t* z_idx,
                                       const float* grad_kps, int B, int K, int D, int num_hypo, int neighbor,
                                       float* grad_logits, float* coef, void* stream) {
  return xas_head_softargmax_bwd_amax(logits, stats, z_idx, grad_kps, B, K, D, num_hypo, neighbor, grad_logits, coef, nullptr, stream);
}

extern "C" int xas_head_softargmax_bwd_amax(const float* logits, const float* stats, const int64_t* z_idx,
                                            const float* grad_kps, int B, int K, int D, int num_hypo, int neighbor,
                                            float* grad_logits, float* coef, float* amax_out, void* stream) {
  const bool pow2 = pow2_policy(D, K);
  HeadGeom g;
  if (make_geom(B, K, D, pow2, &g)) return 1;
  XAS_REQUIRE(logits && stats && grad_kps && grad_logits && coef, "head bwd: null buffer");
  XAS_REQUIRE(num_hypo >= 1 && num_hypo <= 6, "head bwd: num_hypo %d not in [1,6]", num_hypo);
  XAS_REQUIRE(neighbor == 0 || z_idx != nullptr, "head bwd: z_idx required");
  XAS_REQUIRE((((uintptr_t)logits | (uintptr_t)grad_logits | (uintptr_t)coef) & 15) == 0, "head bwd: 16-byte alignment");
  if (check_grid("head bwd", g)) return 1;
  hipLaunchKernelGGL(head_bwd_coef_kernel, dim3(B * K), dim3(D <= 64 ? 64 : 128), 0, as_stream(stream), stats, z_idx,
                     grad_kps, g, num_hypo, neighbor, coef);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pow2 ? head_bwd_kernel<true> : head_bwd_kernel<false>, dim3(g.nchunk, B, g.ntile), dim3(g.C4t * g.R), 0,
                     as_stream(stream), reinterpret_cast<const float4*>(logits), coef, g, reinterpret_cast<float4*>(grad_logits),
                     amax_out);
  XAS_LAUNCH_CHECK();
  return 0;
}
