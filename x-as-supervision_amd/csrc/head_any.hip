// General D x H x W soft-argmax head: every cube side D with D % 4 == 0, 4 <= D <= 128.  gfx950.
//
// Same work, data layout and record layout as head.hip (read that header first); this family drops the three things that
// tie head.hip to power-of-two sides of at most 64:
//   * pix -> (h, w): one division per thread before the loop, then the thread walks (h, w) by its pixel stride
//     (rh rows + rw columns, one carry), so the hot loop has no division and no shift/mask;
//   * the reduction over the G = D/4 lanes of one (slot, joint) goes through LDS in a fixed order (G = 3, 10, 24 ... have no
//     xor tree), which also makes it independent of where a group falls inside a wave;
//   * a block holds the channel quads of KT joints (all K when K*G <= 1024, else the joints are tiled over gridDim.z), and
//     the finalize kernel keeps two depth bins per lane (d and d + 64) of one wave.
// A block of C4t = KT*G quads x R pixel slots reads R consecutive pixels per trip: with one joint tile that is one
// contiguous run of memory per trip, every wave instruction loading 1 KiB of it.
#include "common.h"
#include "head_any.h"

namespace xas {

struct AnyGeom {
  int B, K, D, HW, W, C4, G, rec;   // rec = 3 + D floats per (b,chunk,k)
  int KT, ntile, C4t;               // joints per block, joint tiles (gridDim.z), channel quads per block and pixel
  int R, rh, rw;                    // pixel slots per block; R = rh * W + rw: a thread's step in (h, w)
  int P, nchunk;                    // pixels per block, blocks per image
};

static int make_any_geom(int B, int K, int D, AnyGeom* g) {
  XAS_REQUIRE(B > 0 && K > 0, "head: need B > 0 and K > 0, got B=%d K=%d D=%d", B, K, D);
  XAS_REQUIRE(D >= 4 && D <= 128 && D % 4 == 0,
              "head: depth_dim must be a multiple of 4 in [4,128] (heat-map cube D == H == W), got B=%d K=%d D=%d", B, K, D);
  g->B = B; g->K = K; g->D = D; g->W = D; g->HW = D * D;
  g->G = D / 4;
  g->C4 = K * g->G;
  g->rec = 3 + D;
  const int ktmax = 1024 / g->G;                  // >= 32 joints
  g->ntile = (K + ktmax - 1) / ktmax;
  g->KT = (K + g->ntile - 1) / g->ntile;
  g->C4t = g->KT * g->G;                          // <= 1024
  int R = 1;
  while ((long)g->C4t * R * 2 <= 640 && R * 2 <= g->HW) R *= 2;
  g->R = R; g->rh = R / g->W; g->rw = R % g->W;
  g->P = R > 128 ? R : 128;                       // as head.hip: 128 pixels amortise the block-level merge
  if (g->P > g->HW) g->P = g->HW;
  g->P = (g->P / R) * R;                          // R <= HW, so P >= R
  g->nchunk = (g->HW + g->P - 1) / g->P;
  return 0;
}

static size_t partial_lds_bytes(const AnyGeom& g) {
  return ((size_t)g.R * g.KT * g.rec + 3 * (size_t)g.C4t * g.R) * sizeof(float);
}

__global__ void head_any_partial_kernel(const float4* __restrict__ logits, float* __restrict__ partial, AnyGeom g) {
  extern __shared__ float smem[];            // [R][KT][3 + D] records, then per thread: max, sx, sy
  float* s_m = smem + (size_t)g.R * g.KT * g.rec;
  float* s_x = s_m + blockDim.x;
  float* s_y = s_x + blockDim.x;
  const int tid = threadIdx.x;
  const int c4t = tid % g.C4t, slot = tid / g.C4t;
  const int kt = c4t / g.G, dq = c4t % g.G;
  const int k0 = blockIdx.z * g.KT, k = k0 + kt;
  const bool live = k < g.K;                 // the last joint tile may be ragged
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int pix0 = chunk * g.P;
  const int pend = min(g.P, g.HW - pix0);

  float m = -INFINITY, sx = 0.f, sy = 0.f, z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
  if (live) {
    const float4* base = logits + ((size_t)b * g.HW + pix0) * g.C4 + (k * g.G + dq);
    int h = (pix0 + slot) / g.W, w = (pix0 + slot) - h * g.W;     // the only division; then walk by (rh, rw)
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
        const float fw = (float)w, fh = (float)h;
        const float e0 = __expf(v[u].x - mn), e1 = __expf(v[u].y - mn), e2 = __expf(v[u].z - mn), e3 = __expf(v[u].w - mn);
        const float es = (e0 + e1) + (e2 + e3);
        z0 += e0; z1 += e1; z2 += e2; z3 += e3;
        sx = fmaf(es, fw, sx);
        sy = fmaf(es, fh, sy);
        w += g.rw; h += g.rh;
        if (w >= g.W) { w -= g.W; ++h; }
      }
    }
    for (; p < pend; p += g.R) {
      const float4 v = stream_load(base + (size_t)p * g.C4);
      const float fw = (float)w, fh = (float)h;
      const float mn = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
      const float sc = __expf(m - mn);
      m = mn;
      const float e0 = __expf(v.x - mn), e1 = __expf(v.y - mn), e2 = __expf(v.z - mn), e3 = __expf(v.w - mn);
      const float es = (e0 + e1) + (e2 + e3);
      z0 = z0 * sc + e0; z1 = z1 * sc + e1; z2 = z2 * sc + e2; z3 = z3 * sc + e3;
      sx = sx * sc + es * fw;
      sy = sy * sc + es * fh;
      w += g.rw; h += g.rh;
      if (w >= g.W) { w -= g.W; ++h; }
    }
  }
  // unify the running max over the G threads of this (slot, joint) through LDS, then sum sx / sy in lane order
  s_m[tid] = m;
  __syncthreads();
  const int lead = tid - dq;                  // first thread of the group
  float gm = -INFINITY;
  for (int j = 0; j < g.G; ++j) gm = fmaxf(gm, s_m[lead + j]);
  const float sc = (m == -INFINITY) ? 0.f : __expf(m - gm);
  float* rec = smem + ((size_t)slot * g.KT + kt) * g.rec;
  rec[3 + 4 * dq + 0] = z0 * sc; rec[3 + 4 * dq + 1] = z1 * sc; rec[3 + 4 * dq + 2] = z2 * sc; rec[3 + 4 * dq + 3] = z3 * sc;
  s_x[tid] = sx * sc;
  s_y[tid] = sy * sc;
  __syncthreads();
  if (dq == 0) {
    float ax = 0.f, ay = 0.f;
    for (int j = 0; j < g.G; ++j) { ax += s_x[lead + j]; ay += s_y[lead + j]; }
    rec[0] = gm; rec[1] = ax; rec[2] = ay;
  }
  __syncthreads();
  // merge the R slots; thread t handles entry t of this tile's [joints][rec] record table
  const int kn = min(g.KT, g.K - k0);
  float* out = partial + (((size_t)b * g.nchunk + chunk) * g.K + k0) * g.rec;
  for (int e = tid; e < kn * g.rec; e += blockDim.x) {
    const int kk = e / g.rec, f = e % g.rec;
    float M = -INFINITY;
    for (int s = 0; s < g.R; ++s) M = fmaxf(M, smem[((size_t)s * g.KT + kk) * g.rec]);
    if (f == 0) { out[e] = M; continue; }
    float acc = 0.f;
    for (int s = 0; s < g.R; ++s) {
      const float* r = smem + ((size_t)s * g.KT + kk) * g.rec;
      const float ms = r[0];
      acc += (ms == -INFINITY) ? 0.f : r[f] * __expf(ms - M);
    }
    out[e] = acc;
  }
}

// One wave per (b,k); lane l keeps depth bins l and l + 64.
__global__ void head_any_finalize_kernel(const float* __restrict__ partial, AnyGeom g, int num_hypo, int neighbor,
                                         float* __restrict__ kps, int64_t* __restrict__ z_idx,
                                         float* __restrict__ depth_prob_map, int dmap_every, float* __restrict__ stats) {
  const int b = blockIdx.x / g.K, k = blockIdx.x % g.K;
  const int lane = threadIdx.x;
  const int d0 = lane, d1 = lane + 64;
  const bool live0 = d0 < g.D, live1 = d1 < g.D;
  const float* p0 = partial + ((size_t)b * g.nchunk * g.K + k) * g.rec;
  const size_t cstride = (size_t)g.K * g.rec;
  float M = -INFINITY;
  for (int c = 0; c < g.nchunk; ++c) M = fmaxf(M, p0[c * cstride]);
  float sd0 = 0.f, sd1 = 0.f, SX = 0.f, SY = 0.f;
  for (int c = 0; c < g.nchunk; ++c) {
    const float* r = p0 + c * cstride;
    const float sc = __expf(r[0] - M);
    if (live0) sd0 += r[3 + d0] * sc;
    if (live1) sd1 += r[3 + d1] * sc;
    SX += r[1] * sc;
    SY += r[2] * sc;
  }
  const float S = wave_sum(sd0 + sd1);        // dead bins hold 0
  const float pz0 = live0 ? sd0 / S : 0.f, pz1 = live1 ? sd1 / S : 0.f;
  const float X = SX / S, Y = SY / S;
  float* st = stats + ((size_t)b * g.K + k) * XAS_HEAD_STATS;
  if (b % dmap_every == 0) {
    float* dm = depth_prob_map + ((size_t)(b / dmap_every) * g.K + k) * g.D;
    if (live0) dm[d0] = pz0;
    if (live1) dm[d1] = pz1;
  }
  const float fD = (float)g.D;
  const float xn = X / fD * 2.f - 1.f, yn = Y / fD * 2.f - 1.f;
  if (lane == 0) { st[0] = M + __logf(S); st[1] = X; st[2] = Y; }

  if (neighbor == 0) {                        // single hypothesis: plain expectation
    const float Z = wave_sum(pz0 * (float)d0 + pz1 * (float)d1);
    if (lane == 0) {
      float* o = kps + ((size_t)b * g.K + k) * 3;
      o[0] = xn; o[1] = yn; o[2] = Z / fD * 2.f - 1.f;
      st[3] = Z;
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
      st[3 + h] = Z;
      st[9 + h] = sw;
    }
  }
}

// per (b,k): {cx, cy, c0, lse, gz[D]}; 128 threads, thread = depth bin (nothing crosses lanes here)
__global__ void head_any_bwd_coef_kernel(const float* __restrict__ stats, const int64_t* __restrict__ z_idx,
                                         const float* __restrict__ grad_kps, AnyGeom g, int num_hypo, int neighbor,
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

__global__ void head_any_bwd_kernel(const float4* __restrict__ logits, const float* __restrict__ coef, AnyGeom g,
                                    float4* __restrict__ grad, float* __restrict__ amax_out) {
  __shared__ unsigned s_amax;                          // amax_out != null: max |grad| of the block (bit pattern), then of the launch
  if (threadIdx.x == 0) s_amax = 0u;
  if (amax_out) __syncthreads();
  float amx = 0.f;
  const int tid = threadIdx.x;
  const int c4t = tid % g.C4t, slot = tid / g.C4t;
  const int kt = c4t / g.G, dq = c4t % g.G;
  const int k = blockIdx.z * g.KT + kt;
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int pix0 = chunk * g.P;
  const int pend = min(g.P, g.HW - pix0);
  if (k < g.K) {
    const float* cf = coef + ((size_t)b * g.K + k) * (4 + g.D);
    const float cx = cf[0], cy = cf[1], c0 = cf[2], lse = cf[3];
    const float4 gz = *reinterpret_cast<const float4*>(cf + 4 + 4 * dq);
    const size_t off = ((size_t)b * g.HW + pix0) * g.C4 + (k * g.G + dq);
    int h = (pix0 + slot) / g.W, w = (pix0 + slot) - h * g.W;
#pragma unroll 4
    for (int p = slot; p < pend; p += g.R) {
      const float4 v = stream_load(logits + off + (size_t)p * g.C4);
      const float lin = cx * (float)w + cy * (float)h + c0;
      float4 o;
      o.x = __expf(v.x - lse) * (lin + gz.x);
      o.y = __expf(v.y - lse) * (lin + gz.y);
      o.z = __expf(v.z - lse) * (lin + gz.z);
      o.w = __expf(v.w - lse) * (lin + gz.w);
      amx = amax4(amx, o);
      stream_store(grad + off + (size_t)p * g.C4, o);
      w += g.rw; h += g.rh;
      if (w >= g.W) { w -= g.W; ++h; }
    }
  }
  if (amax_out) {                                      // (the block is not a whole number of waves: reduce through LDS)
    if (amx > 0.f) atomicMax(&s_amax, __float_as_uint(amx));
    __syncthreads();
    // one atomic per block, to the sub-maximum the block index selects (common.h: recorded maxima)
    const unsigned sub = (blockIdx.x + (blockIdx.y + blockIdx.z * gridDim.y) * gridDim.x) % (unsigned)kAmaxSub;
    if (threadIdx.x == 0 && s_amax) atomicMax(reinterpret_cast<unsigned*>(amax_out + sub * kAmaxStride), s_amax);
  }
}

size_t head_any_workspace_floats(int B, int K, int D) {
  AnyGeom g;
  if (make_any_geom(B, K, D, &g)) return 0;
  return (size_t)B * g.nchunk * K * g.rec;
}

static int check_modes(const char* who, int D, int num_hypo, int neighbor, const int64_t* z_idx, int B, int groups) {
  XAS_REQUIRE(num_hypo >= 1 && num_hypo <= 6, "%s: num_hypo %d not in [1,6]", who, num_hypo);
  XAS_REQUIRE(neighbor >= 0 && (neighbor > 0 || num_hypo == 1), "%s: single-hypothesis mode needs num_hypo == 1", who);
  XAS_REQUIRE(neighbor == 0 || (z_idx != nullptr && num_hypo <= D - 2), "%s: z_idx required / too many hypotheses", who);
  XAS_REQUIRE(groups >= 1 && B % groups == 0, "%s: B=%d does not split into %d groups", who, B, groups);
  return 0;
}

static int launch_finalize(const float* partial, const AnyGeom& g, int num_hypo, int neighbor, float* kps, int64_t* z_idx,
                           float* depth_prob_map, int groups, float* stats, void* stream) {
  hipLaunchKernelGGL(head_any_finalize_kernel, dim3(g.B * g.K), dim3(64), 0, as_stream(stream), partial, g, num_hypo,
                     neighbor, kps, z_idx, depth_prob_map, g.B / groups, stats);
  XAS_LAUNCH_CHECK();
  return 0;
}

int head_any_fwd(const float* logits, int B, int K, int D, int num_hypo, int neighbor, float* kps, int64_t* z_idx,
                 float* depth_prob_map, int groups, float* stats, float* partial, void* stream) {
  AnyGeom g;
  if (make_any_geom(B, K, D, &g)) return 1;
  XAS_REQUIRE(logits && kps && depth_prob_map && stats && partial, "head fwd: null buffer");
  if (check_modes("head fwd", D, num_hypo, neighbor, z_idx, B, groups)) return 1;
  XAS_REQUIRE(((uintptr_t)logits & 15) == 0, "head fwd: logits must be 16-byte aligned");
  const size_t lds = partial_lds_bytes(g);
  XAS_REQUIRE(lds <= 64 * 1024, "head fwd: LDS %zu too large", lds);
  XAS_REQUIRE(B <= 65535 && g.ntile <= 65535, "head fwd: B=%d K=%d exceed the launch grid", B, K);
  hipLaunchKernelGGL(head_any_partial_kernel, dim3(g.nchunk, B, g.ntile), dim3(g.C4t * g.R), lds, as_stream(stream),
                     reinterpret_cast<const float4*>(logits), partial, g);
  XAS_LAUNCH_CHECK();
  return launch_finalize(partial, g, num_hypo, neighbor, kps, z_idx, depth_prob_map, groups, stats, stream);
}

int head_any_from_partials(const float* partial, int B, int K, int D, int nchunk, int num_hypo, int neighbor, float* kps,
                           int64_t* z_idx, float* depth_prob_map, int groups, float* stats, void* stream) {
  AnyGeom g;
  if (make_any_geom(B, K, D, &g)) return 1;
  XAS_REQUIRE(partial && kps && depth_prob_map && stats && nchunk >= 1, "head from partials: null buffer");
  if (check_modes("head from partials", D, num_hypo, neighbor, z_idx, B, groups)) return 1;
  g.nchunk = nchunk;
  return launch_finalize(partial, g, num_hypo, neighbor, kps, z_idx, depth_prob_map, groups, stats, stream);
}

int head_any_bwd(const float* logits, const float* stats, const int64_t* z_idx, const float* grad_kps, int B, int K, int D,
                 int num_hypo, int neighbor, float* grad_logits, float* coef, float* amax_out, void* stream) {
  AnyGeom g;
  if (make_any_geom(B, K, D, &g)) return 1;
  XAS_REQUIRE(logits && stats && grad_kps && grad_logits && coef, "head bwd: null buffer");
  XAS_REQUIRE(num_hypo >= 1 && num_hypo <= 6, "head bwd: num_hypo %d not in [1,6]", num_hypo);
  XAS_REQUIRE(neighbor == 0 || z_idx != nullptr, "head bwd: z_idx required");
  XAS_REQUIRE((((uintptr_t)logits | (uintptr_t)grad_logits | (uintptr_t)coef) & 15) == 0, "head bwd: 16-byte alignment");
  XAS_REQUIRE(B <= 65535 && g.ntile <= 65535, "head bwd: B=%d K=%d exceed the launch grid", B, K);
  hipLaunchKernelGGL(head_any_bwd_coef_kernel, dim3(B * K), dim3(128), 0, as_stream(stream), stats, z_idx, grad_kps, g,
                     num_hypo, neighbor, coef);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_any_bwd_kernel, dim3(g.nchunk, B, g.ntile), dim3(g.C4t * g.R), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(logits), coef, g, reinterpret_cast<float4*>(grad_logits), amax_out);
  XAS_LAUNCH_CHECK();
  return 0;
}

}  // namespace xas
