// HBM-bound NHWC training-mode batch norm: the column reduction (stats / backward sums), the sync merge, the two
// element-wise passes (apply / backward apply), the running statistics, and abs_max.  gfx950.
// (The parameter-free layers are in layers.hip, the layout changes in layout.hip.)
//
// Replaces ATen batch_norm_stats / batch_norm_elemt / batch_norm_backward_{reduce,elemt}
// (nn.BatchNorm2d + nn.SyncBatchNorm: resnet.py:18,40, deconv_head.py:30,
// physique_network.py:18,25,33).
// All kernels move float4 (4 channels) per lane: a wave touches 1 KiB of contiguous rows.
#include "common.h"

namespace xas {


// ---------------------------------------------------------------- column reductions
// x is [M][C] = `G` independent groups of Mg = M / G consecutive rows (the camera-batched step sends the images of
// all cameras through the detector as ONE tensor; every camera keeps its own batch statistics, exactly as the
// reference's per-camera calls, model.py:64,147).  A block owns CB = min(C,256) channels (TX = CB/4 lanes along C)
// and a slab of rows of ONE group; it emits per channel sum(f1), sum(f2) of two per-element functions.
// The finalize pass is folded into the same launch: the block that arrives LAST at a ticket counter (one counter
// per channel block) sums the slab partials of all groups in a fixed order (deterministic) and writes the results
// (rocprof, round 1: 1 262 separate finalize launches per step were pure latency, 13 ms).
struct ColGeom { int TX, TY, CB, ncb, nslab, G; long rows_per_slab, Mg; };

static int col_geom(long M, int C, int G, ColGeom* g) {
  XAS_REQUIRE(M > 0 && C >= 4 && C % 4 == 0, "column reduce: channel count %d must be a positive multiple of 4", C);
  XAS_REQUIRE(G >= 1 && G <= 64 && M % G == 0, "column reduce: %ld rows do not split into %d equal groups", M, G);
  // largest power of two <= 64 dividing C: a 64-channel block still moves 256-byte row segments, and the block that
  // finalizes a channel block reads G * nslab * 512 B of partials (one CU pulls ~100 GB/s: keep that in the tens of KB)
  int cb = 4;
  while (cb < 64 && C % (cb * 2) == 0) cb *= 2;
  g->CB = cb; g->G = G; g->Mg = M / G;
  g->TX = g->CB / 4; g->TY = 256 / g->TX; g->ncb = C / g->CB;
  static const long kWant[4] = {256, 512, 128, 64};           // XAS_TUNE_SLAB_* (experiment)
  long want = kWant[(tune_flags() >> XAS_TUNE_SLAB_SHIFT) & XAS_TUNE_SLAB_MASK] * (G > 1 ? 2 : 1) / ((long)g->ncb * G);   // ~1-2 blocks per CU in total
  long maxslab = cdiv(g->Mg, (long)g->TY * 8);   // at least 8 rows per thread
  if (want > maxslab) want = maxslab;
  if (want < 1) want = 1;
  g->rows_per_slab = cdiv(g->Mg, want);
  g->nslab = (int)cdiv(g->Mg, g->rows_per_slab);
  return 0;
}

// Ticket counters of the folded finalize: a zero-initialised pool per device; a launch takes `ncb` consecutive words,
// the last arriver of each word resets it, so a word is zero again whenever a later launch re-uses it (launches that
// share a word are thousands of launches apart).
constexpr int kTicketWords = 65536;
static unsigned* g_tickets[16] = {};
static unsigned g_ticket_next[16] = {};

static unsigned* take_tickets(int n) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  if (!g_tickets[dev]) {
    unsigned* p = nullptr;
    if (hipMalloc(&p, kTicketWords * sizeof(unsigned)) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, kTicketWords * sizeof(unsigned)) != hipSuccess) return nullptr;
    g_tickets[dev] = p;
  }
  if (g_ticket_next[dev] + (unsigned)n > (unsigned)kTicketWords) g_ticket_next[dev] = 0;
  unsigned* r = g_tickets[dev] + g_ticket_next[dev];
  g_ticket_next[dev] += (unsigned)n;
  return r;
}

// Parameter-gradient accumulation into the .grad arena: hardware float atomics (global_atomic_add_f32), because two
// backward chains of one step (xas_amd/streams.py: chains) may finish the same layer's reduction concurrently on two
// streams.  A parameter receives at most one contribution per chain starting from the zeroed arena, and a + b == b + a
// bit for bit: the result does not depend on which chain arrives first.
__device__ __forceinline__ void grad_add4(float* p, float4 v) {
  unsafeAtomicAdd(p + 0, v.x); unsafeAtomicAdd(p + 1, v.y); unsafeAtomicAdd(p + 2, v.z); unsafeAtomicAdd(p + 3, v.w);
}

// The norm kernels sit on the critical chain of the step and share the CUs with the weight-gradient kernels of the side
// stream: like the chain's convolutions (conv_x6.hip XAS_X6_PRIO) they win the issue arbitration.  r02 / early r03: no
// effect (the chain was MFMA-bound); with the f16x3 convolutions the norms are half of the chain: -1.0 ms per step
// (in-box A/B against no priority, 117.5 vs 118.5).
#ifndef XAS_BN_PRIO
#define XAS_BN_PRIO 3
#endif

// What a launch sums per channel and what its finalize writes.  The values are the <N> of col_reduce_kernel<N> in the
// profiles, the tests and the documents.  A mode with two sums accumulates sum(f1) and sum(f1 * w) of col_term's (f1, w);
// dz = dy after the activation's slope, xhat = the normalised input.
enum ColMode : int {
  kColStats = 0,          // x: f1 = w = x - pivot (pivot = first row of the group) -> mean, biased var (, running statistics)
  kColBwdXY = 1,          // x, dy, and y or the mask bytes under an activation: f1 = dz, w = xhat = (x - mean) * rstd -> sums
  kColSum = 2,            // x: f1 = x, one sum -> column sums (the second sums are zeros)
  kColBwdY = 3,           // dy, y, WITHOUT x (act != 0): f1 = dz, w = xhat = (z - beta) / gamma with z recovered from y -> sums
  kColBwdX = 4,           // x, dy, WITHOUT y: f1 = dz with the sign re-derived from x (bn_affine), w = xhat from x -> sums
  kColStatsPartials = 5,  // x = per-tile partial sums of a convolution epilogue, [rows][C/2 channels][sum(v-p), sum((v-p)^2)]
                          // (C = 2 x channels, pivot per channel or null): f1 = x, one sum -> mean, var (, running statistics)
  kColBwdPartials = 6,    // x = per-tile partial sums of a data-gradient epilogue, [rows][2][C/2 channels] (sum dz | sum dz xhat):
                          // f1 = x, one sum -> out1 = sums [G][2][channels]; acc1 / acc2 (dbeta / dgamma) get the two halves
  kColBwdDual = 7,        // x, x2, dy, mask bytes: block output relu(bn3(x) + bn_d(x2)), two norms under ONE dz: f1 = dz, w = xhat of x,
                          // w2 = xhat of x2 -> sum dz | sum dz w (first norm) and sum dz | sum dz w2 (second norm, ColSecond)
};
constexpr bool col_is_bwd(ColMode m) { return m == kColBwdXY || m == kColBwdY || m == kColBwdX || m == kColBwdDual; }
constexpr bool col_two_sums(ColMode m) { return m == kColStats || col_is_bwd(m); }
constexpr bool col_is_stats(ColMode m) { return m == kColStats || m == kColStatsPartials; }

struct ColArgs {
  const float* x; const float* y; const float* dy;       // [M][C]
  const float* mean; const float* var;                   // [G][C]
  const float* gamma; const float* beta;                 // [C]
  const float* pivot;                                    // kColStatsPartials: [C/2] or null (no pivot)
  const uint8_t* mask;                                   // kColBwdXY: != null -> activation sign bits (one byte per float4, bit e = z_e > 0) instead of y
  float eps; int act; long M; int C; ColGeom g;
  float* partial;              // [G][nslab][2][C]
  unsigned* ticket;            // [ncb]
  // finalize
  float* out1; float* out2;    // group g writes out1[g * out_stride + c], out2[g * out_stride + c]
  long out_stride;
  float* count_out;            // != null: count_out[g * out_stride] = rows per group (SyncBatchNorm message)
  float* running_mean; float* running_var; float momentum, unbias;
  float* acc1; float* acc2;    // != null: acc1[c] += sum over groups of out1 ... (parameter gradients, in place)
  long rows_real;              // kColStatsPartials: activation rows per group behind the partial rows
  // kColBwdDual: the second norm's input and statistics, and where ITS publish / finalize go (same geometry, own tickets)
  struct ColSecond {
    const float* x; const float* mean; const float* var; float eps;
    float* partial; unsigned* ticket; float* out1; float* out2; float* acc1; float* acc2;
  } second;
};

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// write-through (sc1) store / L1-bypassing load of a float4 at a per-lane byte offset of ONE wave-uniform buffer: the
// slab partials cross workgroups inside one launch
__device__ __forceinline__ void store_wt(__amdgpu_buffer_rsrc_t r, unsigned byte_off, float4 v) {
  const u32x4_t u = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
  __builtin_amdgcn_raw_buffer_store_b128(u, r, (int)byte_off, 0, 16);          // aux 16 = sc1
}
__device__ __forceinline__ float4 load_wt(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
  const u32x4_t u = __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 16);
  return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
}

// loads of the reduction passes: PLAIN since r05.  r03/r04 shipped non-temporal loads here like for every streamed operand
// (measured with the weight gradients sharing the chip); on ONE stream the apply kernel that follows reads
// the same x and dy again and finds part of them in the caches when the reduction did not mark them for early eviction:
// -0.7 ms/step (in-box, interleaved, 3 rounds: 124.8 -> 124.1).
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ---- what the backward sums (col_term) and the backward apply (bn_bwd_elem) share, four lanes each --------------------
// dz = dy times the activation's slope: 1 where the pre-activation value z was > 0, else neg (ReLU 0, leaky ReLU 0.01); the
// sign of z comes from y (same sign), from x (re-derived with bn_affine: the forward's decision bit for bit) or from a mask
// byte (bit e = lane e > 0)
__device__ __forceinline__ float act_neg_slope(int act) { return act == 1 ? 0.f : 0.01f; }
__device__ __forceinline__ float4 dz_sign_y(float4 dz, float4 yv, float neg) {
  dz.x *= yv.x > 0.f ? 1.f : neg; dz.y *= yv.y > 0.f ? 1.f : neg; dz.z *= yv.z > 0.f ? 1.f : neg; dz.w *= yv.w > 0.f ? 1.f : neg;
  return dz;
}
__device__ __forceinline__ float4 dz_sign_x(float4 dz, float4 xv, const float4& m, const float4& rs, const float4& bt, float neg) {
  dz.x *= bn_affine(xv.x, m.x, rs.x, bt.x) > 0.f ? 1.f : neg; dz.y *= bn_affine(xv.y, m.y, rs.y, bt.y) > 0.f ? 1.f : neg;
  dz.z *= bn_affine(xv.z, m.z, rs.z, bt.z) > 0.f ? 1.f : neg; dz.w *= bn_affine(xv.w, m.w, rs.w, bt.w) > 0.f ? 1.f : neg;
  return dz;
}
__device__ __forceinline__ float4 dz_sign_mask(float4 dz, unsigned mb, float neg) {
  dz.x *= (mb & 1u) ? 1.f : neg; dz.y *= (mb & 2u) ? 1.f : neg; dz.z *= (mb & 4u) ? 1.f : neg; dz.w *= (mb & 8u) ? 1.f : neg;
  return dz;
}
// xhat = (v - m) * s: from x with (mean, rstd); the sums without x: from the recovered z with (beta, 1 / gamma)
__device__ __forceinline__ float4 xhat4(float4 v, const float4& m, const float4& s) {
  return make_float4((v.x - m.x) * s.x, (v.y - m.y) * s.y, (v.z - m.z) * s.z, (v.w - m.w) * s.w);
}
// the pre-activation value recovered from y: y where y > 0, else y / slope (leaky ReLU; ReLU clipped it: 0)
__device__ __forceinline__ float4 act_inv4(float4 yv, int act) {
  const float up = act == 1 ? 0.f : 100.f;
  return make_float4(yv.x > 0.f ? yv.x : yv.x * up, yv.y > 0.f ? yv.y : yv.y * up, yv.z > 0.f ? yv.z : yv.z * up,
                     yv.w > 0.f ? yv.w : yv.w * up);
}

// the per-channel quantities of a thread's channel quadruple; a mode fills what its term reads
struct ColChan {
  float4 pivot, mean, rstd, rsg, beta, inv_gamma;      // rsg = rstd * gamma (rounded once: bn_affine's contract)
  float4 mean2, rstd2;                                 // kColBwdDual: of the second norm
};

template <ColMode MODE>
__device__ __forceinline__ ColChan col_chan(const ColArgs& a, int grp, int c) {
  ColChan ch{};
  if constexpr (MODE == kColStats) ch.pivot = ld4(a.x + (size_t)grp * a.g.Mg * a.C + c);      // first row of the group
  if constexpr (MODE == kColBwdXY || MODE == kColBwdX || MODE == kColBwdDual) {                 // per-group statistics
    ch.mean = ld4(a.mean + (size_t)grp * a.C + c);
    const float4 v = ld4(a.var + (size_t)grp * a.C + c);
    ch.rstd = make_float4(rsqrtf(v.x + a.eps), rsqrtf(v.y + a.eps), rsqrtf(v.z + a.eps), rsqrtf(v.w + a.eps));
  }
  if constexpr (MODE == kColBwdX) {
    const float4 gm = ld4(a.gamma + c);
    ch.rsg = make_float4(__fmul_rn(ch.rstd.x, gm.x), __fmul_rn(ch.rstd.y, gm.y), __fmul_rn(ch.rstd.z, gm.z), __fmul_rn(ch.rstd.w, gm.w));
    ch.beta = ld4(a.beta + c);
  }
  if constexpr (MODE == kColBwdDual) {
    ch.mean2 = ld4(a.second.mean + (size_t)grp * a.C + c);
    const float4 v = ld4(a.second.var + (size_t)grp * a.C + c);
    const float e2 = a.second.eps;
    ch.rstd2 = make_float4(rsqrtf(v.x + e2), rsqrtf(v.y + e2), rsqrtf(v.z + e2), rsqrtf(v.w + e2));
  }
  if constexpr (MODE == kColBwdY) {
    ch.beta = ld4(a.beta + c);
    const float4 gm = ld4(a.gamma + c);
    ch.inv_gamma = make_float4(gm.x != 0.f ? 1.f / gm.x : 0.f, gm.y != 0.f ? 1.f / gm.y : 0.f, gm.z != 0.f ? 1.f / gm.z : 0.f,
                               gm.w != 0.f ? 1.f / gm.w : 0.f);
  }
  return ch;
}

// (f1, w) of the element at float offset i (four lanes) from the operands the mode reads: the first sum takes f1, the
// second f1 * w (kColBwdDual: and the second norm's second sum f1 * w2; its first sum IS the first norm's)
struct ColTerm { float4 f1, w, w2; };

template <ColMode MODE>
__device__ __forceinline__ ColTerm col_term(const ColArgs& a, const ColChan& ch, long i) {
  const float neg = act_neg_slope(a.act);
  if constexpr (MODE == kColBwdY) {
    const float4 dz = ld4(a.dy + i), yv = ld4(a.y + i);
    return {dz_sign_y(dz, yv, neg), xhat4(act_inv4(yv, a.act), ch.beta, ch.inv_gamma)};
  } else {
    const float4 xv = ld4(a.x + i);
    if constexpr (MODE == kColStats) {
      const float4 d = make_float4(xv.x - ch.pivot.x, xv.y - ch.pivot.y, xv.z - ch.pivot.z, xv.w - ch.pivot.w);
      return {d, d};
    } else if constexpr (MODE == kColBwdXY || MODE == kColBwdDual) {
      float4 dz = ld4(a.dy + i);
      if (a.act && a.mask) dz = dz_sign_mask(dz, a.mask[i >> 2], neg);
      else if (a.act) dz = dz_sign_y(dz, ld4(a.y + i), neg);
      if constexpr (MODE == kColBwdDual) return {dz, xhat4(xv, ch.mean, ch.rstd), xhat4(ld4(a.second.x + i), ch.mean2, ch.rstd2)};
      else return {dz, xhat4(xv, ch.mean, ch.rstd)};
    } else if constexpr (MODE == kColBwdX) {
      return {dz_sign_x(ld4(a.dy + i), xv, ch.mean, ch.rsg, ch.beta, neg), xhat4(xv, ch.mean, ch.rstd)};
    } else {
      return {xv, xv};                                        // plain column sums (w is not read)
    }
  }
}

// ---- the tail every mode shares --------------------------------------------------------------------------------------
// Sum (s1, s2) over the row lanes of the block through `red`, publish the slab's partial sums (write-through), take a
// ticket -> true in the block that arrives LAST at its channel block's counter; its L1 then holds no stale partials.
__device__ __forceinline__ bool col_publish(const ColArgs& a, float4 (&red)[2][256], __amdgpu_buffer_rsrc_t prs, float4 s1,
                                            float4 s2, int tx, int ty, int c, int grp) {
  const ColGeom& g = a.g;
  red[0][threadIdx.x] = s1; red[1][threadIdx.x] = s2;
  __syncthreads();
  for (int s = g.TY >> 1; s > 0; s >>= 1) {
    if (ty < s) {
      const float4 u0 = red[0][threadIdx.x + s * g.TX], v0 = red[1][threadIdx.x + s * g.TX];
      float4& u = red[0][threadIdx.x]; float4& v = red[1][threadIdx.x];
      u.x += u0.x; u.y += u0.y; u.z += u0.z; u.w += u0.w;
      v.x += v0.x; v.y += v0.y; v.z += v0.z; v.w += v0.w;
    }
    __syncthreads();
  }
  if (ty == 0) {
    const unsigned o = (unsigned)(((((size_t)grp * g.nslab + blockIdx.x) * 2) * a.C + c) * sizeof(float));
    store_wt(prs, o, red[0][tx]);
    store_wt(prs, o + (unsigned)a.C * 4u, red[1][tx]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave drains its stores ...
  __syncthreads();                                          // ... before one lane signals for the workgroup
  __shared__ int s_last;
  if (threadIdx.x == 0) {
    const unsigned total = (unsigned)(g.nslab * g.G);
    const unsigned old = __hip_atomic_fetch_add(a.ticket + blockIdx.y, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == total - 1u;
    if (last) {
      __hip_atomic_store(a.ticket + blockIdx.y, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for re-use
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");    // drop this CU's stale L1 lines (other blocks' partials)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_last = last;
  }
  __syncthreads();
  return s_last != 0;
}

// (d1, d2) = the two sums of group gi over its slabs, in double: a row lane adds every TY-th slab in slab order, then the
// lanes are added in lane order through the 8 KB of `dred` (first sums, then second sums); complete where ty == 0
template <int FL>
__device__ __forceinline__ void col_slab_sums(const ColArgs& a, double* dred, __amdgpu_buffer_rsrc_t prs, int gi, int tx, int ty,
                                              int c, double (&d1)[4], double (&d2)[4]) {
  const ColGeom& g = a.g;
  const int nl = g.TY;                                      // slab lanes (same thread layout as the reduction)
#pragma unroll
  for (int e = 0; e < 4; ++e) d1[e] = d2[e] = 0.0;
  const unsigned base = (unsigned)((((size_t)gi * g.nslab * 2) * a.C + c) * sizeof(float));
  const unsigned slab_b = 2u * (unsigned)a.C * 4u, half_b = (unsigned)a.C * 4u;
  auto add = [&](const float4& u, const float4& v) {
    d1[0] += (double)u.x; d1[1] += (double)u.y; d1[2] += (double)u.z; d1[3] += (double)u.w;
    d2[0] += (double)v.x; d2[1] += (double)v.y; d2[2] += (double)v.z; d2[3] += (double)v.w;
  };
  int s = ty;
  for (; s + (FL - 1) * nl < g.nslab; s += FL * nl) {      // 2 * FL independent 16-byte loads in flight per lane
    float4 u[FL], v[FL];
#pragma unroll
    for (int k = 0; k < FL; ++k) {
      u[k] = load_wt(prs, base + (unsigned)(s + k * nl) * slab_b);
      v[k] = load_wt(prs, base + (unsigned)(s + k * nl) * slab_b + half_b);
    }
#pragma unroll
    for (int k = 0; k < FL; ++k) add(u[k], v[k]);
  }
  for (; s < g.nslab; s += nl) add(load_wt(prs, base + (unsigned)s * slab_b), load_wt(prs, base + (unsigned)s * slab_b + half_b));
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) dred[(size_t)threadIdx.x * 4 + e] = half ? d2[e] : d1[e];
    __syncthreads();
    if (ty == 0) {
      for (int k = 1; k < nl; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double t = dred[(size_t)(k * g.TX + tx) * 4 + e];
          if (half) d2[e] += t; else d1[e] += t;
        }
    }
  }
}

// L = 4 or 2 consecutive floats as one 16- or 8-byte access (a thread's statistics: four channels, kColStatsPartials two)
template <int L> __device__ __forceinline__ void ld_lanes(const float* p, float (&v)[4]) {
  if constexpr (L == 4) { const float4 t = ld4(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  else { const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1] = t.y; }
}
template <int L> __device__ __forceinline__ void st_lanes(float* p, const float (&v)[4]) {
  if constexpr (L == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
}

// One channel's statistics from m = S1 / n and q = S2 / n of the values around `pivot` (double), then one step of the running
// statistics.  The caller forms m and q: kColStats divides by n, kColStatsPartials multiplies by 1 / n, and their outputs
// keep those bits.
__device__ __forceinline__ void col_stat_lane(double m, double q, float pivot, float& mean, float& var) {
  double v = q - m * m;
  if (v < 0.0) v = 0.0;
  mean = (float)((double)pivot + m); var = (float)v;
}
__device__ __forceinline__ void col_running_lane(float& rm, float& rv, float mean, float var, float mo, float ub) {
  rm = (1.f - mo) * rm + mo * mean;
  rv = (1.f - mo) * rv + mo * (var * ub);
}

// UNR: unroll of the row loop; FL: slabs a finalizing lane loads ahead
template <ColMode MODE, int UNR, int FL>
__device__ __forceinline__ void col_reduce_body(const ColArgs& a) {
  __shared__ __align__(16) float4 red[2][256];         // 8 KB, also the double scratch of the finalize tail
  const ColGeom& g = a.g;
  const int C = a.C;
  const int tx = threadIdx.x % g.TX, ty = threadIdx.x / g.TX;
  const int c = blockIdx.y * g.CB + tx * 4;
  const int grp = blockIdx.z;
  const long r0 = grp * g.Mg + (long)blockIdx.x * g.rows_per_slab;
  const long r1 = min((grp + 1) * g.Mg, r0 + g.rows_per_slab);
  const ColChan ch = col_chan<MODE>(a, grp, c);
  const float4 z4 = make_float4(0, 0, 0, 0);
  float4 s1 = z4, s2 = z4;
#pragma unroll UNR
  for (long r = r0 + ty; r < r1; r += g.TY) {
    const ColTerm t = col_term<MODE>(a, ch, r * C + c);
    s1.x += t.f1.x; s1.y += t.f1.y; s1.z += t.f1.z; s1.w += t.f1.w;
    if constexpr (col_two_sums(MODE)) {
      s2.x = fmaf(t.f1.x, t.w.x, s2.x); s2.y = fmaf(t.f1.y, t.w.y, s2.y);
      s2.z = fmaf(t.f1.z, t.w.z, s2.z); s2.w = fmaf(t.f1.w, t.w.w, s2.w);
    }
  }
  const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
      a.partial, 0, (int)((size_t)g.G * g.nslab * 2 * C * sizeof(float)), 0x00020000);
  if (!col_publish(a, red, prs, s1, s2, tx, ty, c, grp)) return;

  // ---- finalize (last arriver of this channel block): all groups, slabs summed in slab order in double ------------
  constexpr int L = MODE == kColStatsPartials ? 2 : 4;      // statistics of this thread: channels cs .. cs + L - 1
  const int cs = MODE == kColStatsPartials ? c >> 1 : c;
  const long n = MODE == kColStatsPartials ? a.rows_real : g.Mg;
  float4 accg1 = z4, accg2 = z4;                            // sums over groups (parameter gradients)
  float rm[4] = {0, 0, 0, 0}, rv[4] = {0, 0, 0, 0};
  if (col_is_stats(MODE) && a.running_mean && ty == 0) {
    ld_lanes<L>(a.running_mean + cs, rm);
    ld_lanes<L>(a.running_var + cs, rv);
  }
  for (int gi = 0; gi < g.G; ++gi) {
    double d1[4], d2[4];
    col_slab_sums<FL>(a, reinterpret_cast<double*>(&red[0][0]), prs, gi, tx, ty, c, d1, d2);
    if (ty != 0) continue;
    if constexpr (col_is_stats(MODE)) {
      float piv[4] = {0, 0, 0, 0}, mf[4], vf[4];
      if constexpr (MODE == kColStats) ld_lanes<4>(a.x + (size_t)gi * g.Mg * C + c, piv);
      else if (a.pivot) ld_lanes<2>(a.pivot + cs, piv);
      const double inv = 1.0 / (double)n;
#pragma unroll
      for (int e = 0; e < L; ++e) {
        if constexpr (MODE == kColStats) col_stat_lane(d1[e] / (double)n, d2[e] / (double)n, piv[e], mf[e], vf[e]);
        else col_stat_lane(d1[2 * e] * inv, d1[2 * e + 1] * inv, piv[e], mf[e], vf[e]);      // columns: (S1, S2) per channel
      }
      st_lanes<L>(a.out1 + (size_t)gi * a.out_stride + cs, mf);
      st_lanes<L>(a.out2 + (size_t)gi * a.out_stride + cs, vf);
      if (a.running_mean) {               // one update per group, in group order = the order of the reference's per-camera calls
#pragma unroll
        for (int e = 0; e < L; ++e) col_running_lane(rm[e], rv[e], mf[e], vf[e], a.momentum, a.unbias);
      }
    } else {
      const float4 f1 = make_float4((float)d1[0], (float)d1[1], (float)d1[2], (float)d1[3]);
      const float4 f2 = make_float4((float)d2[0], (float)d2[1], (float)d2[2], (float)d2[3]);
      *reinterpret_cast<float4*>(a.out1 + (size_t)gi * a.out_stride + c) = f1;
      if (MODE != kColBwdPartials) *reinterpret_cast<float4*>(a.out2 + (size_t)gi * a.out_stride + c) = f2;
      accg1.x += f1.x; accg1.y += f1.y; accg1.z += f1.z; accg1.w += f1.w;
      accg2.x += f2.x; accg2.y += f2.y; accg2.z += f2.z; accg2.w += f2.w;
    }
    if (a.count_out && blockIdx.y == 0 && tx == 0) a.count_out[(size_t)gi * a.out_stride] = (float)n;
  }
  if (ty != 0) return;
  if constexpr (col_is_stats(MODE)) {
    if (a.running_mean) {
      st_lanes<L>(a.running_mean + cs, rm);
      st_lanes<L>(a.running_var + cs, rv);
    }
  } else if (a.acc1) {                                       // parameter gradients accumulated in place (.grad arena)
    if constexpr (MODE == kColBwdPartials) {                 // columns [0, C/2): dbeta, [C/2, C): dgamma
      const int half = C >> 1;
      grad_add4(c < half ? a.acc1 + c : a.acc2 + (c - half), accg1);
    } else {
      grad_add4(a.acc1 + c, accg1);
      grad_add4(a.acc2 + c, accg2);
    }
  }
}

// kColBwdDual: the row loop with a third accumulator, then publish + finalize once per norm, the second time with the second
// norm's partials, tickets, outputs and accumulators.  Each norm's sums take the path a reduction of its own takes (slab
// geometry, lane order, double finalize): the same bits.  A body of its own, so that the code of the other modes - and with it
// the last bits of every statistic they have ever written - stays what it is.
template <int UNR, int FL>
__device__ __forceinline__ void col_reduce_dual_body(const ColArgs& a0) {
  __shared__ __align__(16) float4 red[2][256];
  const ColGeom& g = a0.g;
  const int C = a0.C;
  const int tx = threadIdx.x % g.TX, ty = threadIdx.x / g.TX;
  const int c = blockIdx.y * g.CB + tx * 4;
  const int grp = blockIdx.z;
  const long r0 = grp * g.Mg + (long)blockIdx.x * g.rows_per_slab;
  const long r1 = min((grp + 1) * g.Mg, r0 + g.rows_per_slab);
  const ColChan ch = col_chan<kColBwdDual>(a0, grp, c);
  const float4 z4 = make_float4(0, 0, 0, 0);
  float4 s1 = z4, s2 = z4, s3 = z4;
#pragma unroll UNR
  for (long r = r0 + ty; r < r1; r += g.TY) {
    const ColTerm t = col_term<kColBwdDual>(a0, ch, r * C + c);
    s1.x += t.f1.x; s1.y += t.f1.y; s1.z += t.f1.z; s1.w += t.f1.w;
    s2.x = fmaf(t.f1.x, t.w.x, s2.x); s2.y = fmaf(t.f1.y, t.w.y, s2.y);
    s2.z = fmaf(t.f1.z, t.w.z, s2.z); s2.w = fmaf(t.f1.w, t.w.w, s2.w);
    s3.x = fmaf(t.f1.x, t.w2.x, s3.x); s3.y = fmaf(t.f1.y, t.w2.y, s3.y);
    s3.z = fmaf(t.f1.z, t.w2.z, s3.z); s3.w = fmaf(t.f1.w, t.w2.w, s3.w);
  }
  for (int norm = 0; norm < 2; ++norm) {
    ColArgs a = a0;
    if (norm) {
      a.partial = a0.second.partial; a.ticket = a0.second.ticket;
      a.out1 = a0.second.out1; a.out2 = a0.second.out2; a.acc1 = a0.second.acc1; a.acc2 = a0.second.acc2;
      __syncthreads();                                    // (the first norm's finalize is done with `red`)
    }
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
        a.partial, 0, (int)((size_t)g.G * g.nslab * 2 * C * sizeof(float)), 0x00020000);
    if (!col_publish(a, red, prs, s1, norm ? s3 : s2, tx, ty, c, grp)) continue;
    float4 accg1 = z4, accg2 = z4;                        // sums over groups (parameter gradients)
    for (int gi = 0; gi < g.G; ++gi) {
      double d1[4], d2[4];
      col_slab_sums<FL>(a, reinterpret_cast<double*>(&red[0][0]), prs, gi, tx, ty, c, d1, d2);
      if (ty != 0) continue;
      const float4 f1 = make_float4((float)d1[0], (float)d1[1], (float)d1[2], (float)d1[3]);
      const float4 f2 = make_float4((float)d2[0], (float)d2[1], (float)d2[2], (float)d2[3]);
      *reinterpret_cast<float4*>(a.out1 + (size_t)gi * a.out_stride + c) = f1;
      *reinterpret_cast<float4*>(a.out2 + (size_t)gi * a.out_stride + c) = f2;
      accg1.x += f1.x; accg1.y += f1.y; accg1.z += f1.z; accg1.w += f1.w;
      accg2.x += f2.x; accg2.y += f2.y; accg2.z += f2.z; accg2.w += f2.w;
    }
    if (ty == 0 && a.acc1) {                              // parameter gradients accumulated in place (.grad arena)
      grad_add4(a.acc1 + c, accg1);
      grad_add4(a.acc2 + c, accg2);
    }
  }
}

// (the kernels keep an int parameter: col_reduce_kernel<1> stays the name that the recorded profiles carry)
template <int MODE>
__global__ __launch_bounds__(256) void col_reduce_kernel(ColArgs a) {
  __builtin_amdgcn_s_setprio(XAS_BN_PRIO);
  if constexpr (MODE == kColBwdDual) col_reduce_dual_body<4, 4>(a);
  else col_reduce_body<(ColMode)MODE, 4, 4>(a);
}

// Same kernel compiled for at most 64 VGPRs: shipped for the backward sums in r04, when they ran beside two weight-gradient
// blocks per CU (which leave 112 VGPRs per SIMD lane - room for two lean waves instead of one).  On ONE stream (r05) the
// build above is 0.7 ms/step faster (in-box, interleaved, 5 rounds: 126.95 -> 126.24) and is the shipped one;
// XAS_TUNE_COL_REDUCE_LEAN selects this build.  What the compiler reports (gfx950, -O3): the build above takes 126 VGPRs for
// kColStats, 120 for kColBwdXY / kColSum / kColBwdY / kColBwdX (4 waves per SIMD), 92 and 84 for the two partials modes
// (5 waves), no scratch; this one 64 VGPRs (8 waves) and SPILLS 12 bytes of scratch per lane in each of its three modes.
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
void col_reduce_lean_kernel(ColArgs a) {
  __builtin_amdgcn_s_setprio(XAS_BN_PRIO);
  if constexpr (MODE == kColBwdDual) col_reduce_dual_body<2, 2>(a);
  else col_reduce_body<(ColMode)MODE, 2, 2>(a);
}

// SyncBatchNorm: merge the per-rank statistics of every group.  gathered: [world][G][msg_stride] = mean | biased var |
// count (| padding) per (rank, group).  Count-weighted merge in double (Chan et al.: total M2 = sum n_i (var_i + (mean_i - mean)^2)),
// then the running-statistic update of each group in group order with the GLOBAL count.
__global__ void bn_sync_merge_kernel(const float* __restrict__ gathered, int world, int G, int C, long msg_stride,
                                     float* __restrict__ mean, float* __restrict__ var,
                                     float* __restrict__ running_mean, float* __restrict__ running_var, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const size_t stride = (size_t)msg_stride;
  float rm = running_mean ? running_mean[c] : 0.f, rv = running_var ? running_var[c] : 0.f;
  for (int g = 0; g < G; ++g) {
    double n = 0.0, mu = 0.0;
    for (int r = 0; r < world; ++r) {
      const float* p = gathered + ((size_t)r * G + g) * stride;
      const double cnt = (double)p[2 * C];
      n += cnt; mu += cnt * (double)p[c];
    }
    mu /= n;
    double m2 = 0.0;
    for (int r = 0; r < world; ++r) {
      const float* p = gathered + ((size_t)r * G + g) * stride;
      const double d = (double)p[c] - mu;
      m2 += (double)p[2 * C] * ((double)p[C + c] + d * d);
    }
    const float mf = (float)mu, vf = (float)(m2 / n);
    mean[(size_t)g * C + c] = mf;
    var[(size_t)g * C + c] = vf;
    if (running_mean) {
      const float unbias = n > 1.0 ? (float)(n / (n - 1.0)) : 1.f;
      rm = (1.f - momentum) * rm + momentum * mf;
      rv = (1.f - momentum) * rv + momentum * (vf * unbias);
    }
  }
  if (running_mean) { running_mean[c] = rm; running_var[c] = rv; }
}

// ---------------------------------------------------------------- the two element-wise passes (apply, backward apply)
// The arithmetic of an element is written ONCE per pass (bn_fwd_elem, bn_bwd_elem); a kernel template per pass wraps it in
// one of two loop policies:
//   streaming: the threads of a grid row are a multiple of C/4, so a thread keeps ONE channel quadruple: its per-channel
//              quantities are read once, the loop is unrolled 4x with non-temporal 16-byte loads issued ahead plus a tail,
//              non-temporal stores, the mode a template argument (no branches) - in the backward pass these kernels share
//              the chip with two weight-gradient blocks per CU and get few wave slots;
//   general  : grid-stride loop, channel quadruple from i % C4 in every trip, plain loads and stores, the mode read at run
//              time from `act` and from which pointers are null: every combination the entry points accept.
// bn_stream_grid (host) picks the policy.  The sign / xhat helpers of bn_bwd_elem are those of the backward sums (col_term,
// above); the convolution epilogues (conv_shared.h) keep their own copy under their register budget.
__device__ __forceinline__ float act_fwd(float v, int act) {
  return act == 0 ? v : (act == 1 ? fmaxf(v, 0.f) : (v > 0.f ? v : 0.01f * v));
}

// the per-channel quantities of one channel quadruple
struct BnChan {
  float4 m, is, rs, g, bt;   // mean, rstd, rstd * gamma (rounded once: bn_affine's contract), gamma, beta
  float4 a, b;               // backward: sum dz, sum dz xhat of the group
};

// of float4 element i of group blockIdx.y.  BWD: with the two sums, and beta may be null where the mode does not read it
template <bool BWD>
__device__ __forceinline__ BnChan bn_chan(const float* mean, const float* var, const float* gamma, const float* beta,
                                          const float* sums, float eps, int C4, long i) {
  const int c = (int)(i % C4) * 4;
  BnChan ch;
  const size_t gc = (size_t)blockIdx.y * C4 * 4 + c;
  ch.m = *reinterpret_cast<const float4*>(mean + gc);
  const float4 v = *reinterpret_cast<const float4*>(var + gc);
  ch.g = *reinterpret_cast<const float4*>(gamma + c);
  ch.bt = (!BWD || beta) ? *reinterpret_cast<const float4*>(beta + c) : make_float4(0, 0, 0, 0);   // (a value, not an lvalue: ONE load)
  ch.a = BWD ? *reinterpret_cast<const float4*>(sums + (size_t)blockIdx.y * C4 * 8 + c) : make_float4(0, 0, 0, 0);
  ch.b = BWD ? *reinterpret_cast<const float4*>(sums + (size_t)blockIdx.y * C4 * 8 + (size_t)C4 * 4 + c) : make_float4(0, 0, 0, 0);
  ch.is = make_float4(rsqrtf(v.x + eps), rsqrtf(v.y + eps), rsqrtf(v.z + eps), rsqrtf(v.w + eps));
  ch.rs = make_float4(__fmul_rn(ch.is.x, ch.g.x), __fmul_rn(ch.is.y, ch.g.y), __fmul_rn(ch.is.z, ch.g.z), __fmul_rn(ch.is.w, ch.g.w));
  return ch;
}

template <bool NT> __device__ __forceinline__ void ew_store(float4* p, float4 v) { if (NT) stream_store(p, v); else *p = v; }

// -> y = act((x - mean) * (rstd * gamma) + beta [+ residual]); amx: running max |y|.  has_mask: *mask = sign bits of the
// pre-activation value (bit e = lane e > 0): what the backward needs of y, 1/16 of its bytes
__device__ __forceinline__ float4 bn_fwd_elem(const BnChan& ch, float4 xv, float4 rv, int act, bool res, bool has_mask,
                                              uint8_t* mask, float& amx) {
  float4 o;
  o.x = bn_affine(xv.x, ch.m.x, ch.rs.x, ch.bt.x); o.y = bn_affine(xv.y, ch.m.y, ch.rs.y, ch.bt.y);
  o.z = bn_affine(xv.z, ch.m.z, ch.rs.z, ch.bt.z); o.w = bn_affine(xv.w, ch.m.w, ch.rs.w, ch.bt.w);
  if (res) { o.x += rv.x; o.y += rv.y; o.z += rv.z; o.w += rv.w; }
  if (has_mask) *mask = (uint8_t)((o.x > 0.f ? 1u : 0u) | (o.y > 0.f ? 2u : 0u) | (o.z > 0.f ? 4u : 0u) | (o.w > 0.f ? 8u : 0u));
  o.x = act_fwd(o.x, act); o.y = act_fwd(o.y, act); o.z = act_fwd(o.z, act); o.w = act_fwd(o.w, act);
  amx = amax4(amx, o);
  return o;
}

// sign: where the activation sign comes from: 0 no activation, 1 y, 2 x (re-derived with bn_affine: the forward's decision
//       bit for bit; layers without a residual), 3 mask bytes
// xh  : normalised input from x (true) or recovered from y (false: z = act^-1(y), xhat = (z - beta) / gamma; leaky ReLU)
// dz  : dy, then the gradient at the pre-activation value = the residual's gradient, stored to *dres if has_dres
// -> dx; amx: running max |dx|
template <bool NT>
__device__ __forceinline__ float4 bn_bwd_elem(const BnChan& ch, float inv_count, float4 xv, float4 yv, float4 dz, unsigned mb,
                                              int act, int sign, bool xh_from_x, bool has_dres, float4* dres, float& amx) {
  const float neg = act_neg_slope(act);
  const float4 &m = ch.m, &is = ch.is, &rs = ch.rs, &g = ch.g, &bt = ch.bt, &a = ch.a, &b = ch.b;
  if (sign == 1) dz = dz_sign_y(dz, yv, neg);
  else if (sign == 2) dz = dz_sign_x(dz, xv, m, rs, bt, neg);
  else if (sign == 3) dz = dz_sign_mask(dz, mb, neg);
  if (has_dres) ew_store<NT>(dres, dz);
  float4 xh;
  if (xh_from_x) xh = xhat4(xv, m, is);
  else {                                               // (a division here, where the sums multiply by 1 / gamma)
    const float4 z = act_inv4(yv, act);
    xh.x = g.x != 0.f ? (z.x - bt.x) / g.x : 0.f; xh.y = g.y != 0.f ? (z.y - bt.y) / g.y : 0.f;
    xh.z = g.z != 0.f ? (z.z - bt.z) / g.z : 0.f; xh.w = g.w != 0.f ? (z.w - bt.w) / g.w : 0.f;
  }
  float4 o;
  o.x = g.x * is.x * (dz.x - a.x * inv_count - xh.x * b.x * inv_count);
  o.y = g.y * is.y * (dz.y - a.y * inv_count - xh.y * b.y * inv_count);
  o.z = g.z * is.z * (dz.z - a.z * inv_count - xh.z * b.z * inv_count);
  o.w = g.w * is.w * (dz.w - a.w * inv_count - xh.w * b.w * inv_count);
  amx = fmaxf(fmaxf(amx, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
  return o;
}

// grid.y = group: the rows of group g use mean / var row g ([G][C]); n4g = float4 elements per group.
// STREAM: mode = <ACT, RES, MASKOUT>; general: mode = (act, res != null, mask_out != null)
template <bool STREAM, int ACT = 0, bool RES = false, bool MASKOUT = false>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float4* __restrict__ x, const float* __restrict__ mean,
                                                      const float* __restrict__ var, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float4* __restrict__ res,
                                                      float eps, int act_rt, long n4g, int C4, float4* __restrict__ y,
                                                      uint8_t* __restrict__ mask_out, float* __restrict__ amax_out) {
  const int act = STREAM ? ACT : act_rt;
  const bool has_res = STREAM ? RES : res != nullptr, has_mask = STREAM ? MASKOUT : mask_out != nullptr;
  float amx = 0.f;                                     // max |y| of this thread (amax_out != null: xas_bn_apply_amax)
  if (STREAM) __builtin_amdgcn_s_setprio(XAS_BN_PRIO);
  const long goff = (long)blockIdx.y * n4g;
  const long stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  BnChan ch;
  auto one = [&](long k, float4 xv, float4 rv) {
    ew_store<STREAM>(y + goff + k, bn_fwd_elem(ch, xv, rv, act, has_res, has_mask, mask_out + goff + k, amx));
  };
  const float4 z4 = make_float4(0, 0, 0, 0);
  if (STREAM) {
    ch = bn_chan<false>(mean, var, gamma, beta, nullptr, eps, C4, i);
    for (; i + 3 * stride < n4g; i += 4 * stride) {
      float4 xv[4], rv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { xv[u] = stream_load(x + goff + i + u * stride); rv[u] = has_res ? stream_load(res + goff + i + u * stride) : z4; }
#pragma unroll
      for (int u = 0; u < 4; ++u) one(i + u * stride, xv[u], rv[u]);
    }
  }
  for (; i < n4g; i += stride) {                       // streaming: the tail; general: the whole loop
    if (!STREAM) ch = bn_chan<false>(mean, var, gamma, beta, nullptr, eps, C4, i);
    one(i, x[goff + i], has_res ? res[goff + i] : z4);
  }
  if (amax_out) publish_amax(amax_out, amx);
}

// grid.y = group; sums: [G][2][C] = sum_dz | sum_dz_xhat of each group.
// STREAM: mode = <ACT, SIGN, XH, DRES>; general: mode = (act, mask ? 3 : y ? 1 : 2 under an activation, x != null, dres != null)
template <bool STREAM, int ACT = 0, int SIGN = 0, bool XH = true, bool DRES = false>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(
    const float4* __restrict__ x, const float4* __restrict__ y, const float4* __restrict__ dy, const float* __restrict__ mean,
    const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ sums, float eps, int act_rt, long n4g, int C4, float inv_count, float4* __restrict__ dx,
    float4* __restrict__ dres, const uint8_t* __restrict__ mask, float* __restrict__ amax_out) {
  const int act = STREAM ? ACT : act_rt;
  const int sign = STREAM ? SIGN : (act_rt == 0 ? 0 : mask ? 3 : y ? 1 : 2);
  const bool xh = STREAM ? XH : x != nullptr, has_dres = STREAM ? DRES : dres != nullptr;
  const bool needx = xh || sign == 2, needy = sign == 1 || !xh;
  if (STREAM) __builtin_amdgcn_s_setprio(XAS_BN_PRIO);
  float amx = 0.f;                                     // max |dx| of this thread (amax_out != null: xas_bn_bwd_apply_amax)
  const long goff = (long)blockIdx.y * n4g;
  const long stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  BnChan ch;
  auto one = [&](long k, float4 xv, float4 yv, float4 dz, unsigned mb) {
    ew_store<STREAM>(dx + goff + k, bn_bwd_elem<STREAM>(ch, inv_count, xv, yv, dz, mb, act, sign, xh, has_dres, dres + goff + k, amx));
  };
  const float4 z4 = make_float4(0, 0, 0, 0);
  if (STREAM) {
    ch = bn_chan<true>(mean, var, gamma, beta, sums, eps, C4, i);
    for (; i + 3 * stride < n4g; i += 4 * stride) {
      float4 xv[4], yv[4], dv[4];
      unsigned mb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long k = goff + i + u * stride;
        dv[u] = stream_load(dy + k);
        xv[u] = needx ? stream_load(x + k) : z4;
        yv[u] = needy ? stream_load(y + k) : z4;
        mb[u] = sign == 3 ? mask[k] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) one(i + u * stride, xv[u], yv[u], dv[u], mb[u]);
    }
  }
  for (; i < n4g; i += stride) {                       // streaming: the tail; general: the whole loop
    if (!STREAM) ch = bn_chan<true>(mean, var, gamma, beta, sums, eps, C4, i);
    const long k = goff + i;
    one(i, needx ? x[k] : z4, needy ? y[k] : z4, dy[k], sign == 3 ? mask[k] : 0u);
  }
  if (amax_out) publish_amax(amax_out, amx);
}

// ---- dual forms: the output of a block with a projection, out = relu(bn3(x) + bn_d(xd)), both norms [M][C] with the same
// groups.  The normalised skip bn_d(xd) and the residual gradient dz exist in registers only; an element goes through
// bn_fwd_elem / bn_bwd_elem once per norm, so the values are those of the single-norm kernels run one after the other.
struct BnNorm {
  const float* mean; const float* var; const float* gamma; const float* beta;      // beta: forward only
  const float* sums;                                                                // backward only: [G][2][C]
  float eps;
};

template <bool BWD>
__device__ __forceinline__ BnChan bn_chan(const BnNorm& n, int C4, long i) {
  return bn_chan<BWD>(n.mean, n.var, n.gamma, n.beta, n.sums, n.eps, C4, i);
}

// STREAM / general as bn_apply_kernel (the one mode: ReLU, sign bytes written)
template <bool STREAM>
__global__ __launch_bounds__(256) void bn_apply_dual_kernel(const float4* __restrict__ x, const float4* __restrict__ xd, BnNorm n3,
                                                           BnNorm nd, long n4g, int C4, float4* __restrict__ y,
                                                           uint8_t* __restrict__ mask_out, float* __restrict__ amax_out) {
  float amx = 0.f;                                     // max |y| of this thread
  if (STREAM) __builtin_amdgcn_s_setprio(XAS_BN_PRIO);
  const long goff = (long)blockIdx.y * n4g;
  const long stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  BnChan ch, chd;
  const float4 z4 = make_float4(0, 0, 0, 0);
  auto one = [&](long k, float4 xv, float4 dv) {
    float skip_amx = 0.f;                              // (the skip's maximum has no reader)
    const float4 skip = bn_fwd_elem(chd, dv, z4, 0, false, false, nullptr, skip_amx);
    ew_store<STREAM>(y + goff + k, bn_fwd_elem(ch, xv, skip, 1, true, true, mask_out + goff + k, amx));
  };
  if (STREAM) {
    ch = bn_chan<false>(n3, C4, i); chd = bn_chan<false>(nd, C4, i);
    for (; i + 3 * stride < n4g; i += 4 * stride) {
      float4 xv[4], dv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { xv[u] = stream_load(x + goff + i + u * stride); dv[u] = stream_load(xd + goff + i + u * stride); }
#pragma unroll
      for (int u = 0; u < 4; ++u) one(i + u * stride, xv[u], dv[u]);
    }
  }
  for (; i < n4g; i += stride) {                       // streaming: the tail; general: the whole loop
    if (!STREAM) { ch = bn_chan<false>(n3, C4, i); chd = bn_chan<false>(nd, C4, i); }
    one(i, x[goff + i], xd[goff + i]);
  }
  if (amax_out) publish_amax(amax_out, amx);
}

// -> dx (bn3's input gradient, sign from the mask bytes) and dxd (the projection norm's, no activation) from ONE dz
template <bool STREAM>
__global__ __launch_bounds__(256) void bn_bwd_apply_dual_kernel(
    const float4* __restrict__ x, const float4* __restrict__ xd, const float4* __restrict__ dy, const uint8_t* __restrict__ mask,
    BnNorm n3, BnNorm nd, long n4g, int C4, float inv_count, float inv_count_d, float4* __restrict__ dx, float4* __restrict__ dxd,
    float* __restrict__ amax_out, float* __restrict__ amax_d_out) {
  if (STREAM) __builtin_amdgcn_s_setprio(XAS_BN_PRIO);
  float amx = 0.f, amxd = 0.f;                         // max |dx|, max |dxd| of this thread
  const long goff = (long)blockIdx.y * n4g;
  const long stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  BnChan ch, chd;
  const float4 z4 = make_float4(0, 0, 0, 0);
  auto one = [&](long k, float4 xv, float4 dv, float4 dz, unsigned mb) {
    ew_store<STREAM>(dx + goff + k, bn_bwd_elem<STREAM>(ch, inv_count, xv, z4, dz, mb, 1, 3, true, false, nullptr, amx));
    const float4 dres = dz_sign_mask(dz, mb, act_neg_slope(1));          // what bn3's apply would have stored for the skip
    ew_store<STREAM>(dxd + goff + k, bn_bwd_elem<STREAM>(chd, inv_count_d, dv, z4, dres, 0u, 0, 0, true, false, nullptr, amxd));
  };
  if (STREAM) {
    ch = bn_chan<true>(n3, C4, i); chd = bn_chan<true>(nd, C4, i);
    for (; i + 3 * stride < n4g; i += 4 * stride) {
      float4 xv[4], dv[4], gv[4];
      unsigned mb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long k = goff + i + u * stride;
        gv[u] = stream_load(dy + k); xv[u] = stream_load(x + k); dv[u] = stream_load(xd + k); mb[u] = mask[k];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) one(i + u * stride, xv[u], dv[u], gv[u], mb[u]);
    }
  }
  for (; i < n4g; i += stride) {                       // streaming: the tail; general: the whole loop
    if (!STREAM) { ch = bn_chan<true>(n3, C4, i); chd = bn_chan<true>(nd, C4, i); }
    const long k = goff + i;
    one(i, x[k], xd[k], dy[k], mask[k]);
  }
  if (amax_out) publish_amax(amax_out, amx);
  __syncthreads();                                     // (publish_amax's LDS words are read by thread 0 after its barrier)
  if (amax_d_out) publish_amax(amax_d_out, amxd);
}

// one update per group, in group order (mean / var: [G][C])
__global__ void bn_running_kernel(const float* mean, const float* var, float* rm, float* rv, float momentum,
                                  float unbias, int C, int G) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float m = rm[c], v = rv[c];
  for (int g = 0; g < G; ++g) {
    m = (1.f - momentum) * m + momentum * mean[(size_t)g * C + c];
    v = (1.f - momentum) * v + momentum * (var[(size_t)g * C + c] * unbias);
  }
  rm[c] = m; rv[c] = v;
}

}  // namespace xas

using namespace xas;

extern "C" size_t xas_bn_workspace_floats(long M, int C, int groups) {
  ColGeom g;
  if (col_geom(M, C, groups, &g)) return 0;
  return (size_t)g.G * g.nslab * 2 * C + C;
}

#ifndef XAS_EW_CAP
#define XAS_EW_CAP 8192                  // blocks of a streaming launch over all groups (r05 re-sweep on one stream, in-box: 2048 +0.9 ms/step, 4096 +0.3, 8192 best, 16384 +0.4)
#endif
static inline unsigned ew_grid_g(long n_per_group, int groups) {
  long b = cdiv(n_per_group, 256);
  const long cap = groups > 1 ? cdiv(XAS_EW_CAP, groups) : XAS_EW_CAP;
  return (unsigned)(b > cap ? cap : (b < 1 ? 1 : b));
}

// The one rule "streaming or general policy" of the two apply passes -> grid.x of the streaming launch, or 0: general policy
// on ew_grid_g blocks.  Streaming needs the threads of a grid row to be a multiple of C/4: C/4 a power of two (it then
// divides 256, or above 256 the row is rounded up to whole multiples of C/4 threads).  XAS_TUNE_GENERAL_KERNELS sends every
// launch to the general policy (coverage).  Under this rule a launch is streaming in the modes of these tables, else general:
//   forward  <ACT, RES, MASKOUT>, 9 modes: act 0 / 1 / 2 x { no residual: <act, false, false> (a mask_out WITHOUT a residual
//            is not written by this policy), residual: <act, true, false>, residual and mask_out: <act, true, true> }
//   backward <ACT, SIGN, XH, DRES>, 7 modes (bn_bwd_elem explains SIGN and XH):
//            0  act 0, x, no dresidual                 <0, 0, true, false>   projection norms
//            1  act 1, x, no y, no mask, no dresidual  <1, 2, true, false>   ReLU without residual (sign re-derived from x)
//            2  act 2, no x, y, no dresidual           <2, 1, false, false>  leaky ReLU without x (physique net)
//            3  act 1, x, y, no mask, dresidual        <1, 1, true, true>    residual layers, sign from y
//            4  act 1, x, y, no mask, no dresidual     <1, 1, true, false>
//            5  act 1, x, mask, dresidual              <1, 3, true, true>    residual layers, sign from the mask bytes
//            6  act 1, x, mask, no dresidual           <1, 3, true, false>
//   general only: act 0 with dresidual; leaky ReLU with x (with or without y / mask / dresidual); C/4 not a power of two.
static unsigned bn_stream_grid(long n4g, int C4, int groups, int tune) {
  if ((C4 & (C4 - 1)) != 0 || (tune & XAS_TUNE_GENERAL_KERNELS)) return 0;
  unsigned gx = ew_grid_g(n4g, groups);
  if (C4 > 256) gx = (gx + (C4 / 256) - 1) / (C4 / 256) * (C4 / 256);
  return gx;
}

using BnFwdKernel = decltype(&bn_apply_kernel<false>);          // both policies of a pass share one signature
using BnBwdKernel = decltype(&bn_bwd_apply_kernel<false>);

static BnFwdKernel bn_fwd_stream_kernel(int act, bool res, bool mask_out) {
#define XAS_BN_FWD(ACT) {bn_apply_kernel<true, ACT, false, false>, bn_apply_kernel<true, ACT, true, false>, bn_apply_kernel<true, ACT, true, true>}
  static const BnFwdKernel k[3][3] = {XAS_BN_FWD(0), XAS_BN_FWD(1), XAS_BN_FWD(2)};
#undef XAS_BN_FWD
  return k[act][res ? (mask_out ? 2 : 1) : 0];
}

// (act, which operands are present) -> the streaming kernel of the backward's mode, or null: general
static BnBwdKernel bn_bwd_stream_kernel(int act, bool x, bool y, bool mask, bool dres) {
  const int sign = act == 0 ? 0 : mask ? 3 : y ? 1 : 2;
  static const struct { int act, sign; bool xh, dres; BnBwdKernel k; } modes[7] = {
#define XAS_BN_BWD(ACT, SIGN, XH, DR) {ACT, SIGN, XH, DR, bn_bwd_apply_kernel<true, ACT, SIGN, XH, DR>}
      XAS_BN_BWD(0, 0, true, false), XAS_BN_BWD(1, 2, true, false), XAS_BN_BWD(2, 1, false, false), XAS_BN_BWD(1, 1, true, true),
      XAS_BN_BWD(1, 1, true, false), XAS_BN_BWD(1, 3, true, true), XAS_BN_BWD(1, 3, true, false)};
#undef XAS_BN_BWD
  for (const auto& m : modes)
    if (m.act == act && m.sign == sign && m.xh == x && m.dres == dres) return m.k;
  return nullptr;
}

// (act, which operands are present) -> the mode of the backward sums: the `sign` rule of bn_bwd_stream_kernel (mask bytes,
// else y, else re-derived from x), and without x the form that recovers xhat from y
static ColMode bn_bwd_reduce_mode(int act, bool x, bool y, bool mask) {
  if (!x) return kColBwdY;
  return act != 0 && !mask && !y ? kColBwdX : kColBwdXY;
}

static int col_args(ColArgs* a, const ColGeom& g, long M, int C, float* workspace) {
  a->M = M; a->C = C; a->g = g; a->partial = workspace;
  a->ticket = take_tickets(g.ncb);
  XAS_REQUIRE(a->ticket != nullptr, "column reduce: could not allocate the ticket counters");
  XAS_REQUIRE((size_t)g.G * g.nslab * 2 * C * sizeof(float) < 0x7fffff00ul, "column reduce: partial buffer too large");
  return 0;
}

// the one launch of the column reductions (grid: slabs x channel blocks x groups of a.g); lean: col_reduce_lean_kernel,
// built for the backward sums only
template <ColMode MODE>
static int launch_col_reduce(const ColArgs& a, bool lean, void* stream) {
  auto k = col_reduce_kernel<MODE>;
  if constexpr (col_is_bwd(MODE)) if (lean) k = col_reduce_lean_kernel<MODE>;
  hipLaunchKernelGGL(k, dim3(a.g.nslab, a.g.ncb, a.g.G), dim3(256), 0, as_stream(stream), a);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_bn_stats(const float* x, long M, int C, int groups, float* mean, float* var_biased, long out_stride,
                            float* count_out, float* workspace, float* running_mean, float* running_var, float momentum,
                            long count, void* stream) {
  ColGeom g;
  if (col_geom(M, C, groups, &g)) return 1;
  XAS_REQUIRE(x && mean && var_biased && workspace && out_stride >= C, "bn_stats: null buffer / bad stride");
  XAS_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_stats: running buffers come in pairs");
  XAS_REQUIRE((((uintptr_t)mean | (uintptr_t)var_biased) & 15) == 0 && out_stride % 4 == 0,
              "bn_stats: outputs must be 16-byte aligned (out_stride a multiple of 4 floats)");
  ColArgs a{};
  if (col_args(&a, g, M, C, workspace)) return 1;
  a.x = x; a.out1 = mean; a.out2 = var_biased; a.out_stride = out_stride; a.count_out = count_out;
  a.running_mean = running_mean; a.running_var = running_var; a.momentum = momentum;
  a.unbias = count > 1 ? (float)((double)count / (double)(count - 1)) : 1.f;
  return launch_col_reduce<kColStats>(a, false, stream);
}

// Statistics from the per-tile partial sums a convolution epilogue left (xas_conv_fwd_bnstats): partial is
// [groups * tiles_per_group... rows][C][2] = (sum(v - pivot), sum((v - pivot)^2)) over rows_per_group / (rows / groups)
// activation rows each.  One launch: column sums of the [rows][2C] matrix + folded finalize.
extern "C" int xas_bn_stats_from_partials(const float* partial, long rows, int C, int groups, long rows_per_group,
                                          const float* pivot, float* mean, float* var_biased, long out_stride,
                                          float* count_out, float* workspace, float* running_mean, float* running_var,
                                          float momentum, void* stream) {
  ColGeom g;
  if (col_geom(rows, 2 * C, groups, &g)) return 1;
  XAS_REQUIRE(partial && mean && var_biased && workspace && out_stride >= C && rows_per_group > 0,
              "bn_stats_from_partials: null buffer / bad stride");
  XAS_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_stats_from_partials: running buffers come in pairs");
  XAS_REQUIRE((((uintptr_t)mean | (uintptr_t)var_biased | (uintptr_t)partial) & 15) == 0 && out_stride % 4 == 0 && C % 4 == 0,
              "bn_stats_from_partials: buffers must be 16-byte aligned, C and out_stride multiples of 4");
  ColArgs a{};
  if (col_args(&a, g, rows, 2 * C, workspace)) return 1;
  a.x = partial; a.pivot = pivot; a.out1 = mean; a.out2 = var_biased; a.out_stride = out_stride; a.count_out = count_out;
  a.running_mean = running_mean; a.running_var = running_var; a.momentum = momentum;
  a.rows_real = rows_per_group;
  a.unbias = rows_per_group > 1 ? (float)((double)rows_per_group / (double)(rows_per_group - 1)) : 1.f;
  return launch_col_reduce<kColStatsPartials>(a, false, stream);
}

// Batch-norm backward sums from the per-tile partial sums a data-gradient epilogue left (xas_conv_dgrad_bn_bwd):
// partial [rows][2][C] (sum dz | sum dz * xhat over the activation rows of a tile) -> sums [groups][2][C], and the LOCAL
// parameter gradients added into dbeta_acc / dgamma_acc (may be NULL).
extern "C" int xas_bn_bwd_sums_from_partials(const float* partial, long rows, int C, int groups, float* sums,
                                             float* workspace, float* dbeta_acc, float* dgamma_acc, void* stream) {
  ColGeom g;
  if (col_geom(rows, 2 * C, groups, &g)) return 1;
  XAS_REQUIRE(partial && sums && workspace && C % 4 == 0, "bn_bwd_sums_from_partials: null buffer / C not a multiple of 4");
  XAS_REQUIRE((dbeta_acc == nullptr) == (dgamma_acc == nullptr), "bn_bwd_sums_from_partials: gradient accumulators come in pairs");
  ColArgs a{};
  if (col_args(&a, g, rows, 2 * C, workspace)) return 1;
  a.x = partial; a.out1 = sums; a.out_stride = 2 * (long)C;
  a.out2 = nullptr;                                                    // (no second sums in this mode)
  a.acc1 = dbeta_acc; a.acc2 = dgamma_acc;
  return launch_col_reduce<kColBwdPartials>(a, false, stream);
}

extern "C" int xas_bn_sync_merge(const float* gathered, int world, int groups, int C, long msg_stride, float* mean,
                                 float* var_biased, float* running_mean, float* running_var, float momentum,
                                 void* stream) {
  XAS_REQUIRE(gathered && mean && var_biased && world >= 1 && groups >= 1 && C >= 1 && msg_stride >= 2 * (long)C + 1,
              "bn_sync_merge: bad arguments");
  XAS_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_sync_merge: running buffers come in pairs");
  hipLaunchKernelGGL(bn_sync_merge_kernel, dim3((unsigned)cdiv(C, 64)), dim3(64), 0, as_stream(stream), gathered, world,
                     groups, C, msg_stride, mean, var_biased, running_mean, running_var, momentum);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_col_sum(const float* x, long M, int C, float* out, float* workspace, void* stream) {
  ColGeom g;
  if (col_geom(M, C, 1, &g)) return 1;
  XAS_REQUIRE(x && out && workspace, "col_sum: null buffer");
  ColArgs a{};
  if (col_args(&a, g, M, C, workspace)) return 1;
  a.x = x; a.out1 = out; a.out2 = workspace + (size_t)g.nslab * 2 * C;     // second sums are unused: workspace tail
  a.out_stride = C;
  return launch_col_reduce<kColSum>(a, false, stream);
}

extern "C" int xas_bn_apply(const float* x, const float* mean, const float* var_biased, const float* gamma,
                            const float* beta, const float* residual, float eps, int act, long M, int C, int groups,
                            float* y, uint8_t* mask_out, void* stream) {
  return xas_bn_apply_amax(x, mean, var_biased, gamma, beta, residual, eps, act, M, C, groups, y, mask_out, nullptr, stream);
}

extern "C" int xas_bn_apply_amax(const float* x, const float* mean, const float* var_biased, const float* gamma,
                                 const float* beta, const float* residual, float eps, int act, long M, int C, int groups,
                                 float* y, uint8_t* mask_out, float* amax_out, void* stream) {
  XAS_REQUIRE(x && mean && var_biased && gamma && beta && y, "bn_apply: null buffer");
  XAS_REQUIRE(M > 0 && C >= 4 && C % 4 == 0 && act >= 0 && act <= 2 && groups >= 1 && M % groups == 0,
              "bn_apply: bad shape M=%ld C=%d act=%d groups=%d", M, C, act, groups);
  const int C4 = C / 4;
  const long n4g = (M / groups) * C4;
  const unsigned gs = bn_stream_grid(n4g, C4, groups, tune_flags());
  const BnFwdKernel k = gs ? bn_fwd_stream_kernel(act, residual != nullptr, mask_out != nullptr) : bn_apply_kernel<false>;
  hipLaunchKernelGGL(k, dim3(gs ? gs : ew_grid_g(n4g, groups), groups), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(x), mean, var_biased, gamma, beta,
                     reinterpret_cast<const float4*>(residual), eps, act, n4g, C4, reinterpret_cast<float4*>(y), mask_out,
                     amax_out);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_bn_update_running(const float* mean, const float* var_biased, float* running_mean,
                                     float* running_var, float momentum, long count, int C, int groups, void* stream) {
  XAS_REQUIRE(mean && var_biased && running_mean && running_var && C > 0 && count > 0 && groups >= 1,
              "bn_update_running: bad arguments");
  const float unbias = count > 1 ? (float)((double)count / (double)(count - 1)) : 1.f;
  hipLaunchKernelGGL(bn_running_kernel, dim3((unsigned)cdiv(C, 64)), dim3(64), 0, as_stream(stream), mean, var_biased,
                     running_mean, running_var, momentum, unbias, C, groups);
  XAS_LAUNCH_CHECK();
  return 0;
}

// acc[c] += sum over rows of x[:, c] (bias gradients added straight into the gradient arena, on the weight-gradient stream)
extern "C" int xas_col_sum_acc(const float* x, long M, int C, float* acc, float* workspace, void* stream) {
  ColGeom g;
  if (col_geom(M, C, 1, &g)) return 1;
  XAS_REQUIRE(x && acc && workspace && (((uintptr_t)acc) & 15) == 0, "col_sum_acc: null / misaligned buffer");
  ColArgs a{};
  if (col_args(&a, g, M, C, workspace)) return 1;
  float* scratch = workspace + (size_t)g.nslab * 2 * C;                 // C floats: plain sums, second sums and their accumulator
  a.x = x; a.out1 = scratch; a.out2 = scratch; a.out_stride = C;
  a.acc1 = acc; a.acc2 = scratch;
  return launch_col_reduce<kColSum>(a, false, stream);
}

extern "C" int xas_bn_bwd_reduce(const float* x, const float* y, const float* dy, const float* mean,
                                 const float* var_biased, const float* gamma, const float* beta, float eps, int act,
                                 long M, int C, int groups, float* sums, float* workspace,
                                 float* dbeta_acc, float* dgamma_acc, const uint8_t* mask, void* stream) {
  ColGeom g;
  if (col_geom(M, C, groups, &g)) return 1;
  XAS_REQUIRE(!mask || (x && act != 0), "bn_bwd_reduce: the sign-mask form needs x and an activation");
  XAS_REQUIRE(dy && mean && var_biased && sums && workspace && (act == 0 || y || mask || (x && gamma && beta)),
              "bn_bwd_reduce: null buffer (an activation needs y, or x with gamma and beta)");
  XAS_REQUIRE(x || (act != 0 && y && gamma && beta), "bn_bwd_reduce: without x the layer needs an activation, y, gamma, beta");
  XAS_REQUIRE((dbeta_acc == nullptr) == (dgamma_acc == nullptr), "bn_bwd_reduce: gradient accumulators come in pairs");
  const bool lean = (tune_flags() & XAS_TUNE_COL_REDUCE_LEAN) != 0;      // shipped: col_reduce_kernel (the flag selects the <= 64-VGPR build: see col_reduce_lean_kernel)
  ColArgs a{};
  if (col_args(&a, g, M, C, workspace)) return 1;
  a.x = x; a.y = y; a.dy = dy; a.mask = mask; a.mean = mean; a.var = var_biased; a.gamma = gamma; a.beta = beta;
  a.eps = eps; a.act = act;
  a.out1 = sums; a.out2 = sums + C; a.out_stride = 2 * (long)C;            // [G][2][C]
  a.acc1 = dbeta_acc; a.acc2 = dgamma_acc;
  switch (bn_bwd_reduce_mode(act, x != nullptr, y != nullptr, mask != nullptr)) {
    case kColBwdXY: return launch_col_reduce<kColBwdXY>(a, lean, stream);   // sign from the mask bytes (layers with a residual: 1/16 of y's bytes) or from y
    case kColBwdX: return launch_col_reduce<kColBwdX>(a, lean, stream);     // layers without a residual
    default: return launch_col_reduce<kColBwdY>(a, lean, stream);           // one activation tensor less to read
  }
}

extern "C" int xas_bn_bwd_apply(const float* x, const float* y, const float* dy, const float* mean,
                                const float* var_biased, const float* gamma, const float* beta, const float* sums,
                                float eps, int act, long M, int C, int groups, double count, float* dx,
                                float* dresidual, const uint8_t* mask, void* stream) {
  return xas_bn_bwd_apply_amax(x, y, dy, mean, var_biased, gamma, beta, sums, eps, act, M, C, groups, count, dx, dresidual, mask,
                               nullptr, stream);
}

extern "C" int xas_bn_bwd_apply_amax(const float* x, const float* y, const float* dy, const float* mean,
                                     const float* var_biased, const float* gamma, const float* beta, const float* sums,
                                     float eps, int act, long M, int C, int groups, double count, float* dx,
                                     float* dresidual, const uint8_t* mask, float* amax_out, void* stream) {
  XAS_REQUIRE(!mask || x, "bn_bwd_apply: the sign-mask form needs x");
  XAS_REQUIRE(dy && mean && var_biased && gamma && sums && dx && (act == 0 || y || mask || (x && beta)),
              "bn_bwd_apply: null buffer (an activation needs y, or x with beta)");
  XAS_REQUIRE(y || mask || !dresidual || act == 0, "bn_bwd_apply: the y-free form is for layers without a residual");
  XAS_REQUIRE(x || (act == 2 && y && beta),
              "bn_bwd_apply: without x the layer needs an INVERTIBLE activation (leaky ReLU), y and beta: dx needs xhat "
              "of every element, also where ReLU clipped the output");
  XAS_REQUIRE(M > 0 && C >= 4 && C % 4 == 0 && count > 0 && groups >= 1 && M % groups == 0, "bn_bwd_apply: bad shape");
  const int C4 = C / 4;
  const long n4g = (M / groups) * C4;
  const unsigned gs = bn_stream_grid(n4g, C4, groups, tune_flags());
  BnBwdKernel k = gs ? bn_bwd_stream_kernel(act, x != nullptr, y != nullptr, mask != nullptr, dresidual != nullptr) : nullptr;
  const unsigned gx = k ? gs : ew_grid_g(n4g, groups);
  if (!k) k = bn_bwd_apply_kernel<false>;
  hipLaunchKernelGGL(k, dim3(gx, groups), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(y),
                     reinterpret_cast<const float4*>(dy), mean, var_biased, gamma, beta, sums, eps, act, n4g,
                     C4, (float)(1.0 / count), reinterpret_cast<float4*>(dx), reinterpret_cast<float4*>(dresidual), mask, amax_out);
  XAS_LAUNCH_CHECK();
  return 0;
}

// ---- dual forms (xas_hip.h): bn3 and the projection norm of a block output in one pass each ---------------------------
static int bn_dual_shape(const char* who, long M, int C, int groups) {
  XAS_REQUIRE(M > 0 && C >= 4 && C % 4 == 0 && groups >= 1 && M % groups == 0, "%s: bad shape M=%ld C=%d groups=%d", who, M, C, groups);
  return 0;
}

extern "C" int xas_bn_apply_dual_amax(const float* x, const float* mean, const float* var_biased, const float* gamma,
                                      const float* beta, float eps, const float* xd, const float* mean_d,
                                      const float* var_biased_d, const float* gamma_d, const float* beta_d, float eps_d,
                                      long M, int C, int groups, float* y, uint8_t* mask_out, float* amax_out, void* stream) {
  XAS_REQUIRE(x && mean && var_biased && gamma && beta && xd && mean_d && var_biased_d && gamma_d && beta_d && y && mask_out,
              "bn_apply_dual: null buffer");
  if (bn_dual_shape("bn_apply_dual", M, C, groups)) return 1;
  const int C4 = C / 4;
  const long n4g = (M / groups) * C4;
  const unsigned gs = bn_stream_grid(n4g, C4, groups, tune_flags());
  const BnNorm n3{mean, var_biased, gamma, beta, nullptr, eps}, nd{mean_d, var_biased_d, gamma_d, beta_d, nullptr, eps_d};
  hipLaunchKernelGGL(gs ? bn_apply_dual_kernel<true> : bn_apply_dual_kernel<false>, dim3(gs ? gs : ew_grid_g(n4g, groups), groups),
                     dim3(256), 0, as_stream(stream), reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(xd), n3,
                     nd, n4g, C4, reinterpret_cast<float4*>(y), mask_out, amax_out);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_bn_bwd_reduce_dual(const float* x, const float* xd, const float* dy, const uint8_t* mask, const float* mean,
                                      const float* var_biased, float eps, const float* mean_d, const float* var_biased_d,
                                      float eps_d, long M, int C, int groups, float* sums, float* sums_d, float* workspace,
                                      float* dbeta_acc, float* dgamma_acc, float* dbeta_d_acc, float* dgamma_d_acc,
                                      void* stream) {
  ColGeom g;
  if (col_geom(M, C, groups, &g)) return 1;
  XAS_REQUIRE(x && xd && dy && mask && mean && var_biased && mean_d && var_biased_d && sums && sums_d && workspace,
              "bn_bwd_reduce_dual: null buffer");
  XAS_REQUIRE((dbeta_acc == nullptr) == (dgamma_acc == nullptr) && (dbeta_d_acc == nullptr) == (dgamma_d_acc == nullptr),
              "bn_bwd_reduce_dual: gradient accumulators come in pairs");
  const bool lean = (tune_flags() & XAS_TUNE_COL_REDUCE_LEAN) != 0;
  const size_t per_norm = (size_t)g.G * g.nslab * 2 * C + C;               // xas_bn_workspace_floats(M, C, groups)
  ColArgs a{};
  a.M = M; a.C = C; a.g = g; a.partial = workspace;
  a.ticket = take_tickets(2 * g.ncb);                                      // ncb words per norm
  XAS_REQUIRE(a.ticket != nullptr, "column reduce: could not allocate the ticket counters");
  XAS_REQUIRE((size_t)g.G * g.nslab * 2 * C * sizeof(float) < 0x7fffff00ul, "column reduce: partial buffer too large");
  a.x = x; a.dy = dy; a.mask = mask; a.mean = mean; a.var = var_biased; a.eps = eps; a.act = 1;
  a.out1 = sums; a.out2 = sums + C; a.out_stride = 2 * (long)C;            // [G][2][C]
  a.acc1 = dbeta_acc; a.acc2 = dgamma_acc;
  a.second = {xd, mean_d, var_biased_d, eps_d, workspace + per_norm, a.ticket + g.ncb, sums_d, sums_d + C, dbeta_d_acc, dgamma_d_acc};
  return launch_col_reduce<kColBwdDual>(a, lean, stream);
}

extern "C" int xas_bn_bwd_apply_dual_amax(const float* x, const float* xd, const float* dy, const uint8_t* mask,
                                          const float* mean, const float* var_biased, const float* gamma, const float* sums,
                                          float eps, const float* mean_d, const float* var_biased_d, const float* gamma_d,
                                          const float* sums_d, float eps_d, long M, int C, int groups, double count,
                                          double count_d, float* dx, float* dxd, float* amax_out, float* amax_d_out,
                                          void* stream) {
  XAS_REQUIRE(x && xd && dy && mask && mean && var_biased && gamma && sums && mean_d && var_biased_d && gamma_d && sums_d && dx && dxd,
              "bn_bwd_apply_dual: null buffer");
  if (bn_dual_shape("bn_bwd_apply_dual", M, C, groups)) return 1;
  XAS_REQUIRE(count > 0 && count_d > 0, "bn_bwd_apply_dual: bad count");
  const int C4 = C / 4;
  const long n4g = (M / groups) * C4;
  const unsigned gs = bn_stream_grid(n4g, C4, groups, tune_flags());
  const BnNorm n3{mean, var_biased, gamma, nullptr, sums, eps}, nd{mean_d, var_biased_d, gamma_d, nullptr, sums_d, eps_d};
  hipLaunchKernelGGL(gs ? bn_bwd_apply_dual_kernel<true> : bn_bwd_apply_dual_kernel<false>,
                     dim3(gs ? gs : ew_grid_g(n4g, groups), groups), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(xd), reinterpret_cast<const float4*>(dy),
                     mask, n3, nd, n4g, C4, (float)(1.0 / count), (float)(1.0 / count_d), reinterpret_cast<float4*>(dx),
                     reinterpret_cast<float4*>(dxd),
                     amax_out, amax_d_out);
  XAS_LAUNCH_CHECK();
  return 0;
}

// max |x| over a tensor -> *amax_out (merged with atomicMax: the caller zeroes it once).  For conv inputs that no kernel of
// this library wrote (images, rendered masks, tensors handed in from outside): one streaming read, HBM bound.
__global__ __launch_bounds__(256) void abs_max_kernel(const float* __restrict__ x, long n, float* __restrict__ amax_out) {
  float amx = 0.f;
  const long n4 = n / 4, stride = (long)gridDim.x * blockDim.x;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = stream_load(x4 + i + u * stride);
#pragma unroll
    for (int u = 0; u < 4; ++u) amx = amax4(amx, v[u]);
  }
  for (; i < n4; i += stride) amx = amax4(amx, x4[i]);
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) amx = fmaxf(amx, fabsf(x[n4 * 4 + threadIdx.x]));
  publish_amax(amax_out, amx);
}

extern "C" int xas_abs_max(const float* x, long n, float* amax_out, void* stream) {
  XAS_REQUIRE(x && amax_out && n > 0 && (((uintptr_t)x) & 15) == 0, "abs_max: need a 16-byte aligned tensor and an output float");
  hipLaunchKernelGGL(abs_max_kernel, dim3(ew_grid(cdiv(n, 4))), dim3(256), 0, as_stream(stream), x, n, amax_out);
  XAS_LAUNCH_CHECK();
  return 0;
}
