// Small fused kernels: mask losses, GCN-discriminator building blocks, SMPL skinning,
// multi-tensor Adam and its gradient guard.  gfx950.
#include <float.h>

#include "common.h"

namespace xas {

// ------------------------------------------------------------------ mask losses
// modules/base_losses/loss_func.py:4-16.  mode bit0 = clip (m > 0.1), bit1 = weighted.
constexpr int kLossThreads = 256;
constexpr int kLossPerThread = 16;

__global__ void mask_loss_partial_kernel(const float* __restrict__ m, const float* __restrict__ gt,
                                         const float* __restrict__ w, long n, int mode, float* __restrict__ partial) {
  __shared__ float sm[20];
  float a = 0.f, b = 0.f;
  const long base = (long)blockIdx.x * kLossThreads * kLossPerThread;
  for (int k = 0; k < kLossPerThread; ++k) {
    const long i = base + (long)k * kLossThreads + threadIdx.x;
    if (i < n) {
      const float mv = m[i], d = mv - gt[i];
      const float clip = ((mode & 1) && !(mv > 0.1f)) ? 0.f : 1.f;
      if (mode & 2) a += d * d * clip * w[i];
      else { a += d * d; b += clip; }
    }
  }
  a = block_sum(a, sm);
  b = block_sum(b, sm);
  if (threadIdx.x == 0) { partial[blockIdx.x * 2] = a; partial[blockIdx.x * 2 + 1] = b; }
}

__global__ void mask_loss_finalize_kernel(const float* __restrict__ partial, int nblk, long n, int mode,
                                          float* __restrict__ out) {
  __shared__ float sm[20];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < nblk; i += blockDim.x) { a += partial[i * 2]; b += partial[i * 2 + 1]; }
  a = block_sum(a, sm);
  b = block_sum(b, sm);
  if (threadIdx.x == 0) {
    out[0] = a / (float)n;
    out[1] = (mode & 2) ? 1.f : b / (float)n;
    out[2] = out[0] * out[1];
  }
}

__global__ void mask_loss_bwd_kernel(const float* __restrict__ m, const float* __restrict__ gt,
                                     const float* __restrict__ w, long n, int mode, const float* __restrict__ out,
                                     const float* __restrict__ gscalar, float* __restrict__ dm) {
  const float g = gscalar[0] * 2.f / (float)n;
  const float clipmean = out[1];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float mv = m[i], d = mv - gt[i];
    if (mode & 2) {
      const float clip = ((mode & 1) && !(mv > 0.1f)) ? 0.f : 1.f;
      dm[i] = g * d * clip * w[i];
    } else {
      dm[i] = g * d * clipmean;
    }
  }
}


// ------------------------------------------------------------------ joint-level losses
// modules/base_losses/loss_func.py:18-76 as the model combines them (modules/model.py:98-164): every loss is a
// batch mean per hypothesis followed by a MIN over the hypothesis axis (symmetry, pseudo supervision) or a
// per-sample min (LSGAN).  One workgroup per launch: B*K*3 values.
//
// pose_loss: kind 0 = supervision  : v_h = mean_{b,k,c} (pred[b,h,k,c] - gt[b,k,c])^2
//            kind 1 = symmetry 3-D : v_h = w0 * bone_sym(p_h) + w1 * kp_sym(p_h)      (p in mm, scaled 1e-3)
//            kind 2 = kp_sym 2-D   : v_h = w0 * mean((mid - anchor)^2) over (x, y) only (no 1e-3 scale)
// out[0] = min_h v_h, out[1] = argmin (as float), out[2..2+Hy) = v_h.
// Choice of the hypothesis: the first NaN if any v_h is NaN (so out[0] is NaN, as torch.min gives), else the first
// minimum, and the backward sends the whole gradient there.  The reference takes torch.min over the stacked values, a
// full reduction whose backward SPLITS the gradient evenly among exactly tied minima (min(dim=...) would give it to one
// index); on an exact tie between hypotheses this kernel therefore differs from the reference: all of it to the first.
constexpr int kPoseThreads = 256;
__constant__ int kLimbFar[8] = {16, 15, 13, 12, 3, 2, 6, 5};
__constant__ int kLimbNear[8] = {15, 14, 12, 11, 2, 1, 5, 4};

__device__ __forceinline__ float limb_len(const float* p, int l) {
  const float dx = p[kLimbFar[l] * 3] - p[kLimbNear[l] * 3], dy = p[kLimbFar[l] * 3 + 1] - p[kLimbNear[l] * 3 + 1],
              dz = p[kLimbFar[l] * 3 + 2] - p[kLimbNear[l] * 3 + 2];
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

__global__ void pose_loss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int B, int Hy, int K,
                                     int kind, float w0, float w1, float w2, float* __restrict__ out) {
  __shared__ float sm[20];
  __shared__ float vh[8];
  for (int h = 0; h < Hy; ++h) {
    float acc = 0.f;
    if (kind == 0) {
      const int n = B * K * 3;
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int b = i / (K * 3), r = i % (K * 3);
        const float d = pred[((size_t)b * Hy + h) * K * 3 + r] - gt[(size_t)b * K * 3 + r];
        acc = fmaf(d, d, acc);
      }
      acc = block_sum(acc, sm) / (float)n;
    } else if (kind == 1) {
      float a_bone = 0.f, a_kp = 0.f;
      for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* p = pred + ((size_t)b * Hy + h) * K * 3;
        for (int l = 0; l < 8; l += 2) {
          const float d = limb_len(p, l) * 1e-3f - limb_len(p, l + 1) * 1e-3f;
          a_bone = fmaf(d, d, a_bone);
        }
        // mid-points of (11,14) vs joint K-1 and of (1,4) vs joint 0
        for (int c = 0; c < 3; ++c) {
          const float m0 = (p[11 * 3 + c] + p[14 * 3 + c]) / 2 * 1e-3f - p[(K - 1) * 3 + c] * 1e-3f;
          const float m1 = (p[1 * 3 + c] + p[4 * 3 + c]) / 2 * 1e-3f - p[0 * 3 + c] * 1e-3f;
          a_kp = fmaf(m0, m0, a_kp); a_kp = fmaf(m1, m1, a_kp);
        }
      }
      a_bone = block_sum(a_bone, sm) / (float)(B * 4);
      a_kp = block_sum(a_kp, sm) / (float)(B * 6);
      acc = w0 * a_bone + w1 * a_kp;
      if (gt) {                      // optional 2-D term on the patch joints `gt` = kps [B][Hy][K][3] (model.py:110-111)
        float a2 = 0.f;
        for (int b = threadIdx.x; b < B; b += blockDim.x) {
          const float* p = gt + ((size_t)b * Hy + h) * K * 3;
          for (int c = 0; c < 2; ++c) {
            const float m0 = (p[11 * 3 + c] + p[14 * 3 + c]) / 2 - p[(K - 1) * 3 + c];
            const float m1 = (p[1 * 3 + c] + p[4 * 3 + c]) / 2 - p[0 * 3 + c];
            a2 = fmaf(m0, m0, a2); a2 = fmaf(m1, m1, a2);
          }
        }
        acc += w2 * block_sum(a2, sm) / (float)(B * 4);
      }
    } else {
      for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* p = pred + ((size_t)b * Hy + h) * K * 3;
        for (int c = 0; c < 2; ++c) {
          const float m0 = (p[11 * 3 + c] + p[14 * 3 + c]) / 2 - p[(K - 1) * 3 + c];
          const float m1 = (p[1 * 3 + c] + p[4 * 3 + c]) / 2 - p[0 * 3 + c];
          acc = fmaf(m0, m0, acc); acc = fmaf(m1, m1, acc);
        }
      }
      acc = w0 * block_sum(acc, sm) / (float)(B * 4);
    }
    if (threadIdx.x == 0) vh[h] = acc;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int best = 0;
    for (int h = 1; h < Hy; ++h)
      if (vh[best] == vh[best] && (vh[h] < vh[best] || vh[h] != vh[h])) best = h;      // a NaN wins and stays
    out[0] = vh[best]; out[1] = (float)best;
    for (int h = 0; h < Hy; ++h) out[2 + h] = vh[h];
  }
}

// gradient of out[0] w.r.t. pred (only hypothesis argmin receives gradient); g = upstream scalar gradient
__global__ void pose_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int B, int Hy, int K,
                                     int kind, float w0, float w1, float w2, const float* __restrict__ out,
                                     const float* __restrict__ gscalar, float* __restrict__ gpred,
                                     float* __restrict__ gaux) {
  const int best = (int)out[1];
  const float g = gscalar[0];
  const int n = B * Hy * K * 3;
  for (int i = threadIdx.x; i < n; i += blockDim.x) { gpred[i] = 0.f; if (gaux) gaux[i] = 0.f; }
  __syncthreads();
  if (kind == 0) {
    const float s = g * 2.f / (float)(B * K * 3);
    for (int i = threadIdx.x; i < B * K * 3; i += blockDim.x) {
      const int b = i / (K * 3), r = i % (K * 3);
      const size_t o = ((size_t)b * Hy + best) * K * 3 + r;
      gpred[o] = s * (pred[o] - gt[(size_t)b * K * 3 + r]);
    }
    return;
  }
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const float* p = pred + ((size_t)b * Hy + best) * K * 3;
    float* q = gpred + ((size_t)b * Hy + best) * K * 3;
    if (kind == 1) {
      const float sb = g * w0 * 2.f / (float)(B * 4), sk = g * w1 * 2.f / (float)(B * 6);
      for (int l = 0; l < 8; l += 2) {
        const float la = limb_len(p, l), lb = limb_len(p, l + 1);
        const float d = (la - lb) * 1e-3f;
        // d/dp of |p_far - p_near| = unit vector; scaled by 1e-3
        for (int side = 0; side < 2; ++side) {
          const int ll = l + side;
          const float len = side == 0 ? la : lb, sgn = side == 0 ? 1.f : -1.f;
          if (len > 0.f)
            for (int c = 0; c < 3; ++c) {
              const float u = (p[kLimbFar[ll] * 3 + c] - p[kLimbNear[ll] * 3 + c]) / len;
              const float gg = sb * d * sgn * 1e-3f * u;
              q[kLimbFar[ll] * 3 + c] += gg;
              q[kLimbNear[ll] * 3 + c] -= gg;
            }
        }
      }
      for (int c = 0; c < 3; ++c) {
        const float m0 = ((p[11 * 3 + c] + p[14 * 3 + c]) / 2 - p[(K - 1) * 3 + c]) * 1e-3f;
        const float m1 = ((p[1 * 3 + c] + p[4 * 3 + c]) / 2 - p[0 * 3 + c]) * 1e-3f;
        const float g0 = sk * m0 * 1e-3f, g1 = sk * m1 * 1e-3f;
        q[11 * 3 + c] += 0.5f * g0; q[14 * 3 + c] += 0.5f * g0; q[(K - 1) * 3 + c] -= g0;
        q[1 * 3 + c] += 0.5f * g1; q[4 * 3 + c] += 0.5f * g1; q[0 * 3 + c] -= g1;
      }
      if (gt && gaux) {
        const float* p2 = gt + ((size_t)b * Hy + best) * K * 3;
        float* q2 = gaux + ((size_t)b * Hy + best) * K * 3;
        const float s2 = g * w2 * 2.f / (float)(B * 4);
        for (int c = 0; c < 2; ++c) {
          const float m0 = (p2[11 * 3 + c] + p2[14 * 3 + c]) / 2 - p2[(K - 1) * 3 + c];
          const float m1 = (p2[1 * 3 + c] + p2[4 * 3 + c]) / 2 - p2[0 * 3 + c];
          q2[11 * 3 + c] += 0.5f * s2 * m0; q2[14 * 3 + c] += 0.5f * s2 * m0; q2[(K - 1) * 3 + c] -= s2 * m0;
          q2[1 * 3 + c] += 0.5f * s2 * m1; q2[4 * 3 + c] += 0.5f * s2 * m1; q2[0 * 3 + c] -= s2 * m1;
        }
      }
    } else {
      const float sk = g * w0 * 2.f / (float)(B * 4);
      for (int c = 0; c < 2; ++c) {
        const float m0 = (p[11 * 3 + c] + p[14 * 3 + c]) / 2 - p[(K - 1) * 3 + c];
        const float m1 = (p[1 * 3 + c] + p[4 * 3 + c]) / 2 - p[0 * 3 + c];
        q[11 * 3 + c] += 0.5f * sk * m0; q[14 * 3 + c] += 0.5f * sk * m0; q[(K - 1) * 3 + c] -= sk * m0;
        q[1 * 3 + c] += 0.5f * sk * m1; q[4 * 3 + c] += 0.5f * sk * m1; q[0 * 3 + c] -= sk * m1;
      }
    }
  }
}

// LSGAN term (loss_func.py:54-76): logits [B][Hy] (Hy = 1 for the 2-D case); out[0] = mean_b min_h (x - t)^2 ;
// argmin per sample is written to idx[b] for the backward.
__global__ void lsgan_fwd_kernel(const float* __restrict__ logits, int B, int Hy, float target, float* __restrict__ out,
                                 int* __restrict__ idx) {
  __shared__ float sm[20];
  float acc = 0.f;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    float best = INFINITY; int bi = 0;
    for (int h = 0; h < Hy; ++h) {
      const float d = logits[b * Hy + h] - target, e = d * d;
      if (e < best || (e != e && best == best)) { best = e; bi = h; }      // a NaN wins and stays, as min(dim=1) gives
    }
    idx[b] = bi;
    acc += best;
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) out[0] = acc / (float)B;
}

__global__ void lsgan_bwd_kernel(const float* __restrict__ logits, int B, int Hy, float target,
                                 const int* __restrict__ idx, const float* __restrict__ gscalar,
                                 float* __restrict__ glogits) {
  const float s = gscalar[0] * 2.f / (float)B;
  for (int i = threadIdx.x; i < B * Hy; i += blockDim.x) {
    const int b = i / Hy, h = i % Hy;
    glogits[i] = (h == idx[b]) ? s * (logits[i] - target) : 0.f;
  }
}

// ------------------------------------------------------------------ graph aggregate
__global__ void graph_aggregate_kernel(const float* __restrict__ x, const float* __restrict__ adj, int B, int N, int C,
                                       float* __restrict__ y) {
  const long total = (long)B * N * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = i % C; const long t = i / C; const int node = t % N; const long b = t / N;
    const float* xb = x + b * N * C + c;
    const float* ar = adj + node * N;
    float acc = 0.f;
    for (int j = 0; j < N; ++j) { const float a = ar[j]; if (a != 0.f) acc = fmaf(a, xb[(size_t)j * C], acc); }
    y[i] = acc;
  }
}

// ------------------------------------------------------------------ graph LayerNorm (+relu, +residual)
// PyG norm.LayerNorm(mode='graph', batch=None): (x - mean_all) / (std_all + eps) * gamma + beta, where
// "all" = the whole [rows, C] tensor of ONE discriminator call.  G independent calls are batched as G
// groups of `rows` rows each (x is [G*rows, C]); statistics stay per group.
constexpr int kGlnThreads = 256;

// how many of a group's n elements block i of nblk visits in its grid-stride loop (>= 1: nblk <= ceil(n / 2048))
__device__ __forceinline__ long gln_block_count(long n, int nblk, int i) {
  const long period = (long)nblk * kGlnThreads, r = n % period - (long)i * kGlnThreads;
  return n / period * kGlnThreads + (r < 0 ? 0 : (r > kGlnThreads ? kGlnThreads : r));
}

// Per block: a = sum (x - pivot) with pivot = the group's first element, then b = sum ((x - pivot) - a / count)^2, the
// squares about the block's OWN mean.  A sum of squares about a point d standard deviations off the mean carries terms
// (d sigma)^2 next to the variance and loses (1 + d^2) of its precision when they are subtracted again; about the block
// mean there is nothing to subtract.  gln_stats_kernel recomputes a / count with the same float division.
__global__ void gln_partial_kernel(const float* __restrict__ x, long n, float* __restrict__ partial) {
  __shared__ float sm[20];
  const float* xg = x + (size_t)blockIdx.y * n;
  const float pivot = xg[0];
  float a = 0.f, b = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) a += xg[i] - pivot;
  a = block_sum(a, sm);
  const float mu = a / (float)gln_block_count(n, gridDim.x, blockIdx.x);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float d = (xg[i] - pivot) - mu;
    b = fmaf(d, d, b);
  }
  b = block_sum(b, sm);
  if (threadIdx.x == 0) {
    float* o = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    o[0] = a; o[1] = b;
  }
}

__global__ void gln_stats_kernel(const float* __restrict__ partial, int nblk, const float* __restrict__ x, long n,
                                 int G, float* __restrict__ stats) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const float* pg = partial + (size_t)g * nblk * 2;
  double a = 0.0, b = 0.0;
  for (int i = 0; i < nblk; ++i) a += pg[i * 2];
  const double m = a / (double)n;
  // sum (d - m)^2 over block i = b_i + 2 (mu_i - m) sum (d - mu_i) + count_i (mu_i - m)^2, with sum (d - mu_i) = a_i - count_i mu_i
  for (int i = 0; i < nblk; ++i) {
    const long cnt = gln_block_count(n, nblk, i);
    const double mu = (double)(pg[i * 2] / (float)cnt), off = mu - m;
    b += (double)pg[i * 2 + 1] + 2.0 * off * ((double)pg[i * 2] - (double)cnt * mu) + (double)cnt * off * off;
  }
  double v = b / (double)n;
  if (v < 0.0) v = 0.0;
  stats[g * 2] = (float)((double)x[(size_t)g * n] + m);
  stats[g * 2 + 1] = (float)sqrt(v);
}

__global__ void gln_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                 const float* __restrict__ beta, const float* __restrict__ res,
                                 const float* __restrict__ stats, long n, int G, int C, float eps, float* __restrict__ y) {
  const long total = n * G;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int g = (int)(i / n);
    const float mean = stats[g * 2], inv = 1.f / (stats[g * 2 + 1] + eps);
    const int c = i % C;
    float v = (x[i] - mean) * inv * gamma[c] + beta[c];
    v = fmaxf(v, 0.f);
    if (res) v += res[i];
    y[i] = v;
  }
}

// per group, per channel: sums of g and g*xhat where g = dy * relu'(ln(x)); block = 64 channels x 16 row lanes
__global__ __launch_bounds__(1024) void gln_bwd_cols_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const float* __restrict__ stats, long rows, int C,
                                                            float eps, float* __restrict__ gsum /* [G][2][C] */) {
  __shared__ float s1[16][64], s2[16][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx, g = blockIdx.y;
  const float mean = stats[g * 2], inv = 1.f / (stats[g * 2 + 1] + eps);
  const size_t base = (size_t)g * rows * C;
  float a = 0.f, b = 0.f;
  if (c < C) {
    const float gmm = gamma[c], bt = beta[c];
    for (long r = ry; r < rows; r += 16) {
      const float xh = (x[base + r * C + c] - mean) * inv;
      const float gg = (xh * gmm + bt > 0.f) ? dy[base + r * C + c] : 0.f;
      a += gg; b = fmaf(gg, xh, b);
    }
  }
  s1[ry][cx] = a; s2[ry][cx] = b;
  __syncthreads();
  if (ry == 0 && c < C) {
    float u = 0.f, v = 0.f;
    for (int k = 0; k < 16; ++k) { u += s1[k][cx]; v += s2[k][cx]; }
    gsum[((size_t)g * 2) * C + c] = u;          // d beta contribution
    gsum[((size_t)g * 2 + 1) * C + c] = v;      // d gamma contribution
  }
}

// per group: A = sum_c gamma*dbeta_g, B = sum_c gamma*dgamma_g ; block 0 also reduces dgamma/dbeta over groups
__global__ void gln_bwd_scalar_kernel(const float* __restrict__ gamma, const float* __restrict__ gsum, int G, int C,
                                      float* __restrict__ ab, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float sm[20];
  const int g = blockIdx.x;
  if (g < G) {
    float a = 0.f, b = 0.f;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      a = fmaf(gamma[c], gsum[((size_t)g * 2) * C + c], a);
      b = fmaf(gamma[c], gsum[((size_t)g * 2 + 1) * C + c], b);
    }
    a = block_sum(a, sm);
    b = block_sum(b, sm);
    if (threadIdx.x == 0) { ab[g * 2] = a; ab[g * 2 + 1] = b; }
  } else {                       // extra block: parameter gradients = sum over groups
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float u = 0.f, v = 0.f;
      for (int k = 0; k < G; ++k) { u += gsum[((size_t)k * 2) * C + c]; v += gsum[((size_t)k * 2 + 1) * C + c]; }
      dbeta[c] = u; dgamma[c] = v;
    }
  }
}

__global__ void gln_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                     const float* __restrict__ stats, const float* __restrict__ ab, long n, int G, int C,
                                     float eps, float* __restrict__ dx) {
  const long total = n * G;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int g = (int)(i / n);
    const float mean = stats[g * 2], sigma = stats[g * 2 + 1], inv = 1.f / (sigma + eps);
    const float A = ab[g * 2] / (float)n;
    const float Bc = sigma > 0.f ? ab[g * 2 + 1] / ((float)n * sigma) : 0.f;
    const int c = i % C;
    const float xh = (x[i] - mean) * inv;
    const float gg = (xh * gamma[c] + beta[c] > 0.f) ? dy[i] * gamma[c] : 0.f;
    dx[i] = (gg - A) * inv - xh * Bc;
  }
}

// ------------------------------------------------------------------ SMPL LBS forward
__global__ void smpl_joints_kernel(const float* __restrict__ betas, const float* __restrict__ vt,
                                   const float* __restrict__ sd, const float* __restrict__ jr, int V,
                                   float* __restrict__ ws, int per /* floats per sample record */) {
  __shared__ float sm[20];
  const int b = blockIdx.x, j = blockIdx.y;
  float bt[10];
  for (int k = 0; k < 10; ++k) bt[k] = betas[b * 10 + k];
  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int v = threadIdx.x; v < V; v += blockDim.x) {
    const float w = jr[(size_t)j * V + v];
    if (w == 0.f) continue;
    float p[3];
    for (int c = 0; c < 3; ++c) {
      float s = vt[v * 3 + c];
      const float* d = sd + ((size_t)v * 3 + c) * 10;
      for (int k = 0; k < 10; ++k) s = fmaf(d[k], bt[k], s);
      p[c] = s;
    }
    ax = fmaf(w, p[0], ax); ay = fmaf(w, p[1], ay); az = fmaf(w, p[2], az);
  }
  ax = block_sum(ax, sm); ay = block_sum(ay, sm); az = block_sum(az, sm);
  if (threadIdx.x == 0) { float* o = ws + (size_t)b * per + j * 3; o[0] = ax; o[1] = ay; o[2] = az; }
}

// one block (64 threads) per sample: Rodrigues, kinematic chain, pose map.
// ws layout per sample: j0[72] | G2[24*16] | pose_map[207]
__global__ void smpl_chain_kernel(const float* __restrict__ pose, const int* __restrict__ parents, int center_idx,
                                  float* __restrict__ ws, float* __restrict__ joints_out) {
  __shared__ float R[24][9];
  __shared__ float G[24][16];
  const int b = blockIdx.x, t = threadIdx.x;
  float* wsb = ws + (size_t)b * (72 + 24 * 16 + 207);
  const float* j0 = wsb;
  if (t < 24) {
    const float ax = pose[b * 72 + t * 3], ay = pose[b * 72 + t * 3 + 1], az = pose[b * 72 + t * 3 + 2];
    const float ex = ax + 1e-8f, ey = ay + 1e-8f, ez = az + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float nx = ax / angle, ny = ay / angle, nz = az / angle;
    const float half = angle * 0.5f, sn = sinf(half);
    float w = cosf(half), x = sn * nx, y = sn * ny, z = sn * nz;
    const float qn = sqrtf(w * w + x * x + y * y + z * z);
    w /= qn; x /= qn; y /= qn; z /= qn;
    float* r = R[t];
    r[0] = w * w + x * x - y * y - z * z; r[1] = 2 * x * y - 2 * w * z; r[2] = 2 * w * y + 2 * x * z;
    r[3] = 2 * w * z + 2 * x * y; r[4] = w * w - x * x + y * y - z * z; r[5] = 2 * y * z - 2 * w * x;
    r[6] = 2 * x * z - 2 * w * y; r[7] = 2 * w * x + 2 * y * z; r[8] = w * w - x * x - y * y + z * z;
    if (t >= 1) {
      float* pm = wsb + 72 + 24 * 16 + (t - 1) * 9;
      for (int e = 0; e < 9; ++e) pm[e] = r[e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
    }
  }
  __syncthreads();
  if (t == 0) {
    for (int i = 0; i < 24; ++i) {
      float L[16];
      const int par = i == 0 ? -1 : parents[i];
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) L[r * 4 + c] = R[i][r * 3 + c];
        L[r * 4 + 3] = j0[i * 3 + r] - (par >= 0 ? j0[par * 3 + r] : 0.f);
      }
      L[12] = L[13] = L[14] = 0.f; L[15] = 1.f;
      if (par < 0) { for (int e = 0; e < 16; ++e) G[i][e] = L[e]; }
      else {
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            float s = 0.f;
            for (int k = 0; k < 4; ++k) s = fmaf(G[par][r * 4 + k], L[k * 4 + c], s);
            G[i][r * 4 + c] = s;
          }
      }
    }
  }
  __syncthreads();
  if (t < 24) {
    float* g2 = wsb + 72 + t * 16;
    for (int r = 0; r < 4; ++r) {
      const float corr = G[t][r * 4] * j0[t * 3] + G[t][r * 4 + 1] * j0[t * 3 + 1] + G[t][r * 4 + 2] * j0[t * 3 + 2];
      for (int c = 0; c < 3; ++c) g2[r * 4 + c] = G[t][r * 4 + c];
      g2[r * 4 + 3] = G[t][r * 4 + 3] - corr;
    }
    float* o = joints_out + ((size_t)b * 24 + t) * 3;
    for (int r = 0; r < 3; ++r) o[r] = G[t][r * 4 + 3] - (center_idx >= 0 ? G[center_idx][r * 4 + 3] : 0.f);
  }
}

__global__ void smpl_verts_kernel(const float* __restrict__ betas, const float* __restrict__ vt,
                                  const float* __restrict__ sd, const float* __restrict__ pd,
                                  const float* __restrict__ wts, const float* __restrict__ ws, int V, int center_idx,
                                  float* __restrict__ verts) {
  __shared__ float g2[24 * 16];
  __shared__ float pm[207];
  __shared__ float bt[10];
  __shared__ float cen[3];
  const int b = blockIdx.y;
  const float* wsb = ws + (size_t)b * (72 + 24 * 16 + 207);
  for (int i = threadIdx.x; i < 24 * 16; i += blockDim.x) g2[i] = wsb[72 + i];
  for (int i = threadIdx.x; i < 207; i += blockDim.x) pm[i] = wsb[72 + 24 * 16 + i];
  if (threadIdx.x < 10) bt[threadIdx.x] = betas[b * 10 + threadIdx.x];
  __syncthreads();
  if (threadIdx.x < 3) {
    // joint translation of the centre joint: G[c][r][3] = G2[c][r][3] + (G[c][r][:3] . j0[c])
    float v = 0.f;
    if (center_idx >= 0) {
      const int r = threadIdx.x;
      const float* g = g2 + center_idx * 16 + r * 4;
      const float* j = wsb + center_idx * 3;
      v = g[3] + g[0] * j[0] + g[1] * j[1] + g[2] * j[2];
    }
    cen[threadIdx.x] = v;
  }
  __syncthreads();
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  float p[3];
  for (int c = 0; c < 3; ++c) {
    float s = vt[v * 3 + c];
    const float* d = sd + ((size_t)v * 3 + c) * 10;
    for (int k = 0; k < 10; ++k) s = fmaf(d[k], bt[k], s);
    const float* q = pd + ((size_t)v * 3 + c) * 207;
    for (int k = 0; k < 207; ++k) s = fmaf(q[k], pm[k], s);
    p[c] = s;
  }
  float T[12];
  for (int e = 0; e < 12; ++e) T[e] = 0.f;
  for (int j = 0; j < 24; ++j) {
    const float w = wts[(size_t)v * 24 + j];
    if (w == 0.f) continue;
    for (int e = 0; e < 12; ++e) T[e] = fmaf(w, g2[j * 16 + e], T[e]);
  }
  float* o = verts + ((size_t)b * V + v) * 3;
  for (int r = 0; r < 3; ++r) o[r] = T[r * 4] * p[0] + T[r * 4 + 1] * p[1] + T[r * 4 + 2] * p[2] + T[r * 4 + 3] - cen[r];
}

// ------------------------------------------------------------------ SMPL LBS backward
// d(verts), d(joints) -> d(pose), d(betas).  Three launches:
//   1. vertex pass (same tiling as the forward): recompute v_posed and the blended transform T of each vertex,
//      dv_posed = T_R^T dV, and reduce over the block's 128 vertices
//        dG'[j] += w[v][j] * [dV (x) v_posed | dV],  dpose_map += PD[v]^T dv_posed,  dbeta += SD[v]^T dv_posed,  sum dV
//      into per-block partial records (no atomics: the second pass sums them in block order);
//   2. per sample: sum the partials, walk the kinematic chain backwards (children before parents), Rodrigues backward;
//   3. per sample: the joint-regressor term of d(betas).
constexpr int kSmplP = 24 * 12 + 207 + 10 + 3;   // dG' | dpose_map | dbeta (vertex term) | sum dV

__global__ __launch_bounds__(128) void smpl_bwd_verts_kernel(const float* __restrict__ betas, const float* __restrict__ vt,
                                                             const float* __restrict__ sd, const float* __restrict__ pd,
                                                             const float* __restrict__ wts, const float* __restrict__ ws,
                                                             const float* __restrict__ dverts, int V,
                                                             float* __restrict__ partial) {
  __shared__ float g2[24 * 16];
  __shared__ float pm[207];
  __shared__ float bt[10];
  __shared__ float s_dv[128][3], s_p[128][3], s_dvp[128][3];
  const int b = blockIdx.y, t = threadIdx.x;
  const float* wsb = ws + (size_t)b * (72 + 24 * 16 + 207);
  for (int i = t; i < 24 * 16; i += blockDim.x) g2[i] = wsb[72 + i];
  for (int i = t; i < 207; i += blockDim.x) pm[i] = wsb[72 + 24 * 16 + i];
  if (t < 10) bt[t] = betas[b * 10 + t];
  __syncthreads();
  const int v0 = blockIdx.x * 128, v = v0 + t;
  const bool on = v < V;
  float p[3] = {0.f, 0.f, 0.f}, dV[3] = {0.f, 0.f, 0.f}, dvp[3] = {0.f, 0.f, 0.f};
  if (on) {
    for (int c = 0; c < 3; ++c) {
      float a = vt[v * 3 + c];
      const float* d = sd + ((size_t)v * 3 + c) * 10;
      for (int k = 0; k < 10; ++k) a = fmaf(d[k], bt[k], a);
      const float* q = pd + ((size_t)v * 3 + c) * 207;
      for (int k = 0; k < 207; ++k) a = fmaf(q[k], pm[k], a);
      p[c] = a;
    }
    float T[12];
    for (int e = 0; e < 12; ++e) T[e] = 0.f;
    for (int j = 0; j < 24; ++j) {
      const float w = wts[(size_t)v * 24 + j];
      if (w == 0.f) continue;
      for (int e = 0; e < 12; ++e) T[e] = fmaf(w, g2[j * 16 + e], T[e]);
    }
    const float* g = dverts + ((size_t)b * V + v) * 3;
    for (int r = 0; r < 3; ++r) dV[r] = g[r];
    for (int c = 0; c < 3; ++c) dvp[c] = T[c] * dV[0] + T[4 + c] * dV[1] + T[8 + c] * dV[2];
  }
  for (int c = 0; c < 3; ++c) { s_dv[t][c] = dV[c]; s_p[t][c] = p[c]; s_dvp[t][c] = dvp[c]; }
  __syncthreads();
  const int nv = min(128, V - v0);
  float* out = partial + ((size_t)b * gridDim.x + blockIdx.x) * kSmplP;
  for (int o = t; o < kSmplP; o += blockDim.x) {
    float a = 0.f;
    if (o < 288) {
      const int j = o / 12, e = o % 12, r = e >> 2, c = e & 3;
      for (int u = 0; u < nv; ++u) {
        const float w = wts[(size_t)(v0 + u) * 24 + j];
        a = fmaf(w * s_dv[u][r], c < 3 ? s_p[u][c] : 1.f, a);
      }
    } else if (o < 288 + 207) {
      const int k = o - 288;
      for (int u = 0; u < nv; ++u) {
        const float* q = pd + (size_t)(v0 + u) * 3 * 207 + k;
        a = fmaf(q[0], s_dvp[u][0], a); a = fmaf(q[207], s_dvp[u][1], a); a = fmaf(q[414], s_dvp[u][2], a);
      }
    } else if (o < 288 + 207 + 10) {
      const int k = o - 288 - 207;
      for (int u = 0; u < nv; ++u) {
        const float* q = sd + (size_t)(v0 + u) * 3 * 10 + k;
        a = fmaf(q[0], s_dvp[u][0], a); a = fmaf(q[10], s_dvp[u][1], a); a = fmaf(q[20], s_dvp[u][2], a);
      }
    } else {
      const int r = o - 288 - 207 - 10;
      for (int u = 0; u < nv; ++u) a += s_dv[u][r];
    }
    out[o] = a;
  }
}

// one block (64 threads) per sample.  ws2 per sample: dJ0 [72] | dbeta (vertex term) [10]
__global__ __launch_bounds__(64) void smpl_bwd_chain_kernel(const float* __restrict__ pose, const int* __restrict__ parents,
                                                            int center_idx, const float* __restrict__ ws,
                                                            const float* __restrict__ partial, int nblk,
                                                            const float* __restrict__ djoints, float* __restrict__ d_pose,
                                                            float* __restrict__ ws2) {
  __shared__ float acc[kSmplP];
  __shared__ float R[24][9], Rg[24][9], dR[24][9], dRg[24][9];
  __shared__ float dtg[24][3], dJ0[24][3];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* j0 = ws + (size_t)b * (72 + 24 * 16 + 207);
  for (int o = t; o < kSmplP; o += blockDim.x) {
    float a = 0.f;
    for (int k = 0; k < nblk; ++k) a += partial[((size_t)b * nblk + k) * kSmplP + o];
    acc[o] = a;
  }
  float qw = 1.f, qx = 0.f, qy = 0.f, qz = 0.f, angle = 1.f, qn = 1.f, sn = 0.f, cs = 1.f;
  float ax = 0.f, ay = 0.f, az = 0.f;
  if (t < 24) {                                        // Rodrigues, exactly as the forward kernel
    ax = pose[b * 72 + t * 3]; ay = pose[b * 72 + t * 3 + 1]; az = pose[b * 72 + t * 3 + 2];
    const float ex = ax + 1e-8f, ey = ay + 1e-8f, ez = az + 1e-8f;
    angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float nx = ax / angle, ny = ay / angle, nz = az / angle;
    const float half = angle * 0.5f;
    sn = sinf(half); cs = cosf(half);
    float w = cs, x = sn * nx, y = sn * ny, z = sn * nz;
    qn = sqrtf(w * w + x * x + y * y + z * z);
    w /= qn; x /= qn; y /= qn; z /= qn;
    qw = w; qx = x; qy = y; qz = z;
    float* r = R[t];
    r[0] = w * w + x * x - y * y - z * z; r[1] = 2 * x * y - 2 * w * z; r[2] = 2 * w * y + 2 * x * z;
    r[3] = 2 * w * z + 2 * x * y; r[4] = w * w - x * x + y * y - z * z; r[5] = 2 * y * z - 2 * w * x;
    r[6] = 2 * x * z - 2 * w * y; r[7] = 2 * w * x + 2 * y * z; r[8] = w * w - x * x - y * y + z * z;
    for (int e = 0; e < 9; ++e) { dR[t][e] = 0.f; dRg[t][e] = 0.f; }
    for (int c = 0; c < 3; ++c) { dtg[t][c] = 0.f; dJ0[t][c] = 0.f; }
  }
  __syncthreads();
  if (t == 0) {
    // global rotations (the translations are not needed by the backward)
    for (int i = 0; i < 24; ++i) {
      const int par = i == 0 ? -1 : parents[i];
      if (par < 0) { for (int e = 0; e < 9; ++e) Rg[i][e] = R[i][e]; }
      else {
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) {
            float a = 0.f;
            for (int k = 0; k < 3; ++k) a = fmaf(Rg[par][r * 3 + k], R[i][k * 3 + c], a);
            Rg[i][r * 3 + c] = a;
          }
      }
    }
    // outputs: joints_out[i] = tg_i - c, verts = ... - c with c = tg_center
    float dc[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < 24; ++i)
      for (int c = 0; c < 3; ++c) {
        const float g = djoints ? djoints[((size_t)b * 24 + i) * 3 + c] : 0.f;
        dtg[i][c] += g;
        dc[c] -= g;
      }
    for (int c = 0; c < 3; ++c) dc[c] -= acc[288 + 207 + 10 + c];
    if (center_idx >= 0) for (int c = 0; c < 3; ++c) dtg[center_idx][c] += dc[c];
    // G'_j = [Rg_j | tg_j - Rg_j J0_j]
    for (int j = 0; j < 24; ++j) {
      const float* a = acc + j * 12;
      for (int r = 0; r < 3; ++r) {
        const float gt = a[r * 4 + 3];
        for (int c = 0; c < 3; ++c) {
          dRg[j][r * 3 + c] += a[r * 4 + c] - gt * j0[j * 3 + c];
          dJ0[j][c] -= Rg[j][r * 3 + c] * gt;
        }
        dtg[j][r] += gt;
      }
    }
    // pose map: p = R_i - I, i >= 1
    for (int i = 1; i < 24; ++i)
      for (int e = 0; e < 9; ++e) dR[i][e] += acc[288 + (i - 1) * 9 + e];
    // chain, children before parents (parents[i] < i)
    for (int i = 23; i >= 0; --i) {
      const int par = i == 0 ? -1 : parents[i];
      if (par < 0) {
        for (int e = 0; e < 9; ++e) dR[i][e] += dRg[i][e];
        for (int c = 0; c < 3; ++c) dJ0[i][c] += dtg[i][c];
        continue;
      }
      float ti[3];
      for (int c = 0; c < 3; ++c) ti[c] = j0[i * 3 + c] - j0[par * 3 + c];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          float a = dtg[i][r] * ti[c];                                    // d tg_i (x) t_i
          for (int k = 0; k < 3; ++k) a = fmaf(dRg[i][r * 3 + k], R[i][c * 3 + k], a);   // dRg_i R_i^T
          dRg[par][r * 3 + c] += a;
          float d = 0.f;
          for (int k = 0; k < 3; ++k) d = fmaf(Rg[par][k * 3 + r], dRg[i][k * 3 + c], d);   // Rg_par^T dRg_i
          dR[i][r * 3 + c] += d;
        }
      for (int c = 0; c < 3; ++c) {
        float dt = 0.f;
        for (int k = 0; k < 3; ++k) dt = fmaf(Rg[par][k * 3 + c], dtg[i][k], dt);          // Rg_par^T d tg_i
        dJ0[i][c] += dt;
        dJ0[par][c] -= dt;
        dtg[par][c] += dtg[i][c];
      }
    }
  }
  __syncthreads();
  float* o2 = ws2 + (size_t)b * 82;
  if (t < 24) {
    for (int c = 0; c < 3; ++c) o2[t * 3 + c] = dJ0[t][c];
    // Rodrigues backward: R(q^), q^ = q / |q|, q = (cos h, sin h * n), h = angle / 2, n = theta / angle, angle = |theta + 1e-8|
    const float* d = dR[t];
    const float w = qw, x = qx, y = qy, z = qz;
    const float dw = 2.f * (w * (d[0] + d[4] + d[8]) - z * d[1] + y * d[2] + z * d[3] - x * d[5] - y * d[6] + x * d[7]);
    const float dx = 2.f * (x * (d[0] - d[4] - d[8]) + y * d[1] + z * d[2] + y * d[3] - w * d[5] + z * d[6] + w * d[7]);
    const float dy = 2.f * (y * (-d[0] + d[4] - d[8]) + x * d[1] + w * d[2] + x * d[3] + z * d[5] - w * d[6] + z * d[7]);
    const float dz = 2.f * (z * (-d[0] - d[4] + d[8]) - w * d[1] + x * d[2] + w * d[3] + y * d[5] + x * d[6] + y * d[7]);
    const float dot = w * dw + x * dx + y * dy + z * dz;
    const float gw = (dw - w * dot) / qn, gx = (dx - x * dot) / qn, gy = (dy - y * dot) / qn, gz = (dz - z * dot) / qn;
    const float nx = ax / angle, ny = ay / angle, nz = az / angle;
    const float dh = -sn * gw + cs * (nx * gx + ny * gy + nz * gz);
    const float dnx = sn * gx, dny = sn * gy, dnz = sn * gz;
    const float dang = 0.5f * dh - (dnx * ax + dny * ay + dnz * az) / (angle * angle);
    d_pose[b * 72 + t * 3] = dnx / angle + dang * (ax + 1e-8f) / angle;
    d_pose[b * 72 + t * 3 + 1] = dny / angle + dang * (ay + 1e-8f) / angle;
    d_pose[b * 72 + t * 3 + 2] = dnz / angle + dang * (az + 1e-8f) / angle;
  }
  if (t < 10) o2[72 + t] = acc[288 + 207 + t];
}

// d(betas) = vertex term + sum_j sum_v J_regressor[j][v] * SD[v]^T dJ0_j   (one block per sample)
__global__ __launch_bounds__(256) void smpl_bwd_betas_kernel(const float* __restrict__ sd, const float* __restrict__ jr, int V,
                                                             const float* __restrict__ ws2, float* __restrict__ d_betas) {
  __shared__ float dj[72];
  __shared__ float sm[20];
  const int b = blockIdx.x, t = threadIdx.x;
  if (t < 72) dj[t] = ws2[(size_t)b * 82 + t];
  __syncthreads();
  float a[10];
  for (int k = 0; k < 10; ++k) a[k] = 0.f;
  for (int v = t; v < V; v += blockDim.x) {
    float g[3] = {0.f, 0.f, 0.f};                      // sum_j J_regressor[j][v] * dJ0_j
    for (int j = 0; j < 24; ++j) {
      const float w = jr[(size_t)j * V + v];
      if (w == 0.f) continue;
      g[0] = fmaf(w, dj[j * 3], g[0]); g[1] = fmaf(w, dj[j * 3 + 1], g[1]); g[2] = fmaf(w, dj[j * 3 + 2], g[2]);
    }
    for (int c = 0; c < 3; ++c) {
      const float* d = sd + ((size_t)v * 3 + c) * 10;
      for (int k = 0; k < 10; ++k) a[k] = fmaf(d[k], g[c], a[k]);
    }
  }
  for (int k = 0; k < 10; ++k) {
    const float r = block_sum(a[k], sm);
    if (t == 0) d_betas[b * 10 + k] = r + ws2[(size_t)b * 82 + 72 + k];
  }
}

// ------------------------------------------------------------------ Adam
__global__ void adam_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                            float4* __restrict__ v, long n4, float b1, float b2, float eps, float step_size,
                            float inv_sqrt_bc2) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 gv = g[i];
    float4 mv = m[i], vv = v[i], pv = p[i];
#define XAS_ADAM1(f)                                                   \
    mv.f = b1 * mv.f + (1.f - b1) * gv.f;                              \
    vv.f = b2 * vv.f + (1.f - b2) * gv.f * gv.f;                       \
    pv.f -= step_size * mv.f / (sqrtf(vv.f) * inv_sqrt_bc2 + eps);
    XAS_ADAM1(x) XAS_ADAM1(y) XAS_ADAM1(z) XAS_ADAM1(w)
    m[i] = mv; v[i] = vv; p[i] = pv;
  }
}

// The averaged shadow of the parameters (xas_hip.h: xas_adam_step_ema), one element: the product rounds once, the fused
// multiply-add once.  decay == 0 gives the new parameter itself.
#define XAS_EMA1(f) ev.f = fmaf(decay, ev.f, omd * pv.f);

// adam_kernel (the same element arithmetic: XAS_ADAM1) + the shadow update while p_new is in a register: one more arena read,
// one more arena write.
__global__ void adam_ema_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                float4* __restrict__ v, float4* __restrict__ e, long n4, float b1, float b2, float eps,
                                float step_size, float inv_sqrt_bc2, float decay, float omd) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 gv = g[i];
    float4 mv = m[i], vv = v[i], pv = p[i], ev = e[i];
    XAS_ADAM1(x) XAS_ADAM1(y) XAS_ADAM1(z) XAS_ADAM1(w)
    XAS_EMA1(x) XAS_EMA1(y) XAS_EMA1(z) XAS_EMA1(w)
    m[i] = mv; v[i] = vv; p[i] = pv; e[i] = ev;
  }
}

// ------------------------------------------------------------------ guarded Adam (xas_hip.h: xas_grad_guard)
// The guard record of the header, as the kernels see it.
struct GuardRecord {
  float norm, scale;
  int skip, t, skipped;
  float step_size, inv_sqrt_bc2;
  int nonfinite;
};
static_assert(sizeof(GuardRecord) == XAS_GUARD_FLOATS * sizeof(float), "guard record layout");

constexpr int kGuardThreads = 256;

// Sum (and OR) over the block in a fixed order: a binary tree over the thread index.  Valid in thread 0.
__device__ __forceinline__ double guard_block_sum(double v, int& flag, double* s_sum) {
  const int t = threadIdx.x;
  flag = __syncthreads_or(flag);
  s_sum[t] = v;
  __syncthreads();
  for (int s = kGuardThreads / 2; s > 0; s >>= 1) {
    if (t < s) s_sum[t] += s_sum[t + s];
    __syncthreads();
  }
  return s_sum[0];
}

// One pass over the gradient arena: block b -> partial[b] = sum of g^2 over its grid-stride share, accumulated in double
// (a thread's elements in index order, then the tree above), and flags[b] = 1 if it met an element that is not finite.
// No atomics: both are pure functions of the arena's contents and the grid.
__global__ __launch_bounds__(kGuardThreads) void grad_sumsq_partial_kernel(const float4* __restrict__ g, long n4,
                                                                           double* __restrict__ partial,
                                                                           int* __restrict__ flags) {
  __shared__ double s_sum[kGuardThreads];
  double acc = 0.0;
  int bad = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 gv = g[i];
#define XAS_SUMSQ1(f)                                  \
    acc = fma((double)gv.f, (double)gv.f, acc);        \
    bad |= !(fabsf(gv.f) <= FLT_MAX);
    XAS_SUMSQ1(x) XAS_SUMSQ1(y) XAS_SUMSQ1(z) XAS_SUMSQ1(w)
#undef XAS_SUMSQ1
  }
  const double r = guard_block_sum(acc, bad, s_sum);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = r;
    flags[blockIdx.x] = bad;
  }
}

// One block: the per-block sums in index order (thread t takes the t-th run of consecutive blocks, then the tree), the
// decision, the step counter and the bias corrections of the step that follows -> the guard record.
__global__ __launch_bounds__(kGuardThreads) void grad_guard_finalize_kernel(const double* __restrict__ partial,
                                                                            const int* __restrict__ flags, int nblk,
                                                                            float max_norm, int skip_nonfinite, float lr,
                                                                            float beta1, float beta2, GuardRecord* rec) {
  __shared__ double s_sum[kGuardThreads];
  const int per = (nblk + kGuardThreads - 1) / kGuardThreads;
  double acc = 0.0;
  int bad = 0;
  for (int k = 0, b = threadIdx.x * per; k < per && b < nblk; ++k, ++b) {
    acc += partial[b];
    bad |= flags[b];
  }
  const double sumsq = guard_block_sum(acc, bad, s_sum);
  if (threadIdx.x != 0) return;
  const double norm = sqrt(sumsq);
  const float normf = (float)norm;
  float scale = 1.0f;
  if (max_norm > 0.f && max_norm <= FLT_MAX) {           // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1)
    const double c = (double)max_norm / (norm + 1e-6);   // (a NaN norm stays a NaN scale, as it does there)
    scale = c > 1.0 ? 1.0f : (float)c;
  }
  const int skip = (skip_nonfinite && (bad || !(normf <= FLT_MAX))) ? 1 : 0;
  const int t = rec->t + (skip ? 0 : 1);
  rec->norm = normf;
  rec->scale = scale;
  rec->skip = skip;
  rec->t = t;
  rec->skipped += skip;
  rec->nonfinite = bad;
  if (t >= 1) {
    rec->step_size = (float)((double)lr / (1.0 - pow((double)beta1, (double)t)));
    rec->inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)t)));
  }
}

// adam_kernel on g * scale, with scale, the bias corrections and the decision read from the guard record (uniform loads).
// A skipped step stores nothing.
__global__ void adam_guarded_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                    float4* __restrict__ v, long n4, float b1, float b2, float eps,
                                    const GuardRecord* __restrict__ rec) {
  if (rec->skip != 0) return;
  const float scale = rec->scale, step_size = rec->step_size, inv_sqrt_bc2 = rec->inv_sqrt_bc2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 gv = g[i];
    float4 mv = m[i], vv = v[i], pv = p[i];
    gv.x *= scale; gv.y *= scale; gv.z *= scale; gv.w *= scale;
    XAS_ADAM1(x) XAS_ADAM1(y) XAS_ADAM1(z) XAS_ADAM1(w)
    m[i] = mv; v[i] = vv; p[i] = pv;
  }
}

// adam_guarded_kernel + the shadow update of adam_ema_kernel.  A skipped step stores nothing: the shadow keeps its bits too.
__global__ void adam_guarded_ema_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                        float4* __restrict__ v, float4* __restrict__ e, long n4, float b1, float b2,
                                        float eps, float decay, float omd, const GuardRecord* __restrict__ rec) {
  if (rec->skip != 0) return;
  const float scale = rec->scale, step_size = rec->step_size, inv_sqrt_bc2 = rec->inv_sqrt_bc2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 gv = g[i];
    float4 mv = m[i], vv = v[i], pv = p[i], ev = e[i];
    gv.x *= scale; gv.y *= scale; gv.z *= scale; gv.w *= scale;
    XAS_ADAM1(x) XAS_ADAM1(y) XAS_ADAM1(z) XAS_ADAM1(w)
    XAS_EMA1(x) XAS_EMA1(y) XAS_EMA1(z) XAS_EMA1(w)
    m[i] = mv; v[i] = vv; p[i] = pv; e[i] = ev;
  }
}
#undef XAS_EMA1
#undef XAS_ADAM1

// ------------------------------------------------------------------ mirrored pair stack (flip test)
// x [B][C][H][W] -> y [2B][H][W][C]: y[b] = x[b] and y[B + b][h][w] = x[b][h][W - 1 - w], the batch a flip-test pass feeds
// the detector (torch.flip + torch.cat + the layout change in one pass that reads x once).  A thread owns one pixel of x:
// the loads of a wave are contiguous in every channel plane, its stores contiguous in both halves of y.
__global__ void nchw_to_nhwc_mirror_pair_kernel(const float* __restrict__ x, int B, int C, int H, int W, float* __restrict__ y) {
  const long HW = (long)H * W, pixels = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (long)gridDim.x * blockDim.x) {
    const long b = i / HW, p = i - b * HW;
    const int w = (int)(p % W);
    const float* src = x + b * C * HW + p;
    float* same = y + i * C;
    float* mirrored = y + (pixels + i + (W - 1 - 2 * w)) * C;      // pixel (B + b, h, W - 1 - w)
    for (int c = 0; c < C; ++c) {
      const float v = src[c * HW];
      same[c] = v;
      mirrored[c] = v;
    }
  }
}

static inline unsigned ew_grid(long n, int per_block = 256) {
  long b = cdiv(n, per_block);
  return (unsigned)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

}  // namespace xas

using namespace xas;

extern "C" int xas_loss_nblk(long n) { return (int)cdiv(n, (long)kLossThreads * kLossPerThread); }

extern "C" int xas_mask_loss_fwd(const float* m, const float* gt, const float* weight, long n, int mode,
                                 float* partial, float* out, void* stream) {
  XAS_REQUIRE(m && gt && partial && out && n > 0, "mask_loss: bad arguments");
  XAS_REQUIRE(!(mode & 2) || weight, "mask_loss: weighted mode needs a weight map");
  const int nblk = xas_loss_nblk(n);
  hipLaunchKernelGGL(mask_loss_partial_kernel, dim3(nblk), dim3(kLossThreads), 0, as_stream(stream), m, gt, weight, n,
                     mode, partial);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mask_loss_finalize_kernel, dim3(1), dim3(256), 0, as_stream(stream), partial, nblk, n, mode, out);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_mask_loss_bwd(const float* m, const float* gt, const float* weight, long n, int mode,
                                 const float* out, const float* grad_scalar, float* dm, void* stream) {
  XAS_REQUIRE(m && gt && out && grad_scalar && dm && n > 0, "mask_loss bwd: bad arguments");
  XAS_REQUIRE(!(mode & 2) || weight, "mask_loss bwd: weighted mode needs a weight map");
  hipLaunchKernelGGL(mask_loss_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, as_stream(stream), m, gt, weight, n, mode,
                     out, grad_scalar, dm);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_graph_aggregate(const float* x, const float* adj, int B, int N, int C, float* y, void* stream) {
  XAS_REQUIRE(x && adj && y && B > 0 && N > 0 && C > 0, "graph_aggregate: bad arguments");
  hipLaunchKernelGGL(graph_aggregate_kernel, dim3(ew_grid((long)B * N * C)), dim3(256), 0, as_stream(stream), x, adj, B,
                     N, C, y);
  XAS_LAUNCH_CHECK();
  return 0;
}

static int gln_nblk(long n) { long b = cdiv(n, (long)kGlnThreads * 8); return (int)(b > 64 ? 64 : (b < 1 ? 1 : b)); }

extern "C" size_t xas_gln_workspace_floats(long n, int groups, int C) {
  return (size_t)groups * (gln_nblk(n) * 2 + 2 + 2 * (size_t)C) + 8;
}

extern "C" int xas_gln_fwd(const float* x, const float* gamma, const float* beta, const float* residual, long rows,
                           int C, int groups, float eps, float* y, float* stats, float* workspace, void* stream) {
  XAS_REQUIRE(x && gamma && beta && y && stats && workspace && rows > 0 && C > 0 && groups > 0, "gln_fwd: bad arguments");
  const long n = rows * C;
  const int nblk = gln_nblk(n);
  hipLaunchKernelGGL(gln_partial_kernel, dim3(nblk, groups), dim3(kGlnThreads), 0, as_stream(stream), x, n, workspace);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gln_stats_kernel, dim3((unsigned)cdiv(groups, 64)), dim3(64), 0, as_stream(stream), workspace, nblk,
                     x, n, groups, stats);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gln_apply_kernel, dim3(ew_grid(n * groups)), dim3(256), 0, as_stream(stream), x, gamma, beta,
                     residual, stats, n, groups, C, eps, y);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_gln_bwd(const float* x, const float* beta, const float* dy, const float* gamma,
                           const float* stats, long rows, int C, int groups, float eps, float* dx, float* dgamma,
                           float* dbeta, float* workspace, void* stream) {
  XAS_REQUIRE(x && beta && dy && gamma && stats && dx && dgamma && dbeta && workspace && rows > 0 && C > 0 && groups > 0,
              "gln_bwd: bad arguments");
  const long n = rows * C;
  float* gsum = workspace;                              // [G][2][C]
  float* ab = workspace + (size_t)groups * 2 * C;       // [G][2]
  hipLaunchKernelGGL(gln_bwd_cols_kernel, dim3((unsigned)cdiv(C, 64), groups), dim3(1024), 0, as_stream(stream), x, dy,
                     gamma, beta, stats, rows, C, eps, gsum);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gln_bwd_scalar_kernel, dim3(groups + 1), dim3(256), 0, as_stream(stream), gamma, gsum, groups, C, ab,
                     dgamma, dbeta);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(gln_bwd_apply_kernel, dim3(ew_grid(n * groups)), dim3(256), 0, as_stream(stream), x, dy, gamma, beta,
                     stats, ab, n, groups, C, eps, dx);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_smpl_lbs_fwd(const float* pose, const float* betas, const float* v_template,
                                const float* shapedirs, const float* posedirs, const float* j_regressor,
                                const float* weights, const int* parents, int B, int V, int center_idx, float* verts,
                                float* joints, float* workspace, void* stream) {
  XAS_REQUIRE(pose && betas && v_template && shapedirs && posedirs && j_regressor && weights && parents && verts &&
                  joints && workspace, "smpl_lbs: null buffer");
  XAS_REQUIRE(B > 0 && V > 0 && center_idx < 24, "smpl_lbs: bad shape");
  hipStream_t st = as_stream(stream);
  const int per = 72 + 24 * 16 + 207;      // per-sample record: j0 | G' | pose map
  hipLaunchKernelGGL(smpl_joints_kernel, dim3(B, 24), dim3(256), 0, st, betas, v_template, shapedirs, j_regressor, V,
                     workspace, per);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(smpl_chain_kernel, dim3(B), dim3(64), 0, st, pose, parents, center_idx, workspace, joints);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(smpl_verts_kernel, dim3((unsigned)cdiv(V, 128), B), dim3(128), 0, st, betas, v_template, shapedirs,
                     posedirs, weights, workspace, V, center_idx, verts);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t xas_smpl_lbs_bwd_workspace_floats(int B, int V) {
  if (B <= 0 || V <= 0) return 0;
  return (size_t)B * cdiv(V, 128) * kSmplP + (size_t)B * 82;
}

extern "C" int xas_smpl_lbs_bwd(const float* pose, const float* betas, const float* v_template, const float* shapedirs,
                                const float* posedirs, const float* j_regressor, const float* weights, const int* parents,
                                int B, int V, int center_idx, const float* fwd_workspace, const float* d_verts,
                                const float* d_joints, float* d_pose, float* d_betas, float* workspace, void* stream) {
  XAS_REQUIRE(pose && betas && v_template && shapedirs && posedirs && j_regressor && weights && parents && fwd_workspace &&
                  d_verts && d_pose && d_betas && workspace, "smpl_lbs_bwd: null buffer");
  XAS_REQUIRE(B > 0 && V > 0 && center_idx < 24, "smpl_lbs_bwd: bad shape");
  hipStream_t st = as_stream(stream);
  const int nblk = (int)cdiv(V, 128);
  float* partial = workspace;
  float* ws2 = workspace + (size_t)B * nblk * kSmplP;
  hipLaunchKernelGGL(smpl_bwd_verts_kernel, dim3(nblk, B), dim3(128), 0, st, betas, v_template, shapedirs, posedirs, weights,
                     fwd_workspace, d_verts, V, partial);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(smpl_bwd_chain_kernel, dim3(B), dim3(64), 0, st, pose, parents, center_idx, fwd_workspace, partial, nblk,
                     d_joints, d_pose, ws2);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(smpl_bwd_betas_kernel, dim3(B), dim3(256), 0, st, shapedirs, j_regressor, V, ws2, d_betas);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                             float eps, int step, void* stream) {
  XAS_REQUIRE(p && g && m && v && n > 0 && n % 4 == 0 && step >= 1, "adam: bad arguments (n must be a multiple of 4)");
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  hipLaunchKernelGGL(adam_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, as_stream(stream), reinterpret_cast<float4*>(p),
                     reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(m), reinterpret_cast<float4*>(v),
                     n / 4, beta1, beta2, eps, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)));
  XAS_LAUNCH_CHECK();
  return 0;
}

// workspace of xas_grad_guard: one double and one flag word per block of the norm pass
extern "C" size_t xas_grad_guard_workspace_bytes(long n) {
  if (n <= 0 || n % 4 != 0) return 0;
  return (size_t)ew_grid(n / 4, kGuardThreads) * (sizeof(double) + sizeof(int));
}

extern "C" int xas_grad_guard(const float* g, long n, float max_norm, int skip_nonfinite, float lr, float beta1,
                              float beta2, void* guard, void* workspace, void* stream) {
  XAS_REQUIRE(g && guard && workspace && n > 0 && n % 4 == 0, "grad_guard: bad arguments (n must be a multiple of 4)");
  XAS_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)guard & 3) == 0 && ((uintptr_t)g & 15) == 0,
              "grad_guard: the arena must be 16-byte, the workspace 8-byte and the guard record 4-byte aligned");
  const unsigned nblk = ew_grid(n / 4, kGuardThreads);
  double* partial = static_cast<double*>(workspace);
  int* flags = reinterpret_cast<int*>(partial + nblk);
  hipLaunchKernelGGL(grad_sumsq_partial_kernel, dim3(nblk), dim3(kGuardThreads), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(g), n / 4, partial, flags);
  XAS_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_guard_finalize_kernel, dim3(1), dim3(kGuardThreads), 0, as_stream(stream), partial, flags,
                     (int)nblk, max_norm, skip_nonfinite, lr, beta1, beta2, static_cast<GuardRecord*>(guard));
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_adam_step_guarded(float* p, const float* g, float* m, float* v, long n, float beta1, float beta2,
                                     float eps, const void* guard, void* stream) {
  XAS_REQUIRE(p && g && m && v && guard && n > 0 && n % 4 == 0, "adam guarded: bad arguments (n must be a multiple of 4)");
  hipLaunchKernelGGL(adam_guarded_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(m),
                     reinterpret_cast<float4*>(v), n / 4, beta1, beta2, eps, static_cast<const GuardRecord*>(guard));
  XAS_LAUNCH_CHECK();
  return 0;
}

// the two arguments every averaged step checks alike: the shadow arena and its decay
#define XAS_REQUIRE_EMA(name)                                                                                        \
  XAS_REQUIRE(ema, name ": the shadow arena (ema) is null");                                                         \
  XAS_REQUIRE(decay >= 0.f && decay < 1.f, name ": decay must be in [0, 1), got %g", (double)decay)

extern "C" int xas_adam_step_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1,
                                 float beta2, float eps, int step, float decay, float one_minus_decay, void* stream) {
  XAS_REQUIRE(p && g && m && v && n > 0 && n % 4 == 0 && step >= 1, "adam ema: bad arguments (n must be a multiple of 4)");
  XAS_REQUIRE_EMA("adam ema");
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  hipLaunchKernelGGL(adam_ema_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, as_stream(stream), reinterpret_cast<float4*>(p),
                     reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(m), reinterpret_cast<float4*>(v),
                     reinterpret_cast<float4*>(ema), n / 4, beta1, beta2, eps, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)),
                     decay, one_minus_decay);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_adam_step_guarded_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1,
                                         float beta2, float eps, float decay, float one_minus_decay, const void* guard,
                                         void* stream) {
  XAS_REQUIRE(p && g && m && v && n > 0 && n % 4 == 0, "adam guarded ema: bad arguments (n must be a multiple of 4)");
  XAS_REQUIRE(guard, "adam guarded ema: the guard record is null");
  XAS_REQUIRE_EMA("adam guarded ema");
  hipLaunchKernelGGL(adam_guarded_ema_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(m),
                     reinterpret_cast<float4*>(v), reinterpret_cast<float4*>(ema), n / 4, beta1, beta2, eps, decay,
                     one_minus_decay, static_cast<const GuardRecord*>(guard));
  XAS_LAUNCH_CHECK();
  return 0;
}
#undef XAS_REQUIRE_EMA

extern "C" int xas_nchw_to_nhwc_mirror_pair(const float* x, int B, int C, int H, int W, float* y, void* stream) {
  XAS_REQUIRE(x && y && x != y && B > 0 && C > 0 && H > 0 && W > 0, "nchw_to_nhwc_mirror_pair: bad arguments");
  XAS_REQUIRE((long)2 * B * C * H * W < (1l << 40), "nchw_to_nhwc_mirror_pair: tensor too large");
  hipLaunchKernelGGL(nchw_to_nhwc_mirror_pair_kernel, dim3(ew_grid((long)B * H * W)), dim3(256), 0, as_stream(stream), x, B, C,
                     H, W, y);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_pose_loss_fwd(const float* pred, const float* gt, int B, int Hy, int K, int kind, float w0, float w1,
                                 float w2, float* out, void* stream) {
  XAS_REQUIRE(pred && out && B > 0 && Hy >= 1 && Hy <= 6 && K >= 1, "pose_loss: bad arguments");
  XAS_REQUIRE(kind >= 0 && kind <= 2 && (kind != 0 || gt) && (kind == 0 || K >= 17), "pose_loss: bad kind / skeleton");
  hipLaunchKernelGGL(pose_loss_fwd_kernel, dim3(1), dim3(kPoseThreads), 0, as_stream(stream), pred, gt, B, Hy, K, kind, w0,
                     w1, w2, out);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_pose_loss_bwd(const float* pred, const float* gt, int B, int Hy, int K, int kind, float w0, float w1,
                                 float w2, const float* out, const float* grad_scalar, float* grad_pred, float* grad_aux,
                                 void* stream) {
  XAS_REQUIRE(pred && out && grad_scalar && grad_pred && B > 0 && Hy >= 1 && Hy <= 6 && K >= 1,
              "pose_loss bwd: bad arguments");
  XAS_REQUIRE(kind >= 0 && kind <= 2 && (kind != 0 || gt) && (kind == 0 || K >= 17), "pose_loss bwd: bad kind / skeleton");
  hipLaunchKernelGGL(pose_loss_bwd_kernel, dim3(1), dim3(kPoseThreads), 0, as_stream(stream), pred, gt, B, Hy, K, kind, w0,
                     w1, w2, out, grad_scalar, grad_pred, grad_aux);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_lsgan_fwd(const float* logits, int B, int Hy, float target, float* out, int* idx, void* stream) {
  XAS_REQUIRE(logits && out && idx && B > 0 && Hy >= 1, "lsgan: bad arguments");
  hipLaunchKernelGGL(lsgan_fwd_kernel, dim3(1), dim3(256), 0, as_stream(stream), logits, B, Hy, target, out, idx);
  XAS_LAUNCH_CHECK();
  return 0;
}

extern "C" int xas_lsgan_bwd(const float* logits, int B, int Hy, float target, const int* idx, const float* grad_scalar,
                             float* grad_logits, void* stream) {
  XAS_REQUIRE(logits && idx && grad_scalar && grad_logits && B > 0 && Hy >= 1, "lsgan bwd: bad arguments");
  hipLaunchKernelGGL(lsgan_bwd_kernel, dim3(1), dim3(256), 0, as_stream(stream), logits, B, Hy, target, idx, grad_scalar,
                     grad_logits);
  XAS_LAUNCH_CHECK();
  return 0;
}
