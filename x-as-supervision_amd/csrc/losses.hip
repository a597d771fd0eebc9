// Losses: the mask reconstruction loss, the joint-level losses (supervision, symmetry, 2-D key-point symmetry) and the
// LSGAN term, each with its backward.  gfx950.
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

// The key-point symmetry term of one sample and coordinate c: the mid-point of joints (11, 14) minus joint K-1 and the
// mid-point of joints (1, 4) minus joint 0.  PRE scales both operands by s BEFORE the subtraction (the 3-D forward:
// mm -> m); the 3-D backward scales the difference instead, and each keeps its own rounding.
template <bool PRE>
__device__ __forceinline__ float mid_residual(const float* p, int a, int b, int anchor, int c, float s) {
  const float mid = (p[a * 3 + c] + p[b * 3 + c]) / 2, an = p[anchor * 3 + c];
  return PRE ? mid * s - an * s : mid - an;
}
struct MidPair { float m0, m1; };
template <bool PRE = false>
__device__ __forceinline__ MidPair mid_residuals(const float* p, int K, int c, float s = 1.f) {
  return {mid_residual<PRE>(p, 11, 14, K - 1, c, s), mid_residual<PRE>(p, 1, 4, 0, c, s)};
}
// Their gradient into q: s * m to the residual, so +1/2 of it to each joint of the pair and -1 to the anchor.
__device__ __forceinline__ void mid_scatter(float* q, int K, int c, float s, const MidPair& r) {
  q[11 * 3 + c] += 0.5f * s * r.m0; q[14 * 3 + c] += 0.5f * s * r.m0; q[(K - 1) * 3 + c] -= s * r.m0;
  q[1 * 3 + c] += 0.5f * s * r.m1; q[4 * 3 + c] += 0.5f * s * r.m1; q[0 * 3 + c] -= s * r.m1;
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
        for (int c = 0; c < 3; ++c) {
          const MidPair r = mid_residuals<true>(p, K, c, 1e-3f);
          a_kp = fmaf(r.m0, r.m0, a_kp); a_kp = fmaf(r.m1, r.m1, a_kp);
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
            const MidPair r = mid_residuals(p, K, c);
            a2 = fmaf(r.m0, r.m0, a2); a2 = fmaf(r.m1, r.m1, a2);
          }
        }
        acc += w2 * block_sum(a2, sm) / (float)(B * 4);
      }
    } else {
      for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* p = pred + ((size_t)b * Hy + h) * K * 3;
        for (int c = 0; c < 2; ++c) {
          const MidPair r = mid_residuals(p, K, c);
          acc = fmaf(r.m0, r.m0, acc); acc = fmaf(r.m1, r.m1, acc);
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
        const MidPair r = mid_residuals(p, K, c);
        const float m0 = r.m0 * 1e-3f, m1 = r.m1 * 1e-3f;
        mid_scatter(q, K, c, 1.f, {sk * m0 * 1e-3f, sk * m1 * 1e-3f});      // the products are the gradients: scale 1
      }
      if (gt && gaux) {
        const float* p2 = gt + ((size_t)b * Hy + best) * K * 3;
        float* q2 = gaux + ((size_t)b * Hy + best) * K * 3;
        const float s2 = g * w2 * 2.f / (float)(B * 4);
        for (int c = 0; c < 2; ++c) mid_scatter(q2, K, c, s2, mid_residuals(p2, K, c));
      }
    } else {
      const float sk = g * w0 * 2.f / (float)(B * 4);
      for (int c = 0; c < 2; ++c) mid_scatter(q, K, c, sk, mid_residuals(p, K, c));
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
