/*
 * xas_hip.h - C ABI of libxas_hip.so: the MI355X (gfx950) kernels behind the
 * X-as-Supervision training step.
 *
 * The reference (Charrrrrlie/X-as-Supervision) is pure Python/PyTorch and has no FFI of
 * its own; the boundary a maintainer binds is "one call per fused op", replacing the
 * chains of ATen/cuDNN kernels listed beside each entry (reference file:line).  The
 * Python host side (x-as-supervision_amd/xas_amd) binds these with ctypes and wraps
 * them in torch.autograd.Function; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless typed otherwise; buffers are
 *     owned by the caller; the library allocates nothing and never synchronises;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it;
 *   - activations are NHWC ("channels last"): x[n][h][w][c];
 *   - return value 0 = enqueued; != 0 = rejected on the host before any launch
 *     (bad shape / unsupported size), message via xas_last_error().
 */
#ifndef XAS_HIP_H
#define XAS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* xas_last_error(void);
/* Kernel-variant selectors (xas_set_tuning flags) kept for coverage tests and A/B runs: 0 = the shipped configuration; results
 * agree to accumulation-order noise under every flag (tests/test_gpu_nn.py::test_conv_kernel_variants,
 * tests/test_gpu_tap_kernels.py, tests/test_gpu_persistent_gemm.py).  xas_amd/_lib.py mirrors the table as TUNE_*. */
enum {
  /* not a caller's flag: the launcher of the bf16-split weight-gradient kernel sets it in the kernel's own copy of the flags */
  XAS_TUNE_WGRAD_SPLIT_XCD = 1,              /* all tiles of a pixel split on one XCD (split count a multiple of 8) */
  /* exact-fp32 kernels (XAS_PREC_F32) */
  XAS_TUNE_PLAIN_KLOOP = 32,                 /* plain K-loop in fwd / dgrad instead of the pipelined one */
  XAS_TUNE_GLOBAL_LOAD = 64,                 /* global-load fwd / dgrad kernels (the >= 2 GiB fallback) */
  XAS_TUNE_WGRAD_GLOBAL_LOAD = 128,          /* the same for the weight gradient */
  XAS_TUNE_WGRAD_ALT_ORDER = 8192,           /* the weight-gradient block order that is not shipped: plain instead of XCD-grouped
                                              * (buffer-load kernel), one pixel split per XCD instead of plain (global-load kernel) */
  XAS_TUNE_WGRAD_PLAIN_KLOOP = 524288,       /* plain K-loop in the weight gradient */
  /* batch-norm / column-sum reductions */
  XAS_TUNE_SLAB_SHIFT = 15,                  /* bits 15-16: slab target of the column reduction, (flags >> SHIFT) & MASK ... */
  XAS_TUNE_SLAB_MASK = 3,
  XAS_TUNE_SLAB_512 = 32768,                 /* ... 0 = 256 (shipped), 1 = 512, */
  XAS_TUNE_SLAB_128 = 65536,                 /* 2 = 128, */
  XAS_TUNE_SLAB_64 = 98304,                  /* 3 = 64 */
  XAS_TUNE_COL_REDUCE_LEAN = 262144,         /* the 64-VGPR build of the backward column sums (8 waves per SIMD, 12 bytes of scratch per lane) instead of the 120-VGPR one (4 waves, none) */
  /* bf16-split kernels (XAS_PREC_F16X3 / XAS_PREC_BF16X6) */
  XAS_TUNE_GENERAL_KERNELS = 1 << 22,        /* three effects: no tap re-use kernels (stride-1 3x3 layers on the implicit-GEMM kernels:
                                              * forward, data and weight gradient), no streaming batch-norm apply / backward-apply
                                              * kernels (every layer on the general ones) AND the soft-argmax head's general
                                              * policy for power-of-two cube sides too (the workspace query follows) */
  XAS_TUNE_NO_WIDE_TILES = 1 << 23,          /* no 64 x 256 tiles for layers whose output channels are a multiple of 256 */
  XAS_TUNE_NO_STEM_WGRAD = 1 << 24,          /* the general weight-gradient kernel for the 7x7 stem instead of stem_wgrad_kernel */
  XAS_TUNE_STEM_FWD_F32 = 1 << 25,           /* the exact-fp32 stem forward kernel in the f16x3 mode too */
  XAS_TUNE_NO_X6P = 1 << 26,                 /* no persistent 1x1 kernel (igemm_x6p_kernel): one 64 x 256 tile per block */
  XAS_TUNE_X6P_ANY_K = 1 << 27               /* persistent 1x1 kernel for every K, also above the build's XAS_X6P_MAX_K */
};
int xas_set_tuning(int flags);
/* Arithmetic of the MFMA convolutions (forward, data gradient, weight gradient).  All modes keep fp32 activations, fp32
 * master weights and fp32 accumulation; they differ in how a product of two fp32 operands is formed:
 *   XAS_PREC_F16X3 (default)  every fp32 operand is split into two fp16 pieces x = h1 + h2 + e, |e| <= 2^-22 |x| (round to
 *                   nearest twice), after an exact power-of-two scaling that keeps both pieces inside fp16's normal
 *                   range: weights as 2^10 w (|w| < 64; anything larger raises xas_f16_weight_overflow), and EVERY tensor
 *                   operand - activation or gradient - at the scale that puts its maximum in [2^14, 2^15): the maximum comes
 *                   with the call (xas_conv_shape.grad_amax / x_amax), recorded by the kernel that wrote the tensor
 *                   (xas_bn_apply_amax, xas_bn_bwd_apply_amax, xas_head_softargmax_bwd_amax) or by xas_abs_max.  There is
 *                   no fixed activation scale, hence no range activations must stay in (r04).  Three partial products
 *                   h1 g1 + h1 g2 + h2 g1, each exact in fp32, accumulated by v_mfma_f32_32x32x16_f16: 3 instead of 6 matrix
 *                   instructions per K = 16.  Measured distance to a float64 convolution: the same as the exact-fp32 MFMA
 *                   path's (its own accumulation error dominates: 5e-7 relative at K = 576).  A launch that comes WITHOUT
 *                   the maxima of its tensor operands runs as bf16x6 (range-free by construction);
 *   XAS_PREC_BF16X6  every fp32 operand is split exactly into three bf16 pieces and six exact partial products
 *                   are accumulated in fp32 by v_mfma_f32_32x32x16_bf16: per-product error below one fp32 rounding
 *                   (1.09e-7 relative against float64 at K = 64, exact-fp32 MFMA 1.06e-7), 2.67x the fp32-MFMA math rate; no
 *                   assumption on operand ranges;
 *   XAS_PREC_F32    v_mfma_f32_32x32x2_f32, bit for bit a k-ordered fmaf chain;
 *   XAS_PREC_BF16   operands rounded to bf16 once (NOT fp32 accurate; a variant that is reported separately).
 * xas_set_precision sets the process default; a call overrides it with xas_conv_shape.mode = 1 + XAS_PREC_* (0 = default).
 * In the split modes forward / data gradient take PRE-SPLIT weights: see xas_conv_weight_planes / xas_split_weight. */
enum { XAS_PREC_F32 = 0, XAS_PREC_BF16 = 1, XAS_PREC_BF16X6 = 2, XAS_PREC_F16X3 = 3 };
/* A RECORDED MAXIMUM ("amax slot": xas_conv_shape.grad_amax / x_amax, the amax_out arguments) is an array of
 * XAS_AMAX_SLOT_FLOATS floats in device memory, 16-byte aligned: XAS_AMAX_SUB sub-maxima XAS_AMAX_STRIDE floats (128 bytes)
 * apart; the value is the maximum over the sub-maxima (the other floats are not touched).  Producers merge with one atomic
 * per block into the sub-maximum the block index selects - one address per tensor serialised 16 384 atomics per launch, 190 us.
 * ZERO the whole array before the first producer merges into it.  To hand over a maximum computed elsewhere, write it to
 * element 0 of a zeroed array. */
#define XAS_AMAX_SUB 32
#define XAS_AMAX_STRIDE 32
#define XAS_AMAX_SLOT_FLOATS (XAS_AMAX_SUB * XAS_AMAX_STRIDE)
enum { XAS_GRAD_IS_X = 0x100 };      /* flag of xas_conv_shape.mode */
int xas_set_precision(int mode);
int xas_get_precision(void);
int xas_abi_version(void);

/* ------------------------------------------------------------------------------------
 * Soft-argmax ("integral") head.
 * Replaces keypoint_detector_integral_multi.py:69-88 (softmax, six marginal sums, peak
 * pick, topk, two avg_pool1d, two gathers) and keypoint_detector_integral.py:48-63.
 *
 * logits  [B][H][W][K*D] (NHWC storage of the reference's [B, K*D, H, W]); D==H==W, the heat-map is a cube.
 *          Accepted: D % 4 == 0 and 4 <= D <= 128 (input patches of side 4*D up to 512), for every K >= 1.  One kernel family
 *          (head.hip): D in {4,8,16,32,64} runs on its power-of-two policy whenever that policy's block exists for K (at most
 *          1024 threads, no more pixel slots than pixels), every other (D, K) on the general one, which tiles the joints;
 *          any other D is refused with status 1 (xas_head_workspace_floats: 0) and a message that names this range.
 * num_hypo >= 1 with neighbor > 0 : multi-hypothesis head; num_hypo == 1 and
 * neighbor == 0 : single-hypothesis head (plain expectation along depth).
 * kps      [B][num_hypo][K][3]   normalised to [-1,1)
 * z_idx    [B][K][num_hypo] int64 (depth-peak bins, 1..D-2; ties: lower index first)
 * depth_prob_map [groups][K][D]  (depth marginal of the FIRST sample of each of `groups` equal sub-batches:
 *                                 sample 0 for groups = 1, multi.py:45; one per camera in a camera-batched pass)
 * stats    [B][K][XAS_HEAD_STATS] saved for backward (lse, X, Y, Z_h, S_h ...)
 * partial  workspace, xas_head_workspace_floats(B,K,D) floats: [B][nchunk][K][3 + D] first-pass records
 * ---------------------------------------------------------------------------------- */
#define XAS_HEAD_STATS 16
size_t xas_head_workspace_floats(int B, int K, int D);
int xas_head_softargmax_fwd(const float* logits, int B, int K, int D, int num_hypo, int neighbor,
                            float* kps, int64_t* z_idx, float* depth_prob_map, int groups, float* stats,
                            float* partial, void* stream);
/* grad_logits [B][H][W][K*D] = d loss / d logits given grad_kps [B][num_hypo][K][3].
 * coef: workspace of B*K*(4+D) floats. */
/* Second pass of xas_head_softargmax_fwd over partial records produced elsewhere (xas_conv_fwd_head): same outputs. */
int xas_head_softargmax_from_partials(const float* partial, int B, int K, int D, int nchunk, int num_hypo, int neighbor,
                                      float* kps, int64_t* z_idx, float* depth_prob_map, int groups, float* stats,
                                      void* stream);
/* Flip test: the head of keypoint_detector_integral_multi.py:36-88 (and keypoint_detector_integral.py:21-65 when
 * neighbor == 0) on the AVERAGE of an image's heat-map and the mirrored, left/right-swapped heat-map of its horizontal
 * mirror.  `partial` holds the first-pass records of 2B images, image B + b being the mirror of image b; `perm` is a DEVICE
 * int32 [K] table, perm[k] = the joint that joint k takes from the mirrored image (its left/right partner; k itself for an
 * unpaired joint; every entry in [0, K): the caller checks it, an entry outside reads as k).  A mirror leaves a record's depth
 * sums and H moment alone and turns its W moment into (W - 1) * sum e - sum e*w, so the merge needs only the records of
 * (b, k) and (B + b, perm[k]), each normalised by its own softmax sum.  kps, z_idx and depth_prob_map are those of
 * xas_head_softargmax_from_partials for B images ([B][num_hypo][K][3], [B][K][num_hypo], [groups][K][D], B % groups == 0).
 * Forward only: no statistics for a backward are written. */
int xas_head_softargmax_flip_from_partials(const float* partial, int B, int K, int D, int nchunk, int num_hypo, int neighbor,
                                           const int* perm, float* kps, int64_t* z_idx, float* depth_prob_map, int groups,
                                           void* stream);
/* The same from the logits [2B][H][W][K*D] (keypoint_detector_integral_multi.py:36-88 on the averaged heat-map): the first
 * pass of xas_head_softargmax_fwd over the 2B images, then the merge above.  partial: workspace of
 * xas_head_workspace_floats(2B, K, D) floats. */
int xas_head_softargmax_fwd_flip(const float* logits, int B, int K, int D, int num_hypo, int neighbor, const int* perm,
                                 float* kps, int64_t* z_idx, float* depth_prob_map, int groups, float* partial, void* stream);

int xas_head_softargmax_bwd(const float* logits, const float* stats, const int64_t* z_idx,
                            const float* grad_kps, int B, int K, int D, int num_hypo, int neighbor,
                            float* grad_logits, float* coef, void* stream);
/* Same, and max |grad_logits| is merged into *amax_out (device float, zeroed by the caller; NULL: none): the scale of the
 * gradient operand of the final 1x1 convolution's f16x3 gradient launches (xas_conv_shape.grad_amax). */
int xas_head_softargmax_bwd_amax(const float* logits, const float* stats, const int64_t* z_idx,
                                 const float* grad_kps, int B, int K, int D, int num_hypo, int neighbor,
                                 float* grad_logits, float* coef, float* amax_out, void* stream);

/* Heat-map spread: the spatial confidence of every joint (no counterpart in the reference).  With p the soft-max over a
 * joint's D*H*W logits and q(h, w) = sum_d p its x-y marginal,
 *   spread [B][K][XAS_HEAD_SPREAD] = { E_q[w], E_q[h], Var_q[w], Var_q[h], Cov_q[w, h] }   in heat-map cells,
 * w and h being the integer cell indices.  logits, the accepted (D, K) and the refusals (status 1, workspace size 0, a
 * message that names the range) are those of xas_head_softargmax_fwd.  One streaming pass with its own online soft-max (the
 * logits are read once), records in mean / centred-second-moment form merged pairwise in a fixed order (no atomics: two calls
 * agree bit for bit), then one wave per (b, k).  Variances are >= 0; a NaN logit makes that joint's five numbers NaN and no
 * other's.  workspace: xas_head_spread_workspace_floats(B, K, D) floats ([B][nchunk][K][7] records).  Forward only. */
#define XAS_HEAD_SPREAD 5
size_t xas_head_spread_workspace_floats(int B, int K, int D);
int xas_head_spread(const float* logits, int B, int K, int D, float* spread /*[B][K][5]*/, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * Patch -> world geometry, all hypotheses in one launch.
 * Replaces modules/util.py:128-152 -> :61-95 (clone/index_put chains + two batched
 * torch.linalg.inv) called per camera per hypothesis at modules/model.py:72-84.
 * kps [B][Hy][K][3]; trans_image [B][2][3]; k_mat [B][3][3]; pelvis [B][3];
 * rot_world [B][3][3]; trans_world [B][3]; world [B][Hy][K][3].
 * flags: bit0 is_norm, bit1 mono, bit2 patch (reference defaults: is_norm|patch).
 * ---------------------------------------------------------------------------------- */
#define XAS_GEO_NORM 1
#define XAS_GEO_MONO 2
#define XAS_GEO_PATCH 4
#define XAS_GEO_IMAGE 8   /* forward only: stop after patch -> image (u px, v px, depth mm), util.py:61-83 */
int xas_patch_to_world_fwd(const float* kps, const float* trans_image, const float* k_mat,
                           const float* pelvis, const float* rot_world, const float* trans_world,
                           int B, int Hy, int K, float image_size, float rect_width, int flags,
                           float* world, void* stream);
int xas_patch_to_world_bwd(const float* kps, const float* grad_world, const float* trans_image,
                           const float* k_mat, const float* pelvis, const float* rot_world,
                           const float* trans_world, int B, int Hy, int K, float image_size,
                           float rect_width, int flags, float* grad_kps, void* stream);

/* ------------------------------------------------------------------------------------
 * World -> patch geometry (the other direction), all hypotheses in one launch.
 * Replaces modules/util.py:155-168 -> :116-125 (world -> image) and :98-113 (image -> patch), and with
 * pre_rot / pelvis_origin the front of project_smpl_to_patch_kps (:376-382: torch.bmm(joints, global_rot) * 1000
 * + convert_pelvis_to_world, :343-352, whose batched torch.linalg.inv becomes a closed-form adjugate).
 * pts [B][Hy][K][3]; pre_rot [B][3][3] or NULL: p <- (p . pre_rot[b]) * pre_scale (row vector times matrix);
 * pelvis_origin != 0: p <- p + inv(rot_world)(pelvis - trans_world); camera arrays as xas_patch_to_world_fwd;
 * out [B][Hy][K][3].  No clamps: a camera-space depth <= 0 gives what IEEE division gives.
 * flags: XAS_GEO_NORM (normalised patch coordinates), XAS_GEO_IMAGE (stop after world -> image: u px, v px, depth mm),
 * XAS_GEO_WORLD (stop after the rotation / pelvis shift: world mm - convert_verts, :367-373, and :343-352 itself).
 * Backward: grad_pts, and with pre_rot grad_pre_rot [B][3][3] (sum over the Hy*K points of a sample, one block per
 * sample, fixed order, no atomics: bit-reproducible).  Camera arrays receive no gradient.
 * ---------------------------------------------------------------------------------- */
#define XAS_GEO_WORLD 16
int xas_world_to_patch_fwd(const float* pts, const float* pre_rot, float pre_scale, int pelvis_origin,
                           const float* trans_image, const float* k_mat, const float* pelvis,
                           const float* rot_world, const float* trans_world, int B, int Hy, int K,
                           float image_size, float rect_width, int flags, float* out, void* stream);
int xas_world_to_patch_bwd(const float* pts, const float* grad_out, const float* pre_rot, float pre_scale,
                           int pelvis_origin, const float* trans_image, const float* k_mat, const float* pelvis,
                           const float* rot_world, const float* trans_world, int B, int Hy, int K,
                           float image_size, float rect_width, int flags, float* grad_pts, float* grad_pre_rot,
                           void* stream);

/* ------------------------------------------------------------------------------------
 * Line-mask renderer fused with the max over lines.
 * Replaces modules/util.py:21-59 (about 25 ATen kernels, 419 MB intermediates) plus
 * torch.max(dim=1) at modules/model.py:94,96.
 * kps: joints, (x,y) of joint j of sample b at kps[b*kp_stride_b + j*kp_stride_j + {0,1}].
 * parents/children: L int32 each (device).  fine_mask: bit l set -> exponent x2
 * (modules/util.py:50-53, applied by the host when L >= 21).
 * mask [B][1][S][S].   partial: workspace B*nblk*K*2 floats, nblk = xas_lines_nblk(S).
 * Both passes take a pixel's line by one rule: the first line with a NaN exponent if there is
 * one, else the first maximum.  A NaN or infinite joint therefore makes the whole mask of its
 * sample NaN, and the backward sends NaN to both end points of every line that touches it
 * (what exp, torch.max and autograd give); other samples are not affected.
 * ---------------------------------------------------------------------------------- */
int xas_lines_nblk(int S);
int xas_draw_lines_max_fwd(const float* kps, long kp_stride_b, long kp_stride_j, int B, int K,
                           const int* parents, const int* children, int L, unsigned fine_mask,
                           float body_width, int S, float* mask, void* stream);
int xas_draw_lines_max_bwd(const float* kps, long kp_stride_b, long kp_stride_j, int B, int K,
                           const int* parents, const int* children, int L, unsigned fine_mask,
                           float body_width, int S, const float* grad_mask, float* partial,
                           float* grad_kps_xy /* [B][K][2] */, void* stream);

/* ------------------------------------------------------------------------------------
 * Convolution family: MFMA implicit GEMM on NHWC fp32 activations (fp32-accurate f16x3 by default - bf16x6 for launches
 * without operand maxima -, exact fp32 MFMA on request: XAS_PREC_*).
 * Replaces the cuDNN calls behind nn.Conv2d / nn.ConvTranspose2d / nn.Linear in
 * integral_base_modules/resnet.py:16-47, deconv_head.py:24-35, physique_network.py:15-50,
 * discriminator.py:8-21 and torchvision's Bottleneck.
 *
 * x  [N][Hi][Wi][Cin]      w  packed [Cout][R][S][Cin] (see xas_pack_weight)
 * y  [N][Ho][Wo][Cout]     Ho = (Hi + 2*pad - R)/stride + 1
 * bias (Cout) may be NULL.  One route function per pass (conv.hip: fwd_route, dgrad_route, wgrad_route) decides the
 * kernel, for the launch and for every query below.  Forward: the 7x7 stem without a bias and the one-channel 3x3 layers
 * have kernels of their own; other shapes outside the MFMA tiles (Cin % 32 != 0 or Cout < 16) run a direct VALU kernel.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  int N, Hi, Wi, Cin;
  int Cout, R, S;
  int stride, pad;
  int Ho, Wo;
  int mode;          /* low byte: 0 = process default precision (xas_set_precision), otherwise 1 + XAS_PREC_* for this call;
                      * | XAS_GRAD_IS_X: in a weight-gradient call grad_amax describes the `x` argument and x_amax the `dy`
                      *   argument (the weight gradient of a ConvTranspose2d, whose gradient tensor is passed as `x`) */
  const float* grad_amax;   /* NULL, or a DEVICE pointer to max |v| over the tensor operand of the call, complete on the call's
                              * stream: the input x of a forward-type launch (xas_conv_fwd*), dy of a data-gradient-type launch
                              * (xas_conv_dgrad*; for a ConvTranspose2d forward that is its input activation), dy of a weight
                              * gradient.  An upper bound is as good as the maximum.  XAS_PREC_F16X3 splits that tensor into two fp16
                              * pieces at the power-of-two scale that puts the maximum just below 2^15; without it the launch runs
                              * as bf16x6.  Producers: xas_bn_apply_amax, xas_bn_bwd_apply_amax, xas_head_softargmax_bwd_amax,
                              * xas_abs_max. */
  const float* x_amax;      /* weight gradient only: the same for its `x` argument (both maxima -> f16x3, else bf16x6) */
} xas_conv_shape;

/* Which weight buffer xas_conv_fwd* (pass 0) / xas_conv_dgrad* (pass 1) expect for this shape in its precision mode:
 * 0 = fp32 packed weights (xas_pack_weight); 1 or 3 = that many bf16 planes, 2 = two fp16 planes of 2^10 w: xas_split_weight of the packed weights
 * [rows][K] with K = R*S*Cin (pass 0, rows = Cout) or R*S*Cout (pass 1, rows = Cin).  The split layout is the MFMA operand
 * image [rows / 32][K / 16][planes][64 lanes][8 bf16] (rows zero-padded to a multiple of 32): the kernels load it straight
 * into operand registers.  Shapes outside the MFMA tiles (stem, one-channel layers) always take fp32 weights.  Built once
 * per optimizer step and weight. */
int xas_conv_weight_planes(const xas_conv_shape* s, int pass);
/* Kernel family a pass of this shape runs on (0 forward-type, 1 data-gradient-type, 2 weight gradient): 0 no MFMA (direct /
 * one-channel kernels), 1 exact-fp32 MFMA, 2 bf16 MFMA, 3 bf16x6 MFMA, 4 f16x3 MFMA.  For measurement (bench.py prices a launch against
 * the peak of the pipe it uses). */
int xas_conv_kernel_class(const xas_conv_shape* s, int pass);
/* f16x3: 1 if a weight of magnitude >= 64 (or a NaN) has gone through xas_split_weight / xas_prepare_weights since the flag
 * was last cleared - such a weight does not fit the 2^10 w scaling of the fp16 pieces and the results of its layer are
 * inf / NaN; 0 otherwise; -1 on a HIP error.  SYNCHRONISES the device (call it rarely: engine.TrainStep every 64 steps).
 * reset != 0 clears the flag.  Remedy: XAS_PREC_BF16X6. */
int xas_f16_weight_overflow(int reset);
/* The same flag WITHOUT a synchronisation: writes it (0 / 1) to the device word *device_out on `stream`; the flag is not
 * cleared.  The caller copies the word to pinned host memory asynchronously and reads it once that copy has completed:
 * engine.TrainStep looks at it one step late, every step, so that a weight leaving the range is reported within a step or two
 * instead of at the next 64-step poll. */
int xas_f16_weight_overflow_peek(unsigned* device_out, void* stream);
size_t xas_split_weight_bytes(long rows, long K, int pieces);
int xas_split_weight(const float* w_packed, void* w_split, long rows, long K, int pieces, void* stream);

/* Pack + split of MANY layers in one launch (the head of every optimisation step: the reference hands cuDNN the fp32
 * parameters, modules/integral_base_modules/resnet.py:16-47; this library wants fragment-ordered bf16 planes of them, rebuilt
 * after every optimizer step).  descs: device array of n entries of 12 int64 each:
 *   { src (OIHW fp32, device), dst (device, xas_split_weight_bytes(rows, K, planes) bytes), Cout, Cin, R, S,
 *     transposed (0: rows = Cout, K = (r, s, ci); 1: rows = Cin, K = (r, s, co), as xas_pack_weight),
 *     planes (3, 2 or 1), rows, K, first block of the entry (prefix sum of ceil(ceil(rows / 32) * (K / 16) * 64 / 256)), 0 }
 * blocks: total number of blocks.  Results are bit-identical to xas_pack_weight followed by xas_split_weight. */
int xas_prepare_weights(const void* descs, int n, long blocks, void* stream);

int xas_conv_fwd(const float* x, const float* w_packed, const float* bias, float* y,
                 const xas_conv_shape* s, void* stream);

/* Final 1x1 convolution of the detector with the soft-argmax head's first pass in its epilogue (forward half):
 * replaces modules/integral_base_modules/deconv_head.py:34-35 followed by the softmax / marginal reductions of
 * modules/keypoint_detector_integral_multi.py:36-62,70-74.  y (the logits, kept for the backward) is written as by xas_conv_fwd;
 * head_partial receives [N][chunks][K][3 + D] floats, chunks = xas_conv_fwd_head_chunks(s, K, D) records of 64 pixels per image
 * (0: the shape is not taken - call xas_conv_fwd and xas_head_softargmax_fwd).  Finish with xas_head_softargmax_from_partials. */
int xas_conv_fwd_head_chunks(const xas_conv_shape* s, int K, int D);
int xas_conv_fwd_head(const float* x, const float* w_packed, const float* bias, float* y, const xas_conv_shape* s,
                      int K, int D, float* head_partial, void* stream);
/* Bias-free convolution followed by training-mode batch norm (resnet.py:17-18 conv1/bn1 and every torchvision Bottleneck
 * conv/bn pair, resnet.py:2): y = conv(x, w) AND the per-group batch statistics of y in one call - the conv epilogue
 * emits per-tile column sums, so y is not read again for its statistics (falls back to xas_conv_fwd + xas_bn_stats when
 * the tile grid does not line up with the groups).  pivot [Cout] or NULL: a value near the channel means (the running
 * mean) that the sums are taken around.  mean / var_biased / out_stride / count_out / running_* / momentum: as
 * xas_bn_stats.  workspace: xas_conv_fwd_bnstats_workspace_floats(s, groups). */
size_t xas_conv_fwd_bnstats_workspace_floats(const xas_conv_shape* s, int groups);
int xas_conv_fwd_bnstats(const float* x, const float* w_packed, float* y, const xas_conv_shape* s, int groups,
                         const float* pivot, float* mean, float* var_biased, long out_stride, float* count_out,
                         float* workspace, float* running_mean, float* running_var, float momentum, void* stream);
/* Backward of  h = relu(batch_norm(xb)) -> conv(h)  (torchvision Bottleneck conv/bn/relu chains, resnet.py:2) in one call:
 * data gradient of the convolution `s` (dy: gradient of its output, w_packed_t as xas_conv_dgrad), ReLU mask re-derived
 * from xb, and the rank-local batch-norm backward (mean / var_biased [groups][Cin], count = rows per group).
 * Outputs: dx = gradient wrt xb; sums [groups][2][Cin] (sum dz | sum dz * xhat); dbeta_acc / dgamma_acc (both or neither
 * NULL) += local parameter gradients; dz: scratch of xb's size.  workspace:
 * xas_conv_dgrad_bn_bwd_workspace_floats(s, groups).  The reductions ride in the data gradient's epilogue when its tile
 * grid lines up with the groups (stride 1), otherwise the call is xas_conv_dgrad + xas_bn_bwd_reduce + xas_bn_bwd_apply.
 * Operand maxima in `s` are IGNORED: w_packed_t is always the format xas_conv_weight_planes(s, 1) names for the shape with
 * grad_amax == NULL (three bf16 planes in both split modes - the fused epilogue exists for that format only). */
size_t xas_conv_dgrad_bn_bwd_workspace_floats(const xas_conv_shape* s, int groups);
int xas_conv_dgrad_bn_bwd(const float* dy, const float* w_packed_t, const xas_conv_shape* s, const float* xb,
                          const float* mean, const float* var_biased, const float* gamma, const float* beta, float eps,
                          int groups, double count, float* dz, float* dx, float* sums, float* workspace, float* dbeta_acc,
                          float* dgamma_acc, void* stream);
/* dx = conv_transpose(dy, w): also the FORWARD of nn.ConvTranspose2d (deconv_head.py:27-29)
 * with roles swapped.  w_packed_t: [Cin][R][S][Cout] (xas_pack_weight transposed=1). */
int xas_conv_dgrad(const float* dy, const float* w_packed_t, float* dx,
                   const xas_conv_shape* s, void* stream);
/* Same, but dx += result: the residual-branch gradient is already in dx (one read-modify-write instead of a
 * separate gradient-accumulation kernel per bottleneck).  MFMA path only (Cout % 32 == 0, Cin % 4 == 0, Cin >= 16). */
int xas_conv_dgrad_acc(const float* dy, const float* w_packed_t, float* dx, const xas_conv_shape* shape, void* stream);
/* dx = dgrad(dy, W) + relu'(mask) * dprev: the block-input gradient of a bottleneck without a projection, with the skip
 * gradient formed in the epilogue from the block-OUTPUT gradient dprev [like dx] and the sign bytes xas_bn_apply wrote for
 * the block output (one byte per float4 of dx): the skip gradient tensor is never materialised.  Same shape limits as
 * xas_conv_dgrad_acc; dx is written, not read. */
int xas_conv_dgrad_acc_masked(const float* dy, const float* w_packed_t, float* dx, const xas_conv_shape* s,
                              const float* dprev, const uint8_t* mask, void* stream);
/* What a launch of xas_conv_fwd (pass 0; has_bias != 0: a bias comes with the call) or of xas_conv_dgrad* (pass 1) on this
 * shape would run - under the shape's precision, the operand maximum it carries and the current tuning flags - written to
 * out[XAS_PLAN_INTS].  Host only: never touches the device; reads the functions the launches read (16-byte aligned
 * operands assumed).  Fields that do not apply are 0.  Non-zero status: null / invalid arguments, or a shape the launch
 * refuses for its dimensions (Ho / Wo inconsistent in a forward, Hi / Wi too small in a data gradient, tensors beyond 32-bit
 * row indices or beyond the offset range of the split kernels).  For tests (tests/test_gpu_igemm.py) and measurement. */
enum {
  XAS_PLAN_ROUTE = 0,        /* XAS_ROUTE_* */
  XAS_PLAN_KERNEL = 1,       /* XAS_KERNEL_* (MFMA route) */
  XAS_PLAN_BM = 2,           /* tile: rows (pixels) ... */
  XAS_PLAN_BN = 3,           /* ... and columns (produced channels) */
  XAS_PLAN_PIPELINED = 4,    /* exact-fp32 kernels: 1 pipelined K-loop, 0 plain */
  XAS_PLAN_PHASES = 5,       /* stride phases (grid z): 1 forward, stride^2 data gradient */
  XAS_PLAN_PIECES = 6,       /* operand planes of the split kernels: 3 bf16x6, 2 f16x3, 1 bf16; 0 exact fp32 */
  XAS_PLAN_PATCH_WIDTH = 7,  /* igemm_x6t_kernel: 16 (8 x 16 patches of one image) or 8 (8 x 8 of two images) */
  XAS_PLAN_TPB = 8,          /* igemm_x6p_kernel: consecutive M-tiles per block */
  XAS_PLAN_IMAGES = 9,       /* images per launch (< N: the call runs as several launches over image ranges) */
  XAS_PLAN_INTS = 10
};
enum { XAS_ROUTE_STEM_F16 = 1, XAS_ROUTE_STEM_F32 = 2, XAS_ROUTE_THIN_VEC_TO_SCALAR = 3, XAS_ROUTE_THIN_SCALAR_TO_VEC = 4,
       XAS_ROUTE_DIRECT = 5, XAS_ROUTE_MFMA = 6 };
enum { XAS_KERNEL_IGEMM_BUF = 1, XAS_KERNEL_IGEMM = 2, XAS_KERNEL_IGEMM_X6 = 3, XAS_KERNEL_IGEMM_X6T = 4, XAS_KERNEL_IGEMM_X6P = 5 };
int xas_conv_igemm_plan(const xas_conv_shape* s, int pass, int has_bias, int* out);
/* dw_packed [Cout][R][S][Cin] (+)= sum_n,ho,wo dy * x ; workspace for split-K partials. */
size_t xas_conv_wgrad_workspace_floats(const xas_conv_shape* s);
int xas_conv_wgrad(const float* x, const float* dy, float* dw_packed, float* workspace,
                   const xas_conv_shape* s, void* stream);
/* same, but the split slabs are summed straight into the parameter's OIHW layout [Cout][Cin][R][S] */
int xas_conv_wgrad_oihw(const float* x, const float* dy, float* dw_oihw, float* workspace,
                        const xas_conv_shape* s, void* stream);
/* same, ACCUMULATING: dw_oihw += gradient (used to add straight into the parameter's .grad arena) */
int xas_conv_wgrad_acc(const float* x, const float* dy, float* dw_oihw, float* workspace,
                       const xas_conv_shape* s, void* stream);
/* OIHW [Cout][Cin][R][S] <-> packed.  transposed=0: [Cout][R][S][Cin];
 * transposed=1: [Cin][R][S][Cout].  unpack adds nothing: it overwrites dst. */
int xas_pack_weight(const float* oihw, float* packed, int Cout, int Cin, int R, int S,
                    int transposed, void* stream);
int xas_unpack_weight(const float* packed, float* oihw, int Cout, int Cin, int R, int S,
                      int transposed, void* stream);

/* ------------------------------------------------------------------------------------
 * Batch normalisation (training mode), activation, residual; NHWC, M = N*H*W rows.
 * Replaces ATen batch_norm_stats / batch_norm_elemt / batch_norm_backward_{reduce,elemt}
 * behind nn.BatchNorm2d and nn.SyncBatchNorm (resnet.py:18,40, deconv_head.py:30,
 * physique_network.py:18,25,33).
 * GROUPS.  The M rows may be `groups` independent batches of M / groups consecutive rows, each normalised with
 * its own statistics: the camera-batched step sends the images of all cameras through the detector as one
 * tensor while every camera keeps its own batch statistics and its own running-statistic update, exactly as
 * the reference's per-camera calls (model.py:64,147,231).  Statistics are [groups][C]; groups = 1 is the plain
 * layer.  Running statistics receive one update per group, in group order.
 * stats step : slab partials (sums around a pivot row) are combined by the LAST-ARRIVING block of the same
 * launch (ticket counter, fixed summation order: deterministic), no separate finalize launch.
 * The host may all-gather (mean | var | count) across ranks between the two steps for SyncBatchNorm (one
 * coalesced message per layer for all groups) and merge with xas_bn_sync_merge.
 * act: 0 none, 1 relu, 2 leaky-relu(0.01).
 * ---------------------------------------------------------------------------------- */
size_t xas_bn_workspace_floats(long M, int C, int groups);
/* mean[g*out_stride + c], var_biased[g*out_stride + c] (out_stride >= C, multiple of 4 floats; C for dense [G][C]).
 * count_out != NULL: count_out[g*out_stride] = M / groups as float (the count slot of a packed SyncBatchNorm
 * message [mean | var | count]: pass mean = msg, var = msg + C, count_out = msg + 2C, out_stride = 2C + 4).
 * running_mean/var != NULL (rank-local norms): the running-statistic updates (momentum, unbiased variance
 * from `count`) are applied in the same launch; pass NULL for SyncBatchNorm (xas_bn_sync_merge updates them). */
int xas_bn_stats(const float* x, long M, int C, int groups, float* mean, float* var_biased, long out_stride,
                 float* count_out, float* workspace, float* running_mean, float* running_var, float momentum,
                 long count, void* stream);
/* Statistics from per-tile partial sums: partial is a [rows][C][2] matrix, (sum(v - pivot), sum((v - pivot)^2)) of
 * rows_per_group / (rows / groups) consecutive activation rows each, the first rows / groups partial rows belonging to
 * group 0 and so on; pivot [C] or NULL (= 0).  Outputs and running-statistic update as xas_bn_stats.
 * workspace: xas_bn_workspace_floats(rows, 2 * C, groups). */
int xas_bn_stats_from_partials(const float* partial, long rows, int C, int groups, long rows_per_group,
                               const float* pivot, float* mean, float* var_biased, long out_stride, float* count_out,
                               float* workspace, float* running_mean, float* running_var, float momentum, void* stream);
/* Batch-norm backward sums from per-tile partial sums: partial [rows][2][C] (sum dz | sum dz * xhat of the activation rows
 * behind each partial row; the first rows / groups partial rows belong to group 0, ...) -> sums [groups][2][C]; the local
 * parameter gradients are added into dbeta_acc / dgamma_acc (both or neither).  workspace:
 * xas_bn_workspace_floats(rows, 2 * C, groups). */
int xas_bn_bwd_sums_from_partials(const float* partial, long rows, int C, int groups, float* sums, float* workspace,
                                  float* dbeta_acc, float* dgamma_acc, void* stream);
/* SyncBatchNorm merge (torch/nn/modules/_functions.py SyncBatchNorm.forward: batch_norm_gather_stats_with_counts):
 * gathered [world][groups][msg_stride] with mean at +0, biased var at +C, count at +2C of each message;
 * count-weighted merge in double -> mean, var_biased [groups][C]; running statistics (may be NULL) updated once per
 * group in group order with the global count. */
int xas_bn_sync_merge(const float* gathered, int world, int groups, int C, long msg_stride, float* mean,
                      float* var_biased, float* running_mean, float* running_var, float momentum, void* stream);
/* out[c] = sum_m x[m][c]  (bias gradients: deconv_head.py:34, physique_network.py:17, discriminator.py:11);
 * workspace: xas_bn_workspace_floats(M, C, 1) */
int xas_col_sum(const float* x, long M, int C, float* out, float* workspace, void* stream);
/* acc[c] += column sums (bias gradients accumulated in place: nn.Conv2d / nn.Linear bias, physique_network.py:16,
 * discriminator.py:23).  workspace as xas_col_sum. */
int xas_col_sum_acc(const float* x, long M, int C, float* acc, float* workspace, void* stream);
/* y = act(gamma*(x-mean_g)*rsqrt(var_g+eps)+beta [+ residual]); mean / var_biased: [groups][C].
 * mask_out (may be NULL): [M*C/4] bytes, bit e of byte i = (pre-activation value of element 4i+e > 0): all the backward
 * needs of y for a layer with a residual, at 1/16 of y's bytes. */
int xas_bn_apply(const float* x, const float* mean, const float* var_biased, const float* gamma,
                 const float* beta, const float* residual, float eps, int act, long M, int C, int groups,
                 float* y, uint8_t* mask_out, void* stream);
/* Same, and max |y| over the whole result is merged into the amax slot amax_out (XAS_AMAX_SLOT_FLOATS floats, zeroed by the
 * caller; atomic maximum on the bit pattern): the scale of y as the input of the next convolution's f16x3 launches (xas_conv_shape.grad_amax; x_amax of
 * its weight gradient).  amax_out == NULL: xas_bn_apply. */
int xas_bn_apply_amax(const float* x, const float* mean, const float* var_biased, const float* gamma,
                      const float* beta, const float* residual, float eps, int act, long M, int C, int groups,
                      float* y, uint8_t* mask_out, float* amax_out, void* stream);
/* max |x| over n floats merged into the amax slot amax_out (as above): for convolution inputs that no kernel of this library wrote
 * (images, rendered masks).  One streaming read. */
int xas_abs_max(const float* x, long n, float* amax_out, void* stream);
/* running = (1-momentum)*running + momentum*stat_g for g = 0..groups-1; var uses the unbiased estimate n/(n-1). */
int xas_bn_update_running(const float* mean, const float* var_biased, float* running_mean,
                          float* running_var, float momentum, long count, int C, int groups, void* stream);
/* backward, step 1: dz = dy * act'(y); sums[g][0][c] = sum_dz, sums[g][1][c] = sum_dz_xhat  ([groups][2][C]).
 * x may be NULL when the layer has an activation and no residual: xhat is then recovered from the saved output,
 * xhat = (act^-1(y) - beta) / gamma (needed only where dz != 0), one activation tensor less to read per pass.
 * A channel with gamma == 0 has no recoverable xhat: its sum_dz_xhat is 0 (sum_dz is right, nothing is non-finite).
 * y may be NULL instead (x, gamma, beta given, no residual): the activation mask is then re-derived from x with the
 * forward's exact arithmetic and the backward never reads y.
 * dbeta_acc / dgamma_acc (both or neither, may be NULL): the parameter gradients (sums over all groups) are ALSO
 * added into these [C] buffers (the .grad arena of the optimizer), which saves the autograd accumulation kernels. */
int xas_bn_bwd_reduce(const float* x, const float* y, const float* dy, const float* mean,
                      const float* var_biased, const float* gamma, const float* beta, float eps, int act,
                      long M, int C, int groups, float* sums, float* workspace,
                      float* dbeta_acc, float* dgamma_acc, const uint8_t* mask, void* stream);
/* mask (may be NULL): the sign bytes xas_bn_apply wrote; when given, y is not read (x required). */
/* step 2: dx = gamma*invstd_g*(dz - sum_dz_g/cnt - xhat*sum_dz_xhat_g/cnt); dres = dz if != NULL; cnt = rows per
 * group (x world size for SyncBatchNorm).  x may be NULL only for the leaky-ReLU layers (invertible activation). */
int xas_bn_bwd_apply(const float* x, const float* y, const float* dy, const float* mean,
                     const float* var_biased, const float* gamma, const float* beta, const float* sums,
                     float eps, int act, long M, int C, int groups, double count,
                     float* dx, float* dresidual, const uint8_t* mask, void* stream);
/* Same, and max |dx| over the whole result is merged into the amax slot amax_out (XAS_AMAX_SLOT_FLOATS device floats, zeroed
 * by the caller before the first launch that merges into it; atomic maximum on the bit pattern): the scale of dx as the gradient operand of the f16x3
 * data / weight gradients (xas_conv_shape.grad_amax).  amax_out == NULL: xas_bn_bwd_apply. */
int xas_bn_bwd_apply_amax(const float* x, const float* y, const float* dy, const float* mean,
                          const float* var_biased, const float* gamma, const float* beta, const float* sums,
                          float eps, int act, long M, int C, int groups, double count, float* dx,
                          float* dresidual, const uint8_t* mask, float* amax_out, void* stream);
/* Dual forms: the output of a bottleneck WITH a projection, out = relu(bn3(x) + bn_d(xd)) (torchvision Bottleneck with
 * `downsample`, resnet.py:2), as one pass per step over both norms.  x / xd [M][C]: the raw results of conv3 and of the
 * projection convolution; every argument with the suffix _d belongs to the projection norm, the others to bn3; both norms
 * share M, C and groups.  Neither the normalised skip bn_d(xd) nor its gradient is ever written; the values are
 * those of xas_bn_apply_amax (act 0) -> xas_bn_apply_amax (act 1, residual, mask_out) forward and of xas_bn_bwd_reduce /
 * xas_bn_bwd_apply_amax run for bn3 (mask, dresidual) and then for the projection norm on that dresidual, bit for bit
 * (the backward apply: where C / 4 is a power of two, the streaming kernels; elsewhere to rounding).
 * forward: y, the sign bytes mask_out (required) and max |y| (amax_out may be NULL). */
int xas_bn_apply_dual_amax(const float* x, const float* mean, const float* var_biased, const float* gamma,
                           const float* beta, float eps, const float* xd, const float* mean_d,
                           const float* var_biased_d, const float* gamma_d, const float* beta_d, float eps_d,
                           long M, int C, int groups, float* y, uint8_t* mask_out, float* amax_out, void* stream);
/* backward, step 1: dz = dy * relu'(mask); sums [groups][2][C] = sum dz | sum dz * xhat(x), sums_d the same with xhat(xd).
 * workspace: 2 * xas_bn_workspace_floats(M, C, groups) floats.  The accumulator pairs as xas_bn_bwd_reduce, one per norm. */
int xas_bn_bwd_reduce_dual(const float* x, const float* xd, const float* dy, const uint8_t* mask, const float* mean,
                           const float* var_biased, float eps, const float* mean_d, const float* var_biased_d,
                           float eps_d, long M, int C, int groups, float* sums, float* sums_d, float* workspace,
                           float* dbeta_acc, float* dgamma_acc, float* dbeta_d_acc, float* dgamma_d_acc, void* stream);
/* step 2: dx = gradient wrt x, dxd = gradient wrt xd, both from the one dz; max |dx| -> amax_out, max |dxd| -> amax_d_out
 * (each may be NULL).  count / count_d: rows per group of each norm (x world size where THAT norm is a SyncBatchNorm). */
int xas_bn_bwd_apply_dual_amax(const float* x, const float* xd, const float* dy, const uint8_t* mask,
                               const float* mean, const float* var_biased, const float* gamma, const float* sums,
                               float eps, const float* mean_d, const float* var_biased_d, const float* gamma_d,
                               const float* sums_d, float eps_d, long M, int C, int groups, double count,
                               double count_d, float* dx, float* dxd, float* amax_out, float* amax_d_out, void* stream);

/* 3x3 stride-2 pad-1 max pool (resnet.py:20), NHWC. idx: int8 argmax tap 0..8 for backward */
int xas_maxpool3x3s2_fwd(const float* x, int N, int H, int W, int C, float* y, int8_t* idx, void* stream);
int xas_maxpool3x3s2_bwd(const float* dy, const int8_t* idx, int N, int H, int W, int C, float* dx, void* stream);

/* bilinear x2 upsample, align_corners=False (physique_network.py:31), NHWC */
int xas_upsample2x_fwd(const float* x, int N, int H, int W, int C, float* y, void* stream);
int xas_upsample2x_bwd(const float* dy, int N, int H, int W, int C, float* dx, void* stream);

/* elementwise: y = sigmoid(x) ; dx = dy*y*(1-y) */
int xas_sigmoid_fwd(const float* x, long n, float* y, void* stream);
int xas_sigmoid_bwd(const float* y, const float* dy, long n, float* dx, void* stream);
/* NCHW -> NHWC and back (input images arrive NCHW: dataloader.py:166) */
int xas_nchw_to_nhwc(const float* x, int N, int C, int H, int W, float* y, void* stream);
int xas_nhwc_to_nchw(const float* x, int N, int C, int H, int W, float* y, void* stream);
/* Input of a flip-test pass (the mirrored image that the head of keypoint_detector_integral_multi.py:36-88 is averaged
 * over): x [B][C][H][W] -> y [2B][H][W][C], y[b] = x[b] and y[B + b][h][w] = x[b][h][W - 1 - w]; x is read once. */
int xas_nchw_to_nhwc_mirror_pair(const float* x, int B, int C, int H, int W, float* y, void* stream);

/* ------------------------------------------------------------------------------------
 * GPU input pipeline: the per-sample work of the reference's CPU loader
 * (human_utils/dataloader/dataloader.py:17-91,150-191; OpenCV + scikit-fmm) over a batch of decoded 8-bit images in HBM.
 * ---------------------------------------------------------------------------------- */
/* cv2.warpAffine(src_b, trans_b, (P, P), flags=INTER_LINEAR) with BORDER_CONSTANT 0 for every image of the batch
 * (common/imglib/affine.py:112, dataloader.py:58).  src: packed 8-bit images [H_b][W_b][C] at byte offsets src_off[b];
 * src_hw [B][2] = (H_b, W_b); minv [B][6] doubles = the INVERTED 2x3 transform (patch pixel -> source pixel), inverted on
 * the host as cv::warpAffine does; dst [B][P][P][C].  OpenCV's fixed-point arithmetic, bit-exact. */
int xas_warp_affine_u8(const uint8_t* src, const long* src_off, const int* src_hw, const double* minv, int B, int C,
                       int P, uint8_t* dst, void* stream);
/* cv2.GaussianBlur(mask, (5,5), 0) then cv2.threshold(127, 255, THRESH_BINARY) (MPI-INF-3DHP masks, dataloader.py:62-65);
 * mask, out: [B][P][P] 8-bit, out != mask */
int xas_mask_blur_threshold(const uint8_t* mask, int B, int P, uint8_t* out, void* stream);
/* convert_cvimg_to_tensor + colour scale / clip + (x - mean) / std + mask / 255 + rm_bg (dataloader.py:56,67-71,185-188):
 * img_bgr [B][P][P][3], mask [B][P][P] 8-bit -> out_img [B][3][P][P] RGB float, out_mask [B][1][P][P] float.
 * color_scale: device [B][3] (RGB order) or NULL; mean3 / std3: HOST pointers to 3 floats (RGB order). */
int xas_patch_finish(const uint8_t* img_bgr, const uint8_t* mask, const float* color_scale, const float* mean3,
                     const float* std3, int rm_bg, int B, int P, float* out_img, float* out_mask, void* stream);
/* compute_geodesic_dis (common/utility/geodesic.py:14-54): mask [B][P][P] float (non-zero = foreground);
 * centers: device [B][2] ints (x, y) or NULL (centroid of the mask, geodesic.py:4-12); params5: HOST pointer to
 * geodesic_param_list (5 floats, [4] must be 0); out [B][1][P][P]; center_out: device [B][2] ints or NULL.
 * Grid Eikonal solves by iterating the first-order upwind update to its fixed point (scikit-fmm: fast marching). */
size_t xas_geodesic_workspace_bytes(int B, int P);
int xas_geodesic_weight(const float* mask, const int* centers, const float* params5, int B, int P, float* out,
                        int* center_out, void* workspace, void* stream);
/* The general form: SEVERAL source pixels per image (geodesic_pt_list: the listed joints, dataloader.py:189-191) and the order
 * of the upwind scheme.  centers: device [B][num_centers][2] ints (x, y), 1 <= num_centers <= 64, or NULL with num_centers = 1
 * (centroid); every centre is a zero of the inside solve; if ANY centre of an image lies on the background that image's map is
 * all ones (geodesic.py:22-27).  order: 2 = the second-order scheme scikit-fmm's `distance` runs by default (one-sided
 * second-order differences where the second upwind neighbour is not larger, first order elsewhere; restated from the
 * library's documented algorithm, parity unpinned), 1 = first order (what xas_geodesic_weight computes).  center_out: device
 * [B][2] ints (first centre) or NULL.  Workspace as above. */
int xas_geodesic_weight_multi(const float* mask, const int* centers, int num_centers, int order, const float* params5, int B, int P,
                              float* out, int* center_out, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * Mask losses (modules/base_losses/loss_func.py:4-16), fused clip * weight * MSE.
 * mode bit0: use_clip (mask > 0.1), bit1: has weight.
 * out: 3 floats.
 *   weight given : out[0] = mean(e * clip * weight), out[1] = 1
 *   no weight    : out[0] = mean((m-gt)^2), out[1] = mean(clip)   (the reference returns the
 *                  tensor mse*clip; its later .mean() equals out[0]*out[1])
 *   out[2] = out[0]*out[1] = the scalar the trainer reduces to (train.py:182)
 * partial: workspace of xas_loss_nblk(n) * 2 floats.
 * bwd: dm = grad_scalar * d(out)/dm for the weighted form; for the unweighted+clip form
 *      dm = grad_scalar * out[1] * 2(m-gt)/n.
 * ---------------------------------------------------------------------------------- */
int xas_loss_nblk(long n);
int xas_mask_loss_fwd(const float* m, const float* gt, const float* weight, long n, int mode,
                      float* partial, float* out, void* stream);
int xas_mask_loss_bwd(const float* m, const float* gt, const float* weight, long n, int mode,
                      const float* out, const float* grad_scalar, float* dm, void* stream);

/* ------------------------------------------------------------------------------------
 * Joint-level losses as the model combines them (loss_func.py:18-76, model.py:98-164): a batch mean per
 * hypothesis, then the MIN over hypotheses; gradient flows to the winning hypothesis only.
 * pred [B][Hy][K][3].  kind 0: supervision vs gt [B][K][3] ; kind 1: w0*bone_sym + w1*kp_sym (3-D, mm*1e-3)
 * [+ w2 * kp_sym on the (x,y) of the patch joints passed as `gt` = kps [B][Hy][K][3], or NULL] ;
 * kind 2: w0 * kp_sym on (x,y).  out: 2+Hy floats = {min, argmin, v_0..v_{Hy-1}}.  grad_aux (kind 1 with the
 * 2-D term, else NULL): gradient w.r.t. the patch joints.
 * xas_lsgan_*: logits [B][Hy] -> out[0] = mean_b min_h (x - target)^2, idx[b] = argmin.
 * Both minima are NaN-faithful like torch.min: the first NaN among the candidates wins (value NaN, gradient NaN
 * there), else the first minimum.  On an exact tie the whole gradient goes to the first minimum (the reference's
 * full-reduction torch.min over the stacked hypothesis values would split it evenly among the tied ones).
 * ---------------------------------------------------------------------------------- */
int xas_pose_loss_fwd(const float* pred, const float* gt, int B, int Hy, int K, int kind, float w0, float w1,
                      float w2, float* out, void* stream);
int xas_pose_loss_bwd(const float* pred, const float* gt, int B, int Hy, int K, int kind, float w0, float w1,
                      float w2, const float* out, const float* grad_scalar, float* grad_pred, float* grad_aux,
                      void* stream);
int xas_lsgan_fwd(const float* logits, int B, int Hy, float target, float* out, int* idx, void* stream);
int xas_lsgan_bwd(const float* logits, int B, int Hy, float target, const int* idx, const float* grad_scalar,
                  float* grad_logits, void* stream);

/* ------------------------------------------------------------------------------------
 * GCN discriminator building blocks (discriminator.py:180-238, gcn.py:79-110 with
 * torch_geometric SAGEConv(mean) / graph LayerNorm semantics).  Node features [B*N][C].
 * ---------------------------------------------------------------------------------- */
/* y[b,i,:] = sum_j adj[i][j] * x[b,j,:]  (adj: N x N row-normalised, device) */
int xas_graph_aggregate(const float* x, const float* adj, int B, int N, int C, float* y, void* stream);
/* graph LayerNorm (normalise over the WHOLE [rows, C] tensor of one discriminator call) + per-channel
 * affine + relu (+ residual).  `groups` independent calls are batched: x is [groups*rows, C] and the
 * statistics are per group.  stats: [groups][2] = (mean, std).
 * workspace: xas_gln_workspace_floats(rows*C, groups, C) floats. */
size_t xas_gln_workspace_floats(long n, int groups, int C);
int xas_gln_fwd(const float* x, const float* gamma, const float* beta, const float* residual,
                long rows, int C, int groups, float eps, float* y, float* stats, float* workspace,
                void* stream);
/* backward of y = relu(ln(x)) (+ residual: pass-through handled by the caller); the relu mask is
 * recomputed from x, gamma, beta; dgamma / dbeta are summed over the groups. */
int xas_gln_bwd(const float* x, const float* beta, const float* dy, const float* gamma,
                const float* stats, long rows, int C, int groups, float eps, float* dx, float* dgamma,
                float* dbeta, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * SMPL linear blend skinning (modules/smplpytorch/pytorch/smpl_layer.py:63-156).
 * ---------------------------------------------------------------------------------- */
int xas_smpl_lbs_fwd(const float* pose /*[B][72]*/, const float* betas /*[B][10]*/,
                     const float* v_template /*[V][3]*/, const float* shapedirs /*[V][3][10]*/,
                     const float* posedirs /*[V][3][207]*/, const float* j_regressor /*[24][V]*/,
                     const float* weights /*[V][24]*/, const int* parents /*[24]*/, int B, int V,
                     int center_idx, float* verts /*[B][V][3]*/, float* joints /*[B][24][3]*/,
                     float* workspace /* B*(24*3 + 24*16 + 207) floats */, void* stream);

/* Backward of xas_smpl_lbs_fwd (autograd of smpl_layer.py:63-156): d_verts [B][V][3], d_joints [B][24][3] (or NULL)
 * -> d_pose [B][72], d_betas [B][10].  fwd_workspace: the workspace the forward call filled for the same inputs.
 * workspace: xas_smpl_lbs_bwd_workspace_floats(B, V).  Deterministic (no atomics). */
size_t xas_smpl_lbs_bwd_workspace_floats(int B, int V);
int xas_smpl_lbs_bwd(const float* pose, const float* betas, const float* v_template, const float* shapedirs,
                     const float* posedirs, const float* j_regressor, const float* weights, const int* parents, int B,
                     int V, int center_idx, const float* fwd_workspace, const float* d_verts, const float* d_joints,
                     float* d_pose, float* d_betas, float* workspace, void* stream);

/* SMPL parameters from the 18 H36M joints of a sample (eval.py --fit-smpl; the reference has no counterpart): the inverse of
 * project_smpl_to_patch_kps' model.  The layer runs with a zero root rotation:
 *   verts = xas_smpl_lbs_fwd((0, 0, 0, theta), beta)[center_idx];   j = smpl_to_h36m(verts, h36m_regressor), 18 joints, root
 *   centred (17 regressed rows, arms exchanged, joint 17 = (j_11 + j_14) / 2, minus joint 0);   Y_k = R(omega) (1000 j_k) + t.
 * The 23 body rotations are the layer's rodrigues (unit quaternion of angle |a + 1e-8|); R(omega) is the plain exponential map
 * I + sin(th) K + (1 - cos(th)) K^2, K the cross matrix of omega / th, th = |omega| (xas_amd.pseudo._rodrigues: pose[:, :3] =
 * omega is what PseudoSynth reads); for th^2 < 1e-16 its series I + K(omega) + K(omega)^2 / 2, so the derivative exists at 0.
 * UNKNOWNS x [85]: omega 3, t 3 (mm), theta 69, beta 10.  Inputs are fp32; everything after the loads is double.
 * RESIDUALS r [133], in this order: 54 joint rows sqrt(w_k) (Y_k - target_k) in mm, row 3 k + c; 69 rows sqrt(pose_prior)
 * theta_i; 10 rows sqrt(shape_prior) beta_i.  A joint is USED if w_k > 0 (NaN and negative weights count as 0); a joint not
 * used has r = 0 and a zero row of J exactly, and its target is never read into arithmetic.  COST C = sum of r_i^2, i ascending.
 * targets [B][18][3] world mm, joint_w [B][18], pose_prior, shape_prior >= 0 finite.  parents [24] int32 on the device (an entry
 * that is not in [0, i) makes joint i a root).  center_idx: the layer's, -1 = none.
 * h36m_regressor [17][V] dense.  reg_verts [V] int32 + reg_count (one int32), both on the device: the vertices that have a
 * non-zero column come first in reg_verts and reg_count says how many; only those are visited, an index outside [0, V) is
 * skipped.  Both NULL = every vertex.  The result does not depend on the list as long as it holds every non-zero column.
 * xas_smpl_fit_linearise: r [B][133] and J = d r / d x [B][133][85] (double) at the given parameters, the exact derivative
 * (forward mode through the Rodrigues formula, the pose blend shapes, the betas' effect on the rest joints, the chain and the
 * skinning).
 * xas_smpl_fit: Levenberg-Marquardt from the given parameters.  H = J^T J, g = J^T r.  A TRIAL is x + d with
 * (H + lambda diag(H)) d = -g by Cholesky, lambda = 1e-3 at the start.  A trial is ACCEPTED if its cost is finite and strictly
 * lower: x moves, lambda *= 0.1, and the fit has CONVERGED if the largest |d_i| of that step is under XAS_SMPLFIT_STEP_TOL
 * (radians, mm and betas alike); otherwise, and at a pivot that is not positive, lambda *= 10.  The loop ends when converged,
 * after max_iters trials (0 <= max_iters <= XAS_SMPLFIT_MAX_ITERS) or when lambda > 1e12.  So cost[1] <= cost[0], always.
 * PASSED THROUGH: fewer than 6 joints used, or the cost at the given parameters is not finite.
 * Outputs, every element written by every call (double unless noted): pose [B][72] = (omega, theta), betas [B][10], trans
 * [B][3], joints [B][18][3] = Y at the result, cost [B][2] = C at the start and at the result, iters [B] int32 = trials made,
 * status [B] bytes: 0 converged, 1 ran out of trials or lambda, 2 passed through (parameters = the inputs exactly, joints = Y
 * there, cost[1] = cost[0], iters = 0).
 * workspace: xas_smpl_fit_workspace_bytes(B, V) bytes, 16-byte aligned.  V >= 1 any size; B == 0 writes nothing.
 * One workgroup of 256 threads per sample and the whole LM in one launch (plus one launch that forms j_regressor . v_template
 * and j_regressor . shapedirs); no atomics, no host synchronisation: a pure function of the inputs bit for bit, per sample. */
#define XAS_SMPLFIT_UNKNOWNS 85
#define XAS_SMPLFIT_RESIDUALS 133
#define XAS_SMPLFIT_MAX_ITERS 200
#define XAS_SMPLFIT_STEP_TOL 1e-7
size_t xas_smpl_fit_workspace_bytes(int B, int V);
int xas_smpl_fit_linearise(const float* pose, const float* betas, const float* trans, const float* v_template,
                           const float* shapedirs, const float* posedirs, const float* j_regressor, const float* weights,
                           const int* parents, const float* h36m_regressor, const int* reg_verts, const int* reg_count,
                           const float* targets, const float* joint_w, float pose_prior, float shape_prior, int B, int V,
                           int center_idx, double* r, double* J, void* workspace, void* stream);
int xas_smpl_fit(const float* pose, const float* betas, const float* trans, const float* v_template, const float* shapedirs,
                 const float* posedirs, const float* j_regressor, const float* weights, const int* parents,
                 const float* h36m_regressor, const int* reg_verts, const int* reg_count, const float* targets,
                 const float* joint_w, float pose_prior, float shape_prior, int B, int V, int center_idx, int max_iters,
                 double* pose_out, double* betas_out, double* trans_out, double* joints_out, double* cost, int* iters,
                 unsigned char* status, void* workspace, void* stream);

/* xas_smpl_fit with the DATA TERM IN PIXELS, per camera (eval.py --fit-smpl --fit-data reproj; the reference has no counterpart).
 * The model, the unknowns x [85], the init (pose, betas, trans), the model arrays, parents, h36m_regressor, reg_verts, reg_count,
 * center_idx and the priors mean what they mean for xas_smpl_fit; there are no targets and no joint weights.  Instead a model
 * joint Y_k(x) is held to what was measured:
 *   points [B][C][18][3] fp32 = (u, v, weight) and P [B][C][3][4] fp32, xas_triangulate_refine's layout and meaning, 1 <= C <=
 *   XAS_TRI_MAX_VIEWS; views [B][18] bytes or NULL; flags = 0 or XAS_REFINE_WEIGHTED; huber >= 0 finite (0 = squared);
 *   anchor [B][18][3] fp32 mm and info [B][18][6] fp32 (xx xy xz yy yz zz), xas_track_anchor_smooth's, both NULL or both given;
 *   anchor_huber >= 0 finite.
 * WHICH OBSERVATIONS COUNT is decided once, at the init, and fixed for the whole fit.  View v counts for joint k if its weight
 * is VALID (finite, > 0), it is in the joint's `views` byte (a zero byte, or views = NULL, stands for all valid views), u and v
 * are finite and Y_k(init) lies in front of it (h_2 <= 0 is behind, as everywhere); a view behind the start is dropped for that
 * joint.  An anchor counts if it is USABLE by xas_track_anchor_smooth's rule.  A joint is USED if it has at least one view or
 * an anchor; a joint that is not used never reads its pixels, anchor or information into arithmetic (NaN there is legal).
 * used [B][18] bytes, written by every call: the mask of the joint's views | 0x80 if it has an anchor.
 * COST C(x), in px^2 (sigma^2 under XAS_REFINE_WEIGHTED), in double from the fp32 inputs: for the joints k ascending, at Y_k(x),
 * xas_triangulate_refine's term over the joint's views ascending (the same scale rule, the same Huber loss) and then
 * xas_track_anchor_smooth's anchor term (Huber anchor_huber of sqrt(max(e^T W e, 0))); then pose_prior theta_i^2, i ascending,
 * and shape_prior beta_i^2, as xas_smpl_fit sums them.  Per joint the data reduce to a cost c_k, a 3x3 Gauss-Newton block A_k
 * (the IRLS blocks w (ju ju^T + jv jv^T) of the views plus psi W of the anchor) and a gradient b_k; with Jy_k = dY_k / dx:
 *   H = sum_k Jy_k^T A_k Jy_k + priors,   g = sum_k Jy_k^T b_k + priors   (k ascending; the priors as xas_smpl_fit's).
 * xas_smpl_fit_views_linearise, at the init: H [B][85][85] full and symmetric in bits, undamped, priors in; g [B][85]; cost [B];
 * joint_blocks [B][18][9] = A_k (xx xy xz yy yz zz) and b_k, zero for a joint not used; used.  No sample is passed through here.
 * xas_smpl_fit_views: xas_smpl_fit's Levenberg-Marquardt rule for rule (lambda = 1e-3, damping lambda diag(H), x10 / x0.1,
 * XAS_SMPLFIT_STEP_TOL, lambda > 1e12, 0 <= max_iters <= XAS_SMPLFIT_MAX_ITERS, the status codes, cost[1] <= cost[0]), with one
 * addition: a trial that puts a used joint behind one of its views is rejected.  PASSED THROUGH by xas_smpl_fit's rule: fewer
 * than 6 joints used, or a cost at the init that is not finite; the outputs then follow xas_smpl_fit's pass-through contract.
 * Outputs: xas_smpl_fit's (pose, betas, trans, joints, cost [B][2], iters, status), and used.
 * workspace: xas_smpl_fit_views_workspace_bytes(B, V) bytes, 16-byte aligned (xas_smpl_fit's layout; the joint blocks live in
 * LDS).  B == 0 writes nothing.  One workgroup of 256 threads per sample and the whole LM in one launch, plus the joint-term
 * launch; no atomics, no host synchronisation: a pure function of the inputs bit for bit, per sample, whatever the workspace held. */
size_t xas_smpl_fit_views_workspace_bytes(int B, int V);
int xas_smpl_fit_views_linearise(const float* pose, const float* betas, const float* trans, const float* v_template,
                                 const float* shapedirs, const float* posedirs, const float* j_regressor, const float* weights,
                                 const int* parents, const float* h36m_regressor, const int* reg_verts, const int* reg_count,
                                 const float* points, const float* P, const unsigned char* views, const float* anchor,
                                 const float* info, int flags, double huber, double anchor_huber, float pose_prior,
                                 float shape_prior, int B, int V, int C, int center_idx, double* H, double* g, double* cost,
                                 double* joint_blocks, unsigned char* used, void* workspace, void* stream);
int xas_smpl_fit_views(const float* pose, const float* betas, const float* trans, const float* v_template, const float* shapedirs,
                       const float* posedirs, const float* j_regressor, const float* weights, const int* parents,
                       const float* h36m_regressor, const int* reg_verts, const int* reg_count, const float* points,
                       const float* P, const unsigned char* views, const float* anchor, const float* info, int flags,
                       double huber, double anchor_huber, float pose_prior, float shape_prior, int B, int V, int C,
                       int center_idx, int max_iters, double* pose_out, double* betas_out, double* trans_out, double* joints_out,
                       double* cost, int* iters, unsigned char* status, unsigned char* used, void* workspace, void* stream);

/* xas_smpl_fit over whole tracks (eval.py --fit-smpl --fit-shape track): ONE beta vector per track, pose and translation per
 * frame.  The model arrays, targets, weights, priors and the init (pose, betas, trans: [N][72], [N][10], [N][3]) mean what they
 * mean above.  track [N] int32 in [0, S) and frame [N] int32 (device) say which track a sample belongs to and where it stands
 * in it; the samples may lie in any order in N.  A frame is USABLE by xas_smpl_fit's rule at its own init (>= 6 joints used and
 * a finite cost there) if its track id is in [0, S); any other frame is PASSED THROUGH: it leaves as its init (pose, trans,
 * joints = Y there, frame_cost = that cost twice, frame_status 2) and adds nothing to any track.
 * UNKNOWNS of track s with usable frames F_s: y_t [75] = omega 3, t 3, theta 69 for every t in F_s, and beta_s [10].
 * COST C_s = sum over t in F_s, ascending frame (a frame held twice: ascending sample index), of c(y_t, beta_s), c the COST above
 * term for term, so the shape prior counts once per usable frame.  START: y_t from the init; beta_s the mean of the init betas
 * over F_s, summed in that order in double.  A track of one frame is xas_smpl_fit's problem, and is solved bit for bit alike.
 * SOLVER: one Levenberg-Marquardt per track with xas_smpl_fit's schedule: lambda = 1e-3, damping lambda diag(H) on every diagonal
 * entry, a trial ACCEPTED if C_s at the trial is finite and strictly lower (lambda *= 0.1, CONVERGED if the largest |d| over all
 * unknowns of the track is under XAS_SMPLFIT_STEP_TOL), otherwise and at a pivot that is not positive lambda *= 10; ends when
 * converged, after max_iters trials or when lambda > 1e12.  So track_cost[1] <= track_cost[0], always.  The arrowhead system is
 * solved by eliminating every frame's 75 unknowns (Cholesky of the frame's damped 85 x 85 matrix stopped after column 75) and
 * summing the 10 x 10 Schur complements and reduced right-hand sides over F_s in the order above; no atomics.
 * Outputs (double unless noted), every element written by every call: pose [N][72], trans [N][3], joints [N][18][3], frame_cost
 * [N][2] = c at the track's start and at the result, frame_status [N] bytes (0 fitted, 2 passed through); track_betas [S][10]
 * (a track without usable frame: the plain mean of the init betas of its samples in the order above, zeros if it has none),
 * track_cost [S][2] = C_s at the start and at the result, track_trials [S] int32, track_status [S] bytes: 0 converged, 1 ran out
 * of trials or lambda, 2 no usable frame.
 * xas_smpl_fit_tracks_linearise: one trial at the given lambda >= 0 from the start: reduced [S][10][10] = the summed, damped
 * Schur complement, rhs [S][10] with reduced . d_beta = rhs, the trial step d_y [N][75] (zeros for a frame passed through) and
 * d_beta [S][10], track_cost [S] = C_s at the start.  A track without usable frame gives zeros; so does a track with a pivot
 * that is not positive: in a frame's elimination the system and the step, in the reduced system the step.
 * Argument errors return 1 before any launch; a track id outside [0, S) is one if `track` is host-visible memory (then it is read
 * on the host), otherwise that frame is passed through.  N == 0 or S == 0 are valid.
 * workspace: xas_smpl_fit_tracks_workspace_bytes(N, V, S) bytes, 16-byte aligned: the vertex-sized scratch exists once per
 * workgroup of a bounded grid (min(N, 512) workgroups that stride over the frames), 61 936 bytes of state per frame whatever V.
 * Set-up cost: a track's samples are found by one workgroup in a pass over N and ordered by ranking each against the others
 * (T^2 comparisons for a track of T samples, nothing beside the trials at T = 256, not meant for one track of 1e5 frames).
 * 5 launches to start, 4 per trial, all max_iters trials enqueued up front (a finished track does nothing in the later ones), no
 * host synchronisation: a pure function of the inputs bit for bit, per track, whatever the order of the samples in N. */
size_t xas_smpl_fit_tracks_workspace_bytes(int N, int V, int S);
int xas_smpl_fit_tracks_linearise(const float* pose, const float* betas, const float* trans, const float* v_template,
                                  const float* shapedirs, const float* posedirs, const float* j_regressor, const float* weights,
                                  const int* parents, const float* h36m_regressor, const int* reg_verts, const int* reg_count,
                                  const float* targets, const float* joint_w, const int* track, const int* frame,
                                  float pose_prior, float shape_prior, int N, int V, int S, int center_idx, double lambda,
                                  double* reduced, double* rhs, double* d_y, double* d_beta, double* track_cost, void* workspace,
                                  void* stream);
int xas_smpl_fit_tracks(const float* pose, const float* betas, const float* trans, const float* v_template,
                        const float* shapedirs, const float* posedirs, const float* j_regressor, const float* weights,
                        const int* parents, const float* h36m_regressor, const int* reg_verts, const int* reg_count,
                        const float* targets, const float* joint_w, const int* track, const int* frame, float pose_prior,
                        float shape_prior, int N, int V, int S, int center_idx, int max_iters, double* pose_out,
                        double* trans_out, double* joints_out, double* frame_cost, unsigned char* frame_status,
                        double* track_betas, double* track_cost, int* track_trials, unsigned char* track_status, void* workspace,
                        void* stream);

/* xas_smpl_fit_tracks with an ACCELERATION PRIOR on pose and translation over the frames of a track (eval.py --fit-smpl --fit-shape
 * track --fit-smooth).  Arguments, usable frames, start, outputs and limits are xas_smpl_fit_tracks', plus rot_w, trans_w >= 0,
 * finite.  With both 0 the problem is xas_smpl_fit_tracks' (solved by another elimination order: equal within rounding, not in bits).
 * COST of track s, its usable frames in xas_smpl_fit_tracks' order i = 0 .. T-1 with frame numbers f_i:
 *   C_s = sum_i c(y_i, beta_s) + sum_{i=1..T-2} ws_i sum_{c<75} w_c (cm_i y_i-1,c + c0_i y_i,c + cp_i y_i+1,c)^2
 * c as above; (cm, c0, cp, ws) the smoothers' stencil on the frame numbers (csrc/track_stencil.h: cm = 1 / (f_i - f_i-1), cp =
 * 1 / (f_i+1 - f_i), c0 = -(cm + cp), ws = 2 / (f_i+1 - f_i-1)); w_c = rot_w for the 72 angles (omega at 0..2, theta at 6..74),
 * trans_w for t at 3..5.  The squared residuals enter H = J^T J, g = J^T r and C like every other row, so the weights are mm^2 per
 * rad^2 (per mm^2) per frame^-3 against the joint rows' mm^2; the rows are linear, their Gauss-Newton block is exact.  A track
 * with fewer than three usable frames has no prior.  The prior acts on parameters: a difference of axis-angle vectors is not a
 * geodesic distance.
 * EQUAL FRAME NUMBERS: when rot_w + trans_w > 0, a usable frame whose frame number equals that of the usable frame before it in the
 * track's order is PASSED THROUGH (frame_status 2, its init): the stencil would divide by zero.
 * UNWRAPPING: omega and omega + 2 pi k omega / |omega| are one rotation but far apart for the prior.  When rot_w > 0 the set-up
 * replaces, in track order, the root omega of each usable frame i >= 1 by the equivalent vector nearest the previous, already
 * unwrapped, frame's: k = nearbyint((u . omega_i-1 - |omega_i|) / (2 pi)), u = omega_i / |omega_i|; |omega_i| = 0 is left alone.
 * Output `pose` holds the unwrapped vectors.  The body pose is NOT unwrapped: its prior keeps it near 0.
 * SOLVER: one Levenberg-Marquardt per track with xas_smpl_fit's schedule (lambda, damping lambda diag(H) with H including the
 * prior's diagonal, acceptance, stop and status rules), so track_cost[1] <= track_cost[0], always.  The damped system is block-
 * pentadiagonal (75 x 75 blocks; the off-diagonal blocks are hoff times diag(w)) with a 10-row border and a 10 x 10 corner.  A
 * trial: frame kernels on xas_smpl_fit_tracks' bounded grid assemble H_i, g_i after an accepted trial and evaluate the data cost
 * at the trial point; ONE WORKGROUP PER TRACK runs the block Cholesky in frame order (L_ii, L_i,i-1, L_i,i-2, the border row
 * L_beta,i filled from both predecessors, the corner last), both substitutions, the prior's cost at the trial point and the
 * decision.  6 launches to start, 4 per trial, all enqueued up front; no atomics, no host synchronisation, every sum in one
 * order: a pure function of the inputs bit for bit, per track, whatever the order of the samples in N and the workspace's contents.
 * Outputs: xas_smpl_fit_tracks'.  frame_cost [N][2] holds the DATA cost c of the frame alone, track_cost [S][2] the whole C_s
 * with the prior: the frame costs of a track no longer sum to its track cost.
 * xas_smpl_fit_tracks_smooth_linearise: one trial at the given lambda >= 0 from the (unwrapped) start.  Per sample: hdiag [N][75][75]
 * the damped diagonal block of the body; hoff [N][2] with H_i,i-1 = hoff[.][0] diag(w) and H_i,i-2 = hoff[.][1] diag(w) towards the
 * one and two usable frames before it in the track; border [N][10][75]; g_y [N][75] the gradient, prior included; d_y [N][75] the
 * trial step.  Per track: corner [S][10][10] summed and damped; g_beta [S][10]; d_beta [S][10]; track_cost [S] = C_s at the start.
 * The system solved is (blocks) d = -(g_y, g_beta).  Zeros for a frame passed through and a track without usable frame; zeros for
 * the steps at a pivot that is not positive.
 * workspace: xas_smpl_fit_tracks_smooth_workspace_bytes(N, V, S) bytes, 16-byte aligned: xas_smpl_fit_tracks' (61 936 bytes per
 * frame) plus 98 432 bytes per frame for the factor's block row (L_ii packed, L_i,i-1, L_i,i-2 packed, the border row, the
 * forward-substituted vector, the prior's diagonal and the gradient): 160 368 bytes per frame, about 330 MB for 2048 frames. */
size_t xas_smpl_fit_tracks_smooth_workspace_bytes(int N, int V, int S);
int xas_smpl_fit_tracks_smooth_linearise(const float* pose, const float* betas, const float* trans, const float* v_template,
                                         const float* shapedirs, const float* posedirs, const float* j_regressor,
                                         const float* weights, const int* parents, const float* h36m_regressor,
                                         const int* reg_verts, const int* reg_count, const float* targets, const float* joint_w,
                                         const int* track, const int* frame, float pose_prior, float shape_prior, double rot_w,
                                         double trans_w, int N, int V, int S, int center_idx, double lambda, double* hdiag,
                                         double* hoff, double* corner, double* border, double* g_y, double* g_beta, double* d_y,
                                         double* d_beta, double* track_cost, void* workspace, void* stream);
int xas_smpl_fit_tracks_smooth(const float* pose, const float* betas, const float* trans, const float* v_template,
                               const float* shapedirs, const float* posedirs, const float* j_regressor, const float* weights,
                               const int* parents, const float* h36m_regressor, const int* reg_verts, const int* reg_count,
                               const float* targets, const float* joint_w, const int* track, const int* frame, float pose_prior,
                               float shape_prior, double rot_w, double trans_w, int N, int V, int S, int center_idx,
                               int max_iters, double* pose_out, double* trans_out, double* joints_out, double* frame_cost,
                               unsigned char* frame_status, double* track_betas, double* track_cost, int* track_trials,
                               unsigned char* track_status, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused multi-tensor Adam (train.py:257-264: betas (0.5, 0.999), eps 1e-8, no decay).
 * One launch updates a flat parameter arena: p, g, m, v are arenas of n floats.
 * ---------------------------------------------------------------------------------- */
int xas_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                  float beta2, float eps, int step, void* stream);

/* Guarded step: gradient norm, clipping and non-finite skip on the device, no host round trip.
 *   xas_grad_guard         one read of the gradient arena -> its L2 norm (every sum in double, fixed order, no atomics: a
 *                          pure function of the arena's contents) and the decision for the step, in the guard record;
 *   xas_adam_step_guarded  xas_adam_step on g * scale, with scale, the bias corrections and the decision taken from the
 *                          record.  A skipped step writes nothing: p, m, v keep their bits.
 * Guard record: XAS_GUARD_FLOATS 4-byte words in device memory, zeroed by the caller before the first step, then owned by
 * these two calls (`t` and `skipped` persist from call to call):
 *   word 0  float norm          L2 norm of g, rounded once from double
 *   word 1  float scale         min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_); exactly 1.0f when
 *                               clipping is off (max_norm <= 0 or infinite)
 *   word 2  int   skip          1 when skip_nonfinite != 0 and an element of g, or the norm, is not finite
 *   word 3  int   t             steps APPLIED so far, this one included; a skipped step leaves it alone, so the bias
 *                               corrections continue as if that step() had never been called
 *   word 4  int   skipped       steps skipped so far
 *   word 5  float step_size     lr / (1 - beta1^t)         } computed in double from the device's own t
 *   word 6  float inv_sqrt_bc2  1 / sqrt(1 - beta2^t)      }
 *   word 7  int   nonfinite     1 when an element of g is not finite (whether or not skipping was asked for)
 * workspace: xas_grad_guard_workspace_bytes(n) bytes, 8-byte aligned.  n % 4 == 0, g 16-byte aligned. */
#define XAS_GUARD_FLOATS 8
size_t xas_grad_guard_workspace_bytes(long n);
int xas_grad_guard(const float* g, long n, float max_norm, int skip_nonfinite, float lr, float beta1, float beta2,
                   void* guard, void* workspace, void* stream);
int xas_adam_step_guarded(float* p, const float* g, float* m, float* v, long n, float beta1, float beta2, float eps,
                          const void* guard, void* stream);

/* Averaged weights: the same two steps, each also maintaining `ema`, an exponential moving average of the parameters (a
 * shadow arena of n floats, aligned like p), in the same launch - one more arena read and one more arena write.
 *   p, m, v   exactly what xas_adam_step / xas_adam_step_guarded compute from the same inputs, bit for bit;
 *   ema       per element, from the NEW parameter: ema = fmaf(decay, ema, one_minus_decay * p_new) - the product rounds
 *             once, the fused multiply-add once.  Both factors come from the host: decay in [0, 1), one_minus_decay rounded
 *             once from 1.0 - (double)decay.  decay == 0 makes the shadow equal the parameters exactly, provided the old
 *             shadow element is finite (0 * inf and 0 * NaN are NaN: a non-finite shadow stays non-finite at every decay).
 *   skip      guarded form: a skipped step stores nothing, ema keeps its bits along with p, m and v.
 * No warm-up of the decay: it would depend on the count of APPLIED steps, which the guarded form keeps on the device (guard
 * record, word 3), and the record's layout is fixed.  The caller starts the shadow as a copy of the parameters instead, so
 * it needs no bias correction.  Status 1 before any launch: null ema, n <= 0 or n % 4 != 0, decay outside [0, 1) or NaN,
 * null guard. */
int xas_adam_step_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1, float beta2,
                      float eps, int step, float decay, float one_minus_decay, void* stream);
int xas_adam_step_guarded_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1, float beta2,
                              float eps, float decay, float one_minus_decay, const void* guard, void* stream);

/* ------------------------------------------------------------------------------------
 * Evaluation path: hypothesis selection, triangulation, pose metrics.
 * One evaluation batch stays on the device; nothing here synchronises with the host.
 * ---------------------------------------------------------------------------------- */

/* Left/right switch + hypothesis selection + 2-D error for ONE camera, one launch.
 * Replaces eval_utils.py:7-30 (switch_points), eval.py:128-148 (per-hypothesis loop, best / confident
 * selection by argmin + gather) and eval_utils.py:32-43 (per_act_mse).
 * kps [B][Hy][K][C] (C = 2 or 3), joints [B][K][C] ground truth in PIXEL units unless
 * XAS_EVAL_GT_NORMALISED; perm [K] = index of the mirrored joint (identity where none).
 * Outputs (each may be NULL): sel3d [B][K][C] (selection by the C-dim squared error),
 * sel2d [B][K][2] (selection by the 2-D squared error), err2d [B], swapped [B][K] (0/1, flags of the LAST
 * hypothesis - what eval.py:132 keeps).  K <= 64. */
#define XAS_EVAL_CONFIDENT 1      /* take hypothesis 0 (eval.py:144-146) instead of the best one */
#define XAS_EVAL_SWITCH_ALL 2     /* one switch decision per sample (switch_points(switch_all=True)) */
#define XAS_EVAL_GT_NORMALISED 4  /* joints already in the detector's output range */
#define XAS_EVAL_NO_SWITCH 8      /* no partner test: every joint is kept as given (swapped = 0), e.g. after xas_multiview_resolve */
int xas_eval_select(const float* kps, const float* joints, const int* perm, int B, int Hy, int K, int C,
                    float image_size, int flags, float* sel3d, float* sel2d, float* err2d,
                    unsigned char* swapped, void* stream);

/* P [B][3][4] = k_mat [B][3][3] * [rot_world [B][3][3] | trans_world [B][3]].  modules/util.py:188. */
int xas_projection_matrix(const float* k_mat, const float* rot_world, const float* trans_world, int B, float* P,
                          void* stream);

/* Weighted DLT triangulation, replaces modules/util.py:198-230 (batch_triangulate: torch.linalg.svd of
 * [B][K][2V][4]).  points [B][V][K][3] = (u, v, weight) image coordinates, P [B][V][3][4];
 * out [B][K][4] = (X/w, Y/w, Z/w, mean weight).  V >= 2. */
int xas_triangulate_dlt(const float* points, const float* P, int B, int V, int K, float* out, void* stream);

/* Outlier-robust triangulation by exhaustive consensus (eval.py --tri robust; the reference has no counterpart, its
 * modules/util.py:198-230 is the DLT above over all views).  points [B][V][K][3] = (u, v, weight), P [B][V][3][4] as for
 * xas_triangulate_dlt; threshold_px > 0.  A view is VALID if its weight is finite and > 0.  Every subset S of >= 2 valid
 * views is a candidate: X_S = its DLT solution; the residual of a view is the pixel distance between its (u, v) and the
 * projection of X_S (+inf behind the camera); I(S) = the valid views with residual < threshold_px.  The best candidate has
 * the most inliers, then the smallest sum of squared inlier residuals, then the smallest bit mask.  The views used, F, are
 * its inliers, or all valid views if it has fewer than two.
 * out [B][K][4] = (X, Y, Z, mean weight over the views used): the DLT over F, the arithmetic of xas_triangulate_dlt
 * restricted to F (bit-identical to it where F is all V views); inliers [B][K] (bit v = view v used; 0 = fallback),
 * resid [B][K] = RMS reprojection residual in pixels of the result over the views used.  inliers / resid may be NULL.
 * Fewer than 2 valid views: NaN in xyz and resid, inliers 0, out[3] = mean weight of the valid views (NaN if none).
 * One wave per (b, joint), lane = subset mask: 2 <= V <= XAS_TRI_MAX_VIEWS. */
#define XAS_TRI_MAX_VIEWS 6
int xas_triangulate_robust(const float* points, const float* P, int B, int V, int K, float threshold_px, float* out,
                           unsigned char* inliers, float* resid, void* stream);

/* Left/right exchange and depth hypothesis of every view WITHOUT labels, by the agreement of the views (eval.py --resolve
 * views).  Stands beside eval_utils.py:7-29 (switch_points: one label bit per view, joint and hypothesis) and
 * eval.py:129-148 (best / confident selection against the label), on the DLT of modules/util.py:198-230; the reference has
 * no counterpart.
 * points [B][V][K][3] = (u px, v px, weight) and P [B][V][3][4] as for xas_triangulate_dlt (x and y are the same for all
 * hypotheses); kps [B][V][Hy][K][3] the detector's patch-normalised joints; world [B][V][Hy][K][3] the same joints through
 * xas_patch_to_world_fwd (single-view world mm); perm [K] as for xas_eval_select (perm[k] == k: unpaired; an entry that
 * is out of range or not mirrored by its partner also counts as unpaired); gt [B][V][K][3] labels in patch pixels,
 * normalised with image_size as xas_eval_select does, or NULL.
 * Stage 1, per sample and pair (a < c = perm[a]): a view is VALID if both joints' weights are finite and > 0; the ANCHOR is
 * the lowest valid view.  Candidates are the masks m over the valid views with the anchor bit clear.  Under m joint a takes
 * points[v][c] where bit v is set, else points[v][a]; joint c takes the other one.  Each joint is solved by the weighted DLT
 * over the valid views (the arithmetic of xas_triangulate_dlt, views in ascending order); cost(m) = the sum over the valid
 * views of both joints' squared reprojection residuals (+inf behind a camera).  The least cost wins, then the smaller mask.
 * An unpaired joint is the DLT over its valid views, mask 0.  Fewer than two valid views: xyz = NaN, mask 0.
 * Stage 2, per view (valid or not) and joint k: s = perm[k] if bit v of the mask is set, else k; h* = argmin_h
 * |world[b][v][h][s] - xyz[b][k]|^2 in double (first minimum; 0 if xyz is not finite); sel[b][v][k] = kps[b][v][h*][s].
 * Stage 3, only with gt, per sample and solved pair: a and c are exchanged in the pair's valid views and in xyzw if and only
 * if that strictly lowers the sum over those views and both joints of |dx| + |dy| of sel against the normalised labels
 * (the L1 criterion of switch_points, pooled); the mask is then complemented over the valid views.
 * Outputs: sel [B][V][K][3] (required); each of the others may be NULL: xyzw [B][K][4] = the triangulated point and the mean
 * weight of the valid views' resolved points (bit-identical to xas_triangulate_dlt on the resolved points where all views are
 * valid); swap [B][K] (bit v = view v's joint k was taken from perm[k]); hyp [B][V][K] = h*; named [B][K] = 1 where stage
 * 3 exchanged (written only with gt).
 * One wave per (b, joint k <= perm[k]), lane = mask: 2 <= V <= XAS_TRI_MAX_VIEWS, 1 <= K <= 64, 1 <= Hy <= 255 (hyp is a
 * byte), B*K < 2^31.  One launch, no host synchronisation. */
int xas_multiview_resolve(const float* points, const float* P, const float* kps, const float* world, const int* perm,
                          const float* gt, int B, int V, int Hy, int K, float image_size, float* sel, float* xyzw,
                          unsigned char* swap, unsigned char* hyp, unsigned char* named, void* stream);

/* Reprojection-error refinement of a triangulated point (eval.py --tri-refine lm; the reference has no counterpart: its
 * modules/util.py:198-230 stops at the DLT, which minimises the algebraic error |c (u P2 - P0) X|, not pixels).
 * points [B][V][K][3] = (u px, v px, weight) and P [B][V][3][4] as for xas_triangulate_dlt; init [B][K][4] = what
 * xas_triangulate_dlt or xas_triangulate_robust wrote; views [B][K] = the inliers of xas_triangulate_robust, or NULL.
 * A view is VALID if its weight is finite and > 0.  The views used, F, are the valid views whose bit is set in
 * views[b][k]; all valid views where views is NULL or the byte is 0 (the robust kernel's fallback code).  Bits of views
 * that are not valid, or >= V, are ignored.
 * For X in R^3 and a view v: h = P_v (X, 1), formed in double from the fp32 entries; X lies BEHIND v if h2 <= 0 (the rule of
 * xas_triangulate_robust; a NaN h2, from a P that is not finite, is not behind: the cost is then NaN, no trial is accepted and
 * the joint ends with status 1, out = init and NaN resid);
 * r_v = (h0 / h2 - u_v, h1 / h2 - v_v); s_v = the weight with XAS_REFINE_WEIGHTED, else 1; e_v = s_v |r_v|;
 * C(X) = sum over F of rho(e_v), rho(e) = e^2 if e <= huber or not huber > 0 (0, negative, NaN: plain least squares), else
 * 2 huber e - huber^2.  huber is in the unit of e: pixels unweighted, sigmas with weights 1 / sigma_px.
 * Levenberg-Marquardt on (X, Y, Z) from init, all arithmetic in double.  At X: psi_v = min(1, huber / e_v) (1 without
 * huber), J_v = d r_v / dX, H = sum psi_v s_v^2 J_v^T J_v, g = sum psi_v s_v^2 J_v^T r_v; a TRIAL is X + d with
 * (H + lambda diag(H)) d = -g, lambda = 1e-3 at the start.  A trial is ACCEPTED if C strictly decreases and it lies behind
 * no view used: X moves, lambda *= 0.1; otherwise lambda *= 10.  The loop stops when an accepted step is shorter than
 * 1e-5 (mm), after max_iter trials (1 <= max_iter <= 64), or when lambda > 1e12.  So C(out) <= C(init), always.
 * PASSED THROUGH: fewer than two views used, x, y or z of init not finite, or init behind a view used.
 * out [B][K][4] (required, must not overlap init) = (X, Y, Z) rounded to fp32 and init's fourth entry; passed through:
 * init bit for bit (NaN stays NaN).  Each of the others may be NULL:
 *   resid [B][K][2]  RMS of |r_v| over F (px, unweighted: the resid of xas_triangulate_robust) at init and at the result
 *   cov [B][K][6]    upper triangle (00 01 02 11 12 22) of the inverse of H at the result: the covariance of the point in
 *                    mm^2 where the weights are 1 / sigma_px; not finite where H is singular
 *   status [B][K]    0 = stopped on the step rule, 1 = ran out of trials or lambda, 2 = passed through (resid, cov = NaN)
 * One thread per (b, joint): 2 <= V <= XAS_TRI_MAX_VIEWS, B > 0, K >= 1, B*K < 2^31.  One launch, no host synchronisation. */
#define XAS_REFINE_WEIGHTED 1   /* residual of view v is scaled by its weight (points[..][2]); else by 1 */
int xas_triangulate_refine(const float* points, const float* P, const float* init, const unsigned char* views, int B, int V,
                           int K, int flags, float huber, int max_iter, float* out, float* resid, float* cov,
                           unsigned char* status, void* stream);

/* Skeleton-level refinement: xas_triangulate_refine with the joints of a sample coupled by left/right limb symmetry (eval.py
 * --tri-skeleton; the reference has no counterpart).  One least-squares problem per sample instead of one per joint.
 * points [B][V][K][3], P [B][V][3][4], init [B][K][4] and views [B][K] (or NULL) are exactly as for xas_triangulate_refine,
 * with its rules for VALID views, the views used F_k, BEHIND, XAS_REFINE_WEIGHTED (the only flag) and huber.
 * limbs [L][4] int32, a HOST array read before the launch: (far_a, near_a, far_b, near_b); limb a runs from joint far_a to
 * joint near_a and limb b is its mirror.  An index outside [0, K) is an error, not skipped.  NULL is allowed with L = 0.
 * sym_w >= 0 and finite, in px^2 per mm^2 (sigma^2 per mm^2 with XAS_REFINE_WEIGHTED).
 * A joint is FREE if xas_triangulate_refine would not pass it through: at least two views used, x, y and z of init finite, and
 * init behind none of the views used.  Otherwise it is FIXED: it leaves as init, bit for bit (NaN stays NaN), and takes part in
 * nothing.  A limb pair is ACTIVE if all four of its joints are free.
 * The cost over the free joints of one sample, in double from the fp32 inputs:
 *   C(X) = sum over free k and v in F_k of rho(s_vk |r_vk|)            (term for term the cost of xas_triangulate_refine)
 *        + sym_w * sum over active limb pairs of e^2,   e = |X_far_a - X_near_a| - |X_far_b - X_near_b|  (mm)
 * Levenberg-Marquardt on all free coordinates of the sample at once, in double.  H = the 3x3 blocks of
 * xas_triangulate_refine on the diagonal (with its psi) + sym_w * sum of J^T J over the active pairs, g = its g per joint +
 * sym_w * sum of J^T e, where J = d e / dX is +a / |a| at far_a, -a / |a| at near_a, -b / |b| at far_b, +b / |b| at near_b
 * (summed where a joint stands in several places).  If limb a or limb b of a pair is shorter than 1e-9 mm, the pair
 * contributes its residual but a zero row J: nothing is divided by the length.
 * A TRIAL is X + d with (H + lambda diag(H)) d = -g, solved by Cholesky; lambda = 1e-3 at the start.  A trial is ACCEPTED if
 * C strictly decreases and no free joint lies behind a view it uses: X moves, lambda *= 0.1; otherwise, and at a pivot that
 * is not positive, lambda *= 10.  The loop stops when the largest |coordinate change| of an accepted step is under 1e-5 (mm),
 * after max_iter trials (1 <= max_iter <= 64), or when lambda > 1e12.  So C(out) <= C(init), always.
 * out [B][K][4] (required, must not overlap init) = the point rounded to fp32 and init's fourth entry.  Each of the others may
 * be NULL:
 *   resid [B][K][2]  as in xas_triangulate_refine: RMS of |r_v| over F_k (px, unweighted) at init and at the result; NaN
 *                    for a fixed joint
 *   sym [B][L][2]    e in mm at init and at the result; NaN where the pair is not active
 *   cost [B][2]      C at init and at the result (0 for a sample with no free joint)
 *   status [B][K]    0 = the sample stopped on the step rule, 1 = it ran out of trials or lambda, 2 = the joint is fixed
 * There is no covariance output: the inverse of the coupled matrix is not formed.
 * One wave per sample; H and its Cholesky factor packed in LDS, 61 KB static per block: 2 <= V <= XAS_TRI_MAX_VIEWS,
 * 3 <= K <= XAS_SKEL_MAX_JOINTS, 0 <= L <= XAS_SKEL_MAX_LIMBS, B > 0, B*K < 2^31.  One launch, no host synchronisation, no
 * atomics: the result is a pure function of the inputs, bit for bit from run to run. */
#define XAS_SKEL_MAX_JOINTS 24
#define XAS_SKEL_MAX_LIMBS 16
int xas_triangulate_skeleton(const float* points, const float* P, const float* init, const unsigned char* views,
                             const int* limbs, int B, int V, int K, int L, int flags, float huber, float sym_w,
                             int max_iter, float* out, float* resid, float* sym, float* cost,
                             unsigned char* status, void* stream);

/* Bundle adjustment of the camera extrinsics over a whole evaluation set (eval.py --calibrate OUT.npz, applied by --calibration IN.npz; the reference has no
 * counterpart: everything above holds the cameras fixed).  points [N][V][K][3], P [N][V][3][4], init [N][K][4] and views [N][K]
 * (or NULL) are exactly as for xas_triangulate_refine, with its rules for VALID views, the views used F, BEHIND,
 * XAS_REFINE_WEIGHTED (the only flag) and huber; N counts the samples of the whole set.  rig_start [R+1] int32, a HOST array read
 * before the launch: samples rig_start[r] .. rig_start[r+1]-1 belong to rig r (non-decreasing, rig_start[0] = 0, rig_start[R] =
 * N, otherwise an error; a rig may be empty).  free_mask: bit v set = camera v of every rig may move; bits >= V are ignored.
 * UNKNOWNS of rig r, all double.  Per free camera v a correction delta_rv = (omega, tau) in R^6, a rigid motion of the world in
 * front of that camera: X' = exp([omega]x) X + tau, then h = P_nv (X', 1); the corrected matrix is P T(delta), T = [exp omega,
 * tau; 0 1], so nothing but P is needed.  exp is the plain exponential map I + sin(th) K / th + (1 - cos(th)) K^2 / th^2, K =
 * [omega]x, th = |omega|; for th^2 < 1e-16 its series I + K + K^2 / 2.  Per FREE point X_nk in R^3; a point is free if
 * xas_triangulate_refine would not pass it through, judged once at the start corrections (at least two views used, init finite,
 * init' in front of every view used); otherwise it is FIXED: it leaves as init, bit for bit, and takes part in nothing.
 * COST of rig r, in double from the fp32 inputs:
 *   C = sum over free points and v in F of rho(s_v |r_v|)  +  prior_rot sum |omega_rv|^2  +  prior_trans sum |tau_rv|^2
 * the first sum term for term the cost of xas_triangulate_refine once the corrections are 0, the prior sums over the free
 * cameras; prior_rot in cost per rad^2, prior_trans in cost per mm^2, both >= 0 and finite.  The prior pulls towards the given
 * calibration; with a camera held fixed it settles the gauge (scale only softly).
 * LINEARISATION: the corrections are updated additively, delta <- delta + d, and the Jacobian is re-linearised about the
 * current rotation with the exact derivative of the exponential map: d(u, v) / dX' = multiview.h's ju / jv,
 * dX' / d tau = I, dX' / d omega = -[exp(omega) X]x Jl(omega), Jl = I + (1 - cos th) K / th^2 + (th - sin th) K^2 / th^3 the left
 * Jacobian of SO(3) (series I + K / 2 + K^2 / 6), dX' / dX = exp(omega).  With psi and s of xas_triangulate_refine,
 * H = sum psi s^2 J^T J and g = sum psi s^2 J^T r over the residuals, plus prior on the diagonal of H_cc and prior * delta in g_c.
 * A TRIAL solves (H + lambda diag H) d = -g over all of the rig's unknowns exactly by eliminating the points: with A_p = H_pp +
 * lambda diag H_pp (3x3, Cholesky) and B_p = H_cp (6 V_free x 3, rows of the views the point uses),
 *   S = H_cc + lambda diag H_cc - sum_p B_p A_p^-1 B_p^T,  b = -g_c + sum_p B_p A_p^-1 g_p,  S d_c = b by Cholesky (S is at most
 *   36 x 36; camera slots are the free cameras in ascending order, 6 rows each: omega, tau),  d_p = -A_p^-1 (g_p + B_p^T d_c).
 * lambda = 1e-3 at the start.  A trial is ACCEPTED if the rig's C strictly decreases and no free point lies behind a view it
 * uses: the state moves, lambda *= 0.1; otherwise, and at a pivot of S that is not positive, lambda *= 10.  The loop stops when
 * an accepted step changes every point coordinate by less than 1e-5 (mm), every omega component by less than
 * XAS_CALIB_STEP_TOL_ROT (rad) and every tau component by less than XAS_CALIB_STEP_TOL_TRANS (mm); after max_iter trials
 * (1 <= max_iter <= 64); or when lambda > 1e12.  So C(out) <= C(start), always.  Rigs are independent: each has its own lambda,
 * stop and status, and its result does not depend on the other rigs, bit for bit.
 * xas_calibrate_bundle.  delta [R][V][6] double (required) is read as the start (0, or an earlier result; entries of fixed
 * cameras are taken as 0) and written with the result (fixed cameras: 0).  out [N][K][4] (required, must not overlap init) =
 * the point rounded to fp32 and init's fourth entry.  Each of the others may be NULL:
 *   cost [R][2] double    C at the start and at the result
 *   rms [R][2] double     RMS of |r_v| in px, unweighted, over the views used of the free points, at the start and at the
 *                         result; NaN for a rig with no free point
 *   cam_cov [R][6V][6V]   double: the inverse of S at the result with lambda = 0, rows and columns by view (6 v + (omega, tau));
 *                         those of fixed cameras are 0; NaN where S has no positive pivot.  A large entry = a camera parameter
 *                         that the data (and the prior) did not determine.
 *   status [R] bytes      0 = stopped on the step rule, 1 = ran out of trials or lambda, 2 = the rig has no free point:
 *                         everything passed through, delta = the start.  With no free camera (free_mask = 0) the free points
 *                         alone are solved (S is empty, d_p = -A_p^-1 g_p): xas_triangulate_refine's problem per point under
 *                         one lambda and one stop per rig
 *   trials [R][2] int32   trials made and trials accepted (what the tests compare with the oracle's schedule)
 * xas_calibrate_linearise: one linearisation at the state (delta, the points of init) with the given lambda >= 0: S [R][n][n]
 * (dense, symmetric, n = 6 * the number of free cameras), b [R][n] and C [R], all double and required (S and b may be NULL
 * when n = 0).  It exists so that the
 * Schur assembly can be tested on its own.
 * workspace: xas_calibrate_workspace_bytes(N, V, K, R) bytes (0 for a shape outside the limits), 16-byte aligned.
 * Limits: 2 <= V <= XAS_TRI_MAX_VIEWS, K >= 1, N > 0, N*K < 2^31, 1 <= R <= XAS_CALIB_MAX_RIGS.
 * Four launches per trial, all enqueued up front (a stopped rig's blocks return at once), no host synchronisation, no atomics,
 * every sum in one order: two calls on the same inputs give the same bits in every output. */
#define XAS_CALIB_MAX_RIGS 16
#define XAS_CALIB_STEP_TOL_ROT 1e-9     /* rad: 1e-5 mm at 10 m.  Untuned. */
#define XAS_CALIB_STEP_TOL_TRANS 1e-5   /* mm, the points' tolerance.  Untuned. */
size_t xas_calibrate_workspace_bytes(int N, int V, int K, int R);
int xas_calibrate_linearise(const float* points, const float* P, const float* init, const unsigned char* views,
                            const int* rig_start, int N, int V, int K, int R, int free_mask, int flags, float huber,
                            double prior_rot, double prior_trans, double lambda, const double* delta, double* S, double* b,
                            double* C, void* workspace, void* stream);
int xas_calibrate_bundle(const float* points, const float* P, const float* init, const unsigned char* views,
                         const int* rig_start, int N, int V, int K, int R, int free_mask, int flags, float huber,
                         double prior_rot, double prior_trans, int max_iter, double* delta, float* out, double* cost,
                         double* rms, double* cam_cov, unsigned char* status, int* trials, void* workspace, void* stream);

/* Temporal smoothing of triangulated joint tracks over a whole evaluation set (eval.py --smooth OUT.npz; the reference has no
 * counterpart: everything above works inside one frame).  points [N][V][K][3], P [N][V][3][4], init [N][K][4] and views [N][K]
 * (or NULL) are exactly as for xas_triangulate_refine, with its rules for VALID views, the views used F, BEHIND,
 * XAS_REFINE_WEIGHTED (the only flag) and huber; N counts the samples of the whole set, sorted by track and frame.
 * start [S+1] int32, a HOST array read before the launch: samples start[s] .. start[s+1]-1 are track s (start[0] = 0, start[S]
 * = N, increasing: every track has a sample; otherwise an error).  frame [N] int32 on the device: the frame number tau of every
 * sample, strictly increasing inside a track (the caller's duty: the kernel does not check it; a repeated frame gives a step
 * h = 0, a cost that is not finite, no accepted trial and out = the start).  acc_w >= 0 and finite, in px^2 per
 * (mm^2 / frame^3) (sigma^2 with XAS_REFINE_WEIGHTED).
 * Per (track, joint), T = the track's length: a frame is a DATA frame if xas_triangulate_refine would not pass it through (at
 * least two views used, x, y and z of init finite, init behind no view used).  Every other frame is a GAP frame: it has no
 * reprojection term, and it starts on the line in tau through the nearest data frames on either side, X_l + (X_r - X_l)
 * (tau - tau_l) / (tau_r - tau_l); beyond the ends of the data at the nearest data frame's point.  A (track, joint) with fewer
 * than two data frames is PASSED THROUGH: out = init bit for bit (NaN stays NaN).
 * COST, in double from the fp32 inputs, over X_t in R^3, t = 0 .. T-1:
 *   C = sum over data t and v in F_t of rho(s_v |r_v(X_t)|)            (term for term the cost of xas_triangulate_refine)
 *     + acc_w sum_{t=1..T-2} 2 / (h0 + h1) |(X_t+1 - X_t) / h1 - (X_t - X_t-1) / h0|^2,  h0 = tau_t - tau_t-1, h1 = tau_t+1 - tau_t
 * the second sum the discretised integral of |X''|^2 of a cubic smoothing spline on a non-uniform grid: X^T (A x I3) X with A
 * pentadiagonal, A = sum_t 2 / (h0 + h1) c_t c_t^T, c_t = (1 / h0 at t-1, -(1 / h0 + 1 / h1) at t, 1 / h1 at t+1).
 * Levenberg-Marquardt on all 3 T coordinates at once, in double.  H = the 3x3 blocks of xas_triangulate_refine on the diagonal
 * of the data frames (with its psi) + acc_w (A x I3), g = its g per data frame + acc_w (A x I3) X.  A TRIAL is X + d with
 * (H + lambda diag H) d = -g by a block-pentadiagonal Cholesky (3x3 blocks, half-bandwidth 8); lambda = 1e-3 at the start.  A
 * trial is ACCEPTED if C strictly decreases and no data frame's point lies behind a view it uses: X moves, lambda *= 0.1;
 * otherwise, and at a pivot that is not positive, lambda *= 10.  The loop stops when the longest per-frame step |d_t| of an
 * accepted trial is under 1e-5 (mm), after max_iter trials (1 <= max_iter <= 64), or when lambda > 1e12.  So C(out) <=
 * C(start), always.  With acc_w = 0 a gap frame has a zero pivot: every trial is rejected and out = the start.
 * xas_track_smooth.  out [N][K][4] (required, must not overlap init) = (X, Y, Z) rounded to fp32 and init's fourth entry bit
 * for bit.  Each of the others may be NULL:
 *   status [N][K] bytes        0 = data frame smoothed, 1 = gap frame filled, 2 = passed through
 *   resid [N][K][2]            RMS of |r_v| over F (px, unweighted) at the start and at the result; NaN for gap and
 *                              passed-through frames
 *   track_status [S][K] bytes  0 = stopped on the step rule, 1 = ran out of trials or lambda, 2 = passed through
 *   cost [S][K][2] double      C at the start and at the result (0 where passed through)
 *   trials [S][K] int32        trials made (0 where passed through)
 * xas_track_linearise: one linearisation at the start (the points of init, gap frames filled) with the given lambda >= 0, all
 * double and required: band [N][K][3][9], entry [n][k][c][o] = element (i, i - o) of H + lambda diag H for row i = 3 t + c
 * of the (track, joint) that sample n is frame t of (0 where i - o < 0, and where the column lies outside the block row);
 * g [N][K][3]; C [S][K].  Passed through: band, g and C are 0.  It exists so that the assembly can be tested on its own.
 * workspace: xas_track_smooth_workspace_bytes(N, K) bytes (0 for a shape outside the limits), 16-byte aligned; its content
 * before the call does not matter.  The band's factor, g, d, X and the trial point live there: no bound on T beyond N.
 * Limits: 2 <= V <= XAS_TRI_MAX_VIEWS, K >= 1, N > 0, N*K < 2^31, 1 <= S <= N, S*K < 2^31.
 * One wave per (track, joint); one launch after the copy of start (one small launch per 512 tracks), all enqueued up front,
 * no host synchronisation, no atomics, every sum in one order: two calls on the same inputs give the same bits in every output. */
size_t xas_track_smooth_workspace_bytes(int N, int K);
int xas_track_linearise(const float* points, const float* P, const float* init, const unsigned char* views, const int* start,
                        const int* frame, int N, int V, int K, int S, int flags, float huber, double acc_w, double lambda,
                        double* band, double* g, double* C, void* workspace, void* stream);
int xas_track_smooth(const float* points, const float* P, const float* init, const unsigned char* views, const int* start,
                     const int* frame, int N, int V, int K, int S, int flags, float huber, double acc_w, int max_iter,
                     float* out, unsigned char* status, float* resid, unsigned char* track_status, double* cost, int* trials,
                     void* workspace, void* stream);

/* xas_track_smooth with one more kind of observation, a 3-D ANCHOR per frame and joint (eval.py --smooth --smooth-data anchor;
 * the reference has no counterpart): a point A with a symmetric 3x3 information matrix W.  One camera's chosen point on its ray
 * is one (W = depth_w r r^T along the ray r: the pixels know the point across the ray, the anchor along it), the point of
 * xas_triangulate_volume with the inverse of its covariance another.  Everything not said here is exactly as xas_track_smooth
 * and xas_track_linearise state it: points, P, init, views, start, frame, flags, huber, acc_w, the gap frames' start line, the
 * pass-through of a (track, joint) with fewer than two data frames, the prior, the lambda schedule, the acceptance and stop
 * rules, every output, "C(out) <= C(start)", the workspace (xas_track_anchor_workspace_bytes(N, K), the same number) and the
 * limits, except that 1 <= V <= XAS_TRI_MAX_VIEWS.
 * anchor [N][K][3] fp32 (mm) and info [N][K][6] fp32, the entries xx, xy, xz, yy, yz, zz of W in cost units per mm^2 (px^2, or
 * sigma^2 with XAS_REFINE_WEIGHTED, like the reprojection term beside it): both NULL or both given, otherwise an error.  W
 * positive semi-definite is the caller's duty, as an increasing `frame` is.  anchor_huber >= 0 and finite; 0 = squared.
 * A frame's anchor is USABLE if its nine numbers are finite, no diagonal entry of W is negative and trace W > 0.
 * The START of a frame is init's point if its x, y and z are finite, otherwise the usable anchor.
 * Without a usable anchor a frame is a data frame by xas_track_smooth's rule.  With one it is ALWAYS a data frame: its
 * reprojection term runs over the views F that xas_triangulate_refine would use (VALID views, and `views`: a zero byte stands
 * for all valid views here too, so the term is switched off by weights of 0, not by `views`), however few; if the start lies
 * behind one of them, F is empty and the frame keeps its anchor term only.
 * COST of a data frame, in double from the fp32 inputs: sum_{v in F} rho(s_v |r_v(X_t)|) + rho_a(m_t), m_t = sqrt(max(e_t^T W_t
 * e_t, 0)), e_t = X_t - A_t, rho_a the Huber function of the reprojection term with delta anchor_huber (the clamp: a
 * rank-deficient W rounded to fp32 may be indefinite in its last bit).  The anchor term adds psi(m) W to the frame's
 * Gauss-Newton block and psi(m) W e to its gradient, psi = 1 on the quadratic part and anchor_huber / m on the linear one, as
 * xas_triangulate_refine weights its own Huber.
 * Outputs as there; resid's two entries stay the pixel RMS over F and are NaN where F is empty; status 0 = data frame (with or
 * without an anchor).  With NULL anchors and V >= 2 every output of both entry points equals xas_track_smooth's and
 * xas_track_linearise's bit for bit: the schedule is one piece of code (csrc/track_band.h).
 * One wave per (track, joint); one launch after the copy of start, no host synchronisation, no atomics, every sum in one
 * order: two calls on the same inputs give the same bits in every output. */
size_t xas_track_anchor_workspace_bytes(int N, int K);
int xas_track_anchor_linearise(const float* points, const float* P, const float* init, const unsigned char* views,
                               const float* anchor, const float* info, const int* start, const int* frame, int N, int V, int K,
                               int S, int flags, float huber, double anchor_huber, double acc_w, double lambda, double* band,
                               double* g, double* C, void* workspace, void* stream);
int xas_track_anchor_smooth(const float* points, const float* P, const float* init, const unsigned char* views,
                            const float* anchor, const float* info, const int* start, const int* frame, int N, int V, int K,
                            int S, int flags, float huber, double anchor_huber, double acc_w, int max_iter, float* out,
                            unsigned char* status, float* resid, unsigned char* track_status, double* cost, int* trials,
                            void* workspace, void* stream);

/* xas_track_anchor_smooth for all joints of a track at once, COUPLED BY THE LENGTHS OF THE BONES (eval.py --smooth
 * --smooth-bones; the reference has no counterpart).  points, P, init, views, anchor, info, start, frame, N, V, K, S, flags,
 * huber, anchor_huber and acc_w are exactly those of xas_track_anchor_smooth, with its rules word for word: valid views, the
 * views used, BEHIND, data and gap frames, the start of a frame, the start line of a gap frame, the prior, XAS_REFINE_WEIGHTED.
 * bones [Bn][2] int32, a HOST array read before the launch like limbs of xas_triangulate_skeleton: joint indices in [0, K); an
 * index outside, or a bone from a joint to itself, is an error; NULL with Bn = 0.  length [S][Bn] fp32 on the device: the
 * bone's length in mm for that track.  bone_w >= 0 and finite, in cost units per mm^2 (px^2, or sigma^2 with the flag).
 * A (track, joint) that xas_track_anchor_smooth would pass through (fewer than two data frames) is FIXED: out = init bit for
 * bit in every frame, and it takes part in nothing.  Every other is FREE.  A bone is ACTIVE in a track if both its joints are
 * free and its length is finite and > 0; an active bone acts in EVERY frame of the track, gap frames included.
 * COST of a track, in double from the fp32 inputs, over the free joints X[t,k]:
 *   C = sum over free k of C_k                      (term for term the cost of xas_track_anchor_smooth for that joint)
 *     + bone_w sum over active b = (i, j) and all t of e^2,  e = |X[t,i] - X[t,j]| - length[s][b]
 * The Gauss-Newton row of a bone is +u at i and -u at j, u = d / |d|, d = X[t,i] - X[t,j]; where |d| < 1e-9 mm the residual
 * counts but the row is zero and nothing is divided by |d| (the rule of xas_triangulate_skeleton).
 * ONE Levenberg-Marquardt problem per track over all free joints and frames.  A TRIAL is X + d with (H + lambda diag H) d = -g;
 * the lambda schedule, the acceptance rule and the stop rule are those of xas_track_smooth (lambda from 1e-3; accepted if C
 * strictly decreases and no data frame's point lies behind a view it uses, then lambda *= 0.1, otherwise and at a pivot that is
 * not positive lambda *= 10; stop when the longest |d[t,k]| of an accepted trial is under 1e-5 mm, after max_iter trials, 1 <=
 * max_iter <= 64, or when lambda > 1e12).  So C(out) <= C(start), always.
 * With the unknown 3K t + 3k + c the matrix is block-pentadiagonal with blocks of side n = 3K: the diagonal block of frame t
 * holds the joints' 3x3 data blocks and acc_w A_tt on its diagonal plus bone_w sum J^T J, which couples the joints of that
 * frame; the blocks (t, t-1) and (t, t-2) are acc_w A_t,t-1 and acc_w A_t,t-2 times the identity on the free joints.  It is
 * solved by a block Cholesky with a forward and a back substitution over the frames.  A fixed joint's rows are identity rows
 * with a zero right-hand side: the other unknowns do not feel them.
 * xas_track_skeleton_smooth.  out [N][K][4] (required, must not overlap init), status [N][K] and resid [N][K][2] as
 * xas_track_smooth (2 and NaN for a fixed joint).  Each but out may be NULL:
 *   bone [N][Bn][2] fp32       e in mm at the start and at the result; NaN where the bone is not active in that track
 *   track_status [S] bytes     0 = stopped on the step rule, 1 = ran out of trials or lambda, 2 = no free joint
 *   cost [S][2] double         C at the start and at the result (0 with no free joint)
 *   trials [S] int32           trials made (0 with no free joint)
 * xas_track_skeleton_linearise: one linearisation at the start with the given lambda >= 0, all double and required: g
 * [N][K][3]; hdiag [N][3K][3K], the diagonal block of H + lambda diag H of that sample's frame, rows and columns of fixed
 * joints 0; hoff [N][2], the scalars acc_w A_t,t-1 and acc_w A_t,t-2 (0 where t-1 or t-2 lies outside the track); d [N][K][3],
 * the solution of the trial system, 0 for fixed joints, NaN for the whole track if a pivot was not positive; C [S].  d is there
 * so that the block factorisation can be tested apart from the loop.
 * workspace: xas_track_skeleton_workspace_bytes(N, K) bytes (0 for a shape outside the limits or a size that does not fit
 * size_t, else a multiple of 16), 16-byte aligned; its content before the call does not matter.  Per frame it holds the three
 * factor blocks L_tt, L_t,t-1 and L_t,t-2 (3 n^2 doubles) and 10 n + 3 doubles of X, the trial point, g, d and the data
 * blocks: 74,328 bytes per frame at K = 18, 69,984 of them the factor.  T is bounded by N alone.
 * Limits: 1 <= V <= XAS_TRI_MAX_VIEWS, 1 <= K <= XAS_SKEL_MAX_JOINTS, 0 <= Bn <= XAS_TRACK_MAX_BONES, N > 0, 1 <= S <= N.
 * One workgroup of 256 threads per track, the block in work and its factor in LDS (125 KB static); one launch after the copy
 * of start, no host synchronisation, no atomics, every sum in one order: two calls on the same inputs give the same bits in
 * every output. */
#define XAS_TRACK_MAX_BONES 32
size_t xas_track_skeleton_workspace_bytes(int N, int K);
int xas_track_skeleton_linearise(const float* points, const float* P, const float* init, const unsigned char* views,
                                 const float* anchor, const float* info, const int* bones, const float* length,
                                 const int* start, const int* frame, int N, int V, int K, int S, int Bn, int flags, float huber,
                                 double anchor_huber, double acc_w, double bone_w, double lambda, double* g, double* hdiag,
                                 double* hoff, double* d, double* C, void* workspace, void* stream);
int xas_track_skeleton_smooth(const float* points, const float* P, const float* init, const unsigned char* views,
                              const float* anchor, const float* info, const int* bones, const float* length, const int* start,
                              const int* frame, int N, int V, int K, int S, int Bn, int flags, float huber, double anchor_huber,
                              double acc_w, double bone_w, int max_iter, float* out, unsigned char* status, float* resid,
                              float* bone, unsigned char* track_status, double* cost, int* trials, void* workspace,
                              void* stream);

/* Depth hypothesis and left/right exchange of ONE camera chosen over time (eval.py --resolve-track OUT.npz; the reference has
 * no counterpart, and no labels are read).  kps [N][Hy][K][3] the detector's patch-normalised joints, world [N][Hy][K][3] their
 * single-view world points in mm, unary [N][Hy][K] an extra cost per candidate or NULL (= 0), all fp32 on the device; N counts
 * the samples of the whole set, sorted by track and frame; start [S+1] and frame [N] exactly as for xas_track_smooth.
 * perm [K] int32, a HOST array like start, read before the launch (the kernel receives it by value, so no device copy exists
 * that could differ from what was checked): an involution, perm[perm[k]] = k, as ops_eval.switch_perm builds it.
 * A UNIT is a pair (a, b = perm[a]), a < b, or a joint k = perm[k].  The state of a pair at a frame is (e, h0, h1), e in
 * {0, 1}, h0 and h1 in [0, Hy), index e Hy^2 + h0 Hy + h1: joint a is candidate h0 of channel (e ? b : a), joint b candidate
 * h1 of channel (e ? a : b).  The state of a single joint is h.  A frame is USABLE for a unit if every coordinate of every
 * candidate of the unit's channels in world, and every such value of unary if given, is finite.  Over the usable frames
 * t0 < t1 < ... of the track, in double from the fp32 inputs, with Xa, Xb the world points the state reads and ua, ub their
 * unary values,
 *   C = sum_t [ hyp_w (h0 + h1) + swap_w e + ua + ub ]
 *     + vel_w sum over consecutive usable (t', t) of (|Xa_t - Xa_t'|^2 + |Xb_t - Xb_t'|^2) / (frame_t - frame_t')
 * (a random walk: an unusable frame is bridged with the variance of the gap; a single joint has no e and no b terms).  The
 * result is an exact minimiser (Viterbi); among equal costs the smallest predecessor index at every frame and the smallest end
 * state.  A unit with fewer than two usable frames is PASSED THROUGH: hypothesis 0, not exchanged, status 1, cost 0; so is an
 * unusable frame of a resolved unit, for that frame only.
 *   sel [N][K][3] (required)   the chosen candidate's entry of kps, bit for bit: the layout of xas_eval_select's sel3d
 *   hyp, swap, status [N][K] bytes, each may be NULL: the hypothesis, the exchange bit (both joints of a pair carry it),
 *                              0 = resolved / 1 = passed through
 *   cost [S][K] double or NULL C of the unit (both joints of a pair carry it)
 * workspace: xas_track_resolve_workspace_bytes(N, Hy, K) bytes (0 for a shape outside the limits, else a multiple of 16),
 * 16-byte aligned; its content before the call does not matter.  It holds start and one back-pointer byte per frame and state.
 * Limits: 1 <= Hy <= XAS_TRACK_MAX_HYPO (2 Hy^2 states are the lanes of one wave), 1 <= K <= XAS_TRACK_MAX_JOINTS, N > 0,
 * N*K < 2^31, 1 <= S <= N; vel_w, hyp_w, swap_w finite and >= 0; no output may overlap kps, world, unary or frame.
 * One wave per (track, unit); one launch after the copy of start, no host synchronisation, no atomics: two calls on the same
 * inputs give the same bits in every output, and the inputs are not written. */
#define XAS_TRACK_MAX_HYPO 5
#define XAS_TRACK_MAX_JOINTS 64
size_t xas_track_resolve_workspace_bytes(int N, int Hy, int K);
int xas_track_resolve(const float* kps, const float* world, const float* unary, const int* perm, const int* start,
                      const int* frame, int N, int Hy, int K, int S, double vel_w, double hyp_w, double swap_w, float* sel,
                      unsigned char* hyp, unsigned char* swap, unsigned char* status, double* cost, void* workspace,
                      void* stream);

/* Volumetric fusion of the views' heat-map cubes (eval.py --tri-volume; the reference has no counterpart).  Every other
 * triangulation here starts from ONE point per view, the soft-argmax of that view's heat-map; this one multiplies the views'
 * whole distributions over a voxel grid round the triangulated point (a product of experts) and takes the soft-argmax of the
 * product in world space, so a view whose heat-map has two modes contributes both and the other views choose.
 * logits: a HOST array of V device pointers, read before the launch; logits[v] is view v's [B][H][W][K*D] fp32 logits, the
 * head's NHWC layout (L[b,k,d,h,w] = logits[v][((b H + h) W + w) K D + k D + d]), D == H == W.
 * chan [V][B][K] int32 on the device, or NULL = k: the heat-map channel that view v reads for joint k (it carries a left/right
 * exchange of a view or of a joint).  trans_image [V][B][2][3], k_mat [V][B][3][3], pelvis [V][B][3], rot_world [V][B][3][3],
 * trans_world [V][B][3]: the arrays of xas_world_to_patch_fwd with a leading [V].  init [B][K][3] world mm.  views [B][K] or
 * NULL = every bit set: bit v = view v is selected (a zero byte selects NO view here).  weight [V][B][K] or NULL = 1.
 * View v TAKES PART in joint (b, k) if its bit is set, its weight is finite and > 0 and its channel lies in [0, K).
 * Grid: level l = 0 .. levels - 1 is an axis-aligned world cube of side side_l = side_mm 2^-l with G^3 voxels, centres
 * c_l + ((i + 0.5) / G - 0.5) side_l per axis, i = 0 .. G - 1; c_0 = init, c_(l+1) = the result of level l (in double).
 * World -> cube of view v, with S = image_size (the inverse of the head's normalisation followed by xas_patch_to_world_fwd):
 *   Pc = R X + T;  u = fx Xc / Zc + cx, v = fy Yc / Zc + cy;  (u', v') = A (u, v) + t;
 *   w = u' W / (S - 1), h = v' H / (S - 1), d = ((Zc - pelvis_z) S / rect_width / (S - 1) + 1) D / 2.
 * sample_v(X): each of (w, h, d) is clamped to [0, D - 1]; o = the L1 distance in cells that the clamp removed; the sample
 * is the trilinear interpolation of the logits at the clamped point (base cell min(floor(c), D - 2) per axis) minus
 * out_penalty * o: continuous across the cube's border, and no softmax normaliser is needed because a constant per view
 * changes nothing below.  Zc <= 0: o = 3 D and the point is (0, 0, 0).
 * score(X) = beta * sum over the views taking part, in ascending order, of weight_v sample_v(X).  The result of a level is
 * sum over its voxels of softmax(score) X; cov is the covariance of that distribution at the last level.
 * Logits are read as fp32; projections, interpolation, exp and every sum run in double; xyz and cov are rounded once.
 * xyz [B][K][3] (required); cov [B][K][6] mm^2 (xx xy xz yy yz zz) and status [B][K] may be NULL.  status:
 *   0 fused;  1 passed through (xyz = init bit for bit, cov = NaN): fewer than two views take part, or init is not finite;
 *   2 fused, but the voxel of the largest score at the last level (the first in x-fastest order among equals) lies on a face
 *     of the grid: the mode may lie outside;
 *   3 one of the eight logits read for a sample, at any level, was not finite: passed through as for 1, that joint only.
 * One workgroup per (b, joint), voxels strided over its threads, per-thread online-softmax records merged by wave shuffles
 * and then through LDS in a fixed order; the level loop runs inside the kernel: one launch, no host synchronisation, no
 * atomics, the result is a pure function of the inputs bit for bit.  D % 4 == 0 in [4, 128] (the head's range),
 * 1 <= V <= XAS_TRI_MAX_VIEWS, 2 <= G <= 32, 1 <= levels <= 4, side_mm, beta and out_penalty finite and > 0, B*K < 2^31. */
int xas_triangulate_volume(const float* const* logits, const int* chan, const float* trans_image, const float* k_mat,
                           const float* pelvis, const float* rot_world, const float* trans_world, const float* init,
                           const unsigned char* views, const float* weight, int B, int V, int K, int D, int G, int levels,
                           float side_mm, float beta, float out_penalty, float image_size, float rect_width, float* xyz,
                           float* cov, unsigned char* status, void* stream);

/* Smallest (lambda_1 - lambda_0) / lambda_3 at which xas_multiview_consistency_bwd differentiates through X (below). */
#define XAS_MV_MIN_GAP 1e-10
/* Multi-view consistency loss of the training step (train.py --mv-2d / --mv-3d; the reference has no counterpart: its step
 * treats the cameras of a sample as independent images).  The joint that the views triangulate to is a label-free 3-D target
 * of every view and its reprojection a label-free 2-D target: the algebraic-triangulation loss of Iskakov et al. 2019 and
 * the triangulated pseudo-label of Kocabas et al. 2019, differentiable through the DLT's null vector.
 * Inputs, contiguous fp32: kps_xy [B][V][K][2] = hypothesis 0's normalised patch x, y of every camera (the hypotheses share
 * x and y); trans_image [B][V][2][3] the crop affines; world [B][V][Hy][K][3] every hypothesis's single-view world point in
 * mm (xas_patch_to_world_fwd); P [B][V][3][4]; weight [B][V][K] or NULL = every view counts 1.  image_size S > 1.
 * A view is VALID for a joint if its weight is finite and > 0 (the rule of xas_triangulate_robust); x or y that is not
 * finite does not invalidate a view, it makes X not finite.  F = the valid views, n = |F|.  Per (b, k):
 *   1. (u_v, v_v) = A_v^-1 ((x + 1) / 2 (S - 1) - t0, (y + 1) / 2 (S - 1) - t1), A_v | t the crop affine: the patch stage
 *      of xas_patch_to_world_fwd in fp32, rounding for rounding (bit for bit what it writes under XAS_GEO_IMAGE): det =
 *      fl(a00 a11) - fl(a01 a10); the four entries of A^-1 each one division; p = fl(fl((x + 1) / 2) (S - 1)); d = p - t;
 *      u = fma(i00, du, fl(i01 dv)), v = fma(i11, dv, fl(i10 du)).  Everything after this is in double from the fp32 numbers.
 *   2. X = the DLT over F, the arithmetic of xas_triangulate_dlt restricted to F: rows c_v (u P2 - P0), c_v (v P2 - P1)
 *      formed in fp32, Gram matrix and null vector in double, views in ascending order.
 *   3. r_v = (h0 / h2 - u_v, h1 / h2 - v_v), h = P_v (X, 1), in pixels; e_v = |r_v|.
 *   4. reproj[b][k] = (1 / n) sum over F of rho(e_v); rho(e) = e^2 if e <= huber_px or huber_px = 0, else
 *      2 huber_px e - huber_px^2 (the rho of xas_triangulate_refine).
 *   5. h*_v = argmin_h |world[b][v][h][k] - X|^2 (first minimum; NaN never wins), for every view, valid or not: the rule of
 *      xas_multiview_resolve.  0 for a joint passed through.
 *   6. depth[b][k] = (1 / n) sum over F of |world[b][v][h*_v][k] - X|^2 in mm^2.
 * PASSED THROUGH (status 2; reproj = depth = 0 exactly, every gradient of the joint exactly 0, xyz = NaN): n < 2, X not
 * finite, or X behind a view of F (h2 <= 0 there: the rule of xas_triangulate_robust).  Otherwise status 0.
 * Outputs of the forward: reproj [B][K], depth [B][K], xyz [B][K][3] = X rounded to fp32, hsel [B][V][K] int32 = h*_v,
 * status [B][K] bytes; all required.
 * The backward takes the same inputs and g_reproj [B][K], g_depth [B][K], recomputes the Gram matrix and ALL its eigenpairs,
 * and writes EVERY entry of grad_kps_xy [B][V][K][2] and grad_world [B][V][Hy][K][3] (zeros for views not in F, hypotheses
 * not selected and joints passed through): nothing needs a memset, and no atomics, so the result is a pure function of the
 * inputs.  h*_v is a constant of the differentiation.  With a = g_reproj / n, d = g_depth / n, psi_v = 1 or huber_px / e_v
 * in rho's linear part:
 *   d / d world[b][v][h*_v][k] = 2 d (world - X);       direct d / d (u_v, v_v) = -2 a psi_v r_v.
 * With XAS_MV_DETACH_TARGET that is all: X is a constant, the 2-D term pulls each (u_v, v_v) towards the reprojection and
 * the 3-D term each selected world point towards X.  Without it the gradient also flows through X into every view of F:
 *   g_X = sum over F of (2 a psi_v J_v^T r_v - 2 d (world - X)), J_v = d (h0 / h2, h1 / h2) / dX;
 *   x = the unit eigenvector of the smallest eigenvalue lambda_0 of the Gram matrix G, X = x[:3] / x[3], (lambda_j, v_j) the
 *   other three:  g_x = (g_X / x3, -(g_X . x[:3]) / x3^2);
 *   g_G = sum over j != 0 of (v_j . g_x) / (lambda_0 - lambda_j) sym(v_j x^T), sym(M) = (M + M^T) / 2;
 *   d / du_v = 2 c_v^2 a_u^T g_G P2_v with a_u = u_v P2_v - P0_v, d / dv_v likewise with a_v = v_v P2_v - P1_v.
 * The terms through X grow like 1 / (lambda_1 - lambda_0).  Where lambda_1 - lambda_0 <= XAS_MV_MIN_GAP * lambda_3 (views that
 * coincide, rays that are parallel: x is any vector of a plane and has no derivative) they are left out and the joint gets the
 * gradient of XAS_MV_DETACH_TARGET; above that gap they are finite but may be large, and it is the caller's gradient clipping
 * that bounds them.
 * Then (u, v) -> (x, y): the transposed inverse affine and (S - 1) / 2.  Gradients go to kps_xy and world only.
 * One thread per (b, joint), loops over the views unrolled to XAS_TRI_MAX_VIEWS and predicated: 2 <= V <= XAS_TRI_MAX_VIEWS,
 * 1 <= Hy <= 8, B >= 1, K >= 1, B*K < 2^31, huber_px >= 0 and finite.  One launch each, no host synchronisation. */
#define XAS_MV_DETACH_TARGET 1  /* X is a constant of the backward pass (a pseudo-label), not a function of the views */
int xas_multiview_consistency_fwd(const float* kps_xy, const float* trans_image, const float* world, const float* P,
                                  const float* weight, int B, int V, int Hy, int K, float image_size, float huber_px,
                                  int flags, float* reproj, float* depth, float* xyz, int* hsel, unsigned char* status,
                                  void* stream);
int xas_multiview_consistency_bwd(const float* kps_xy, const float* trans_image, const float* world, const float* P,
                                  const float* weight, const float* g_reproj, const float* g_depth, int B, int V, int Hy,
                                  int K, float image_size, float huber_px, int flags, float* grad_kps_xy,
                                  float* grad_world, void* stream);

/* Z-buffered triangle rasteriser: the last stage of the online pseudo-image path (train.py --pseudo-online; the reference
 * reads pre-rendered PNGs and has no renderer).  Forward only, no atomics, a pure function of its inputs bit for bit.
 * Inputs, contiguous: verts [B][Nv][3] fp32 = (x px, y px of the patch with pixel centres at the integers 0 .. S - 1, depth in
 * any unit, smaller = nearer); faces [F][3] int32 vertex indices shared by the batch; face_rgb [F][3] fp32 or NULL = white;
 * light [3] fp32 on the DEVICE, the direction towards the light in (x, y, depth * depth_scale) space, or NULL = (0, 0, -1).
 * SKIPPED faces (never read out of bounds, hit nothing): an index outside [0, Nv), a vertex coordinate that is not finite,
 * area == 0 (below).  No back-face culling, no near plane (the caller marks vertices behind the camera NaN), no clipping but
 * by the pixel grid, no antialiasing, no top-left rule: a pixel on a shared edge belongs to both faces and the depth decides.
 * Everything below is in double precision from the fp32 numbers, each operation rounded on its own (no fused multiply-add),
 * in the order written; tests/_render_oracle.py restates it.  For a face (a, b, c) and a pixel centre p:
 *   E(q, s, t) = (s.x - q.x) (t.y - q.y) - (s.y - q.y) (t.x - q.x);   area = E(a, b, c);
 *   w0 = E(b, c, p), w1 = E(c, a, p), w2 = E(a, b, p);
 *   COVERED: p lies in the closed box of the three vertices, and w0, w1, w2 are all >= 0 if area > 0, all <= 0 if area < 0;
 *   depth z = ((w0 a.z + w1 b.z) + w2 c.z) / area    (affine in the patch, not perspective-correct).
 * The covering face of the smallest z keeps the pixel (comparison `z < best`: a z that is NaN or +inf never wins); of equal z
 * the smallest face index.  Colour, flat per face: with e1 = b - a, e2 = c - a in (x, y, depth * depth_scale), n = e1 x e2
 * negated if n.z > 0, |n| = sqrt((n.x^2 + n.y^2) + n.z^2), l = light / |light|, d = ((n.x / |n|) l.x + (n.y / |n|) l.y) +
 * (n.z / |n|) l.z:   rgb = fp32(face_rgb * (ambient + (1 - ambient) * (d > 0 ? d : 0))), rounded once.
 * ambient = 1: pure face colours; ambient < 1 on white faces: an untextured shaded body.
 * Outputs, every element written by every call: img [B][3][S][S] (background where nothing was hit), mask [B][1][S][S]
 * (1 / 0); zbuf [B][S][S] = fp32(z), +inf where nothing was hit, or NULL; face_id [B][S][S] int32, -1 where nothing was hit,
 * or NULL.  workspace: xas_mesh_render_workspace_bytes(B, F, S) bytes, 16-byte aligned (per face and sample 8 bytes of pixel
 * box and a 64-byte record); may be NULL when B * F == 0.
 * Two launches: one thread per (sample, face) writes box and record; one workgroup of 256 threads per (sample, 16 x 16 tile)
 * reads the boxes 256 at a time, compacts the records whose box meets the tile into LDS in face order and lets every thread
 * resolve its pixel against them before the next 256: no capacity to overflow.  F == 0 writes the background, B == 0
 * nothing.  1 <= S <= 4096, B <= 65535, B*F < 2^31; status 1 and xas_last_error() on any other shape or a null required buffer. */
size_t xas_mesh_render_workspace_bytes(int B, int F, int S);
int xas_mesh_render(const float* verts, const int* faces, const float* face_rgb, const float* light, float ambient,
                    float depth_scale, float background, int B, int Nv, int F, int S, float* img, float* mask, float* zbuf,
                    int* face_id, void* workspace, void* stream);

/* Pose metrics, replaces metrics.py:5-244 (numpy, per-sample SVD on the host).
 * pred, gt [N][K][3]; both are divided by in_div on load (eval.py:52-53 passes mm / 1000 for PCK / AUC);
 * mask [N][K] (0/1) or NULL = all visible.  Outputs (each may be NULL):
 *   err [3][N][K]       per-joint error * mask under alignment none / scale / procrustes
 *   aligned [2][N][K][3] the scale- and procrustes-aligned predictions
 *   pck [N][K]          100 where err[pck_align] < pck_threshold, * mask
 *   auc_hits [N][31]    visible joints with err[pck_align] < linspace(0, 0.15, 31)[t]
 * 3 <= K <= 64. */
int xas_pose_metrics(const float* pred, const float* gt, const unsigned char* mask, int N, int K, float in_div,
                     int pck_align, float pck_threshold, float* err, float* aligned, float* pck, int* auc_hits,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
