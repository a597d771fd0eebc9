"""Evaluation-path ops over the C ABI: hypothesis selection, triangulation, pose metrics (no autograd: eval runs
under torch.no_grad, eval.py:393), and the one op of the same geometry that training differentiates, multiview_consistency.
Everything returns device tensors; nothing here synchronises with the host."""
import ctypes

import torch

from ._lib import call, ptr
from .ops_head import GEO_NORM, GEO_PATCH

GEO_IMAGE = 8
EVAL_CONFIDENT, EVAL_SWITCH_ALL, EVAL_GT_NORMALISED, EVAL_NO_SWITCH = 1, 2, 4, 8
SWITCH_PAIRS = ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13))     # eval_utils.py:8

_perm_cache = {}


def switch_perm(num_kp, pairs, device):
    key = (num_kp, tuple(tuple(p) for p in pairs), str(device))
    if key not in _perm_cache:
        perm = list(range(num_kp))
        for a, b in pairs:
            perm[a], perm[b] = b, a
        _perm_cache[key] = torch.tensor(perm, dtype=torch.int32, device=device)
    return _perm_cache[key]


def _f32(t):
    return t.detach().contiguous().float()


def eval_select(kps, joints, pairs=SWITCH_PAIRS, image_size=256.0, mode='best', switch_all=False, gt_normalised=False,
                want=('sel3d', 'sel2d', 'err2d', 'swapped'), no_switch=False):
    """kps [B,Hy,K,C], joints [B,K,C] -> dict of the requested outputs (eval.py:117-148 for one camera).  `no_switch`: the
    partner test is skipped and every joint kept as given (for joints that multiview_resolve has already resolved)."""
    if mode not in ('best', 'confident'):
        raise ValueError('Unknown mode: {}'.format(mode))
    kps, joints = _f32(kps), _f32(joints)
    B, Hy, K, C = kps.shape
    if joints.shape != (B, K, C):
        raise RuntimeError('eval_select: joints %s do not match kps %s' % (tuple(joints.shape), tuple(kps.shape)))
    dev = kps.device
    flags = (EVAL_CONFIDENT if (mode == 'confident' or Hy == 1) else 0) | (EVAL_SWITCH_ALL if switch_all else 0) | \
        (EVAL_GT_NORMALISED if gt_normalised else 0) | (EVAL_NO_SWITCH if no_switch else 0)
    out = {}
    if 'sel3d' in want:
        out['sel3d'] = torch.empty(B, K, C, device=dev)
    if 'sel2d' in want:
        out['sel2d'] = torch.empty(B, K, 2, device=dev)
    if 'err2d' in want:
        out['err2d'] = torch.empty(B, device=dev)
    if 'swapped' in want:
        out['swapped'] = torch.empty(B, K, 1, device=dev, dtype=torch.uint8)
    call('xas_eval_select', ptr(kps), ptr(joints), ptr(switch_perm(K, pairs, dev)), B, Hy, K, C, float(image_size), flags,
         ptr(out.get('sel3d')), ptr(out.get('sel2d')), ptr(out.get('err2d')), ptr(out.get('swapped')))
    if 'swapped' in out:
        out['swapped'] = out['swapped'].bool()
    return out


def patch_to_image(kps, trans_image, pelvis, image_size=256.0, rect_width=2000.0, is_norm=True):
    """[B,K,3] normalised patch coordinates -> image (u px, v px, depth mm).  modules/util.py:61-83."""
    kps = _f32(kps).unsqueeze(1)
    B, _, K, _ = kps.shape
    ti, pv = _f32(trans_image), _f32(pelvis)
    out = torch.empty_like(kps)
    call('xas_patch_to_world_fwd', ptr(kps), ptr(ti), None, ptr(pv), None, None, B, 1, K, float(image_size),
         float(rect_width), (GEO_NORM if is_norm else 0) | GEO_PATCH | GEO_IMAGE, ptr(out))
    return out.squeeze(1)


def projection_matrix(k_mat, rot_world, trans_world):
    """P [B,3,4] = K [R | t].  modules/util.py:188."""
    km, rw, tw = _f32(k_mat), _f32(rot_world), _f32(trans_world)
    P = torch.empty(km.shape[0], 3, 4, device=km.device)
    call('xas_projection_matrix', ptr(km), ptr(rw), ptr(tw), km.shape[0], ptr(P))
    return P


def triangulate_dlt(points, pmat):
    """points [B,V,K,3] (u, v, weight), pmat [B,V,3,4] -> [B,K,4] (X/w, mean weight).  modules/util.py:198-230."""
    points, pmat = _f32(points), _f32(pmat)
    B, V, K, _ = points.shape
    if pmat.shape != (B, V, 3, 4):
        raise RuntimeError('triangulate_dlt: projection matrices %s do not match points %s' % (tuple(pmat.shape), tuple(points.shape)))
    out = torch.empty(B, K, 4, device=points.device)
    call('xas_triangulate_dlt', ptr(points), ptr(pmat), B, V, K, ptr(out))
    return out


# Default inlier threshold of the robust triangulation, in pixels of the full-resolution image.  Argued, not measured
# (DESIGN.md 4): a 256-px patch covers a roughly 1000-px HM36 frame, so 20 image px are about 5 patch px, a little over one
# cell of the D = 64 heat-map (4 patch px per cell).
TRI_ROBUST_PX = 20.0
TRI_MAX_VIEWS = 6        # xas_hip.h XAS_TRI_MAX_VIEWS


def triangulate_robust(points, pmat, threshold_px=TRI_ROBUST_PX, want=('inliers', 'resid')):
    """points [B,V,K,3] (u, v, weight), pmat [B,V,3,4] -> dict: xyzw [B,K,4] (the DLT over the largest set of views that agree
    within threshold_px, mean weight of those views), inliers [B,K] uint8 (bit v = view v used, 0 = no two views agreed and
    all valid views were used), resid [B,K] (RMS reprojection residual of the result over the views used, px)."""
    points, pmat = _f32(points), _f32(pmat)
    B, V, K, _ = points.shape
    if pmat.shape != (B, V, 3, 4):
        raise RuntimeError('triangulate_robust: projection matrices %s do not match points %s' % (tuple(pmat.shape), tuple(points.shape)))
    dev = points.device
    out = {'xyzw': torch.empty(B, K, 4, device=dev)}
    if 'inliers' in want:
        out['inliers'] = torch.empty(B, K, device=dev, dtype=torch.uint8)
    if 'resid' in want:
        out['resid'] = torch.empty(B, K, device=dev)
    call('xas_triangulate_robust', ptr(points), ptr(pmat), B, V, K, float(threshold_px), ptr(out['xyzw']),
         ptr(out.get('inliers')), ptr(out.get('resid')))
    return out


REFINE_WEIGHTED = 1      # xas_hip.h XAS_REFINE_WEIGHTED


def _solver_inputs(name, points, pmat, init, views, batch='B'):
    """The inputs that the four solvers share (triangulate_refine, triangulate_skeleton, ops_calib, ops_track): points
    [B,V,K,3], pmat [B,V,3,4] and init [B,K,4] as contiguous float32, views [B,K] uint8 or None -> them and B, V, K.  `batch` is
    the letter the caller's documentation has for B."""
    points, pmat, init = _f32(points), _f32(pmat), _f32(init)
    B, V, K, _ = points.shape
    if pmat.shape != (B, V, 3, 4):
        raise RuntimeError('%s: projection matrices %s do not match points %s' % (name, tuple(pmat.shape), tuple(points.shape)))
    if init.shape != (B, K, 4):
        raise RuntimeError('%s: start points %s do not match points %s' % (name, tuple(init.shape), tuple(points.shape)))
    if views is not None:
        if views.shape != (B, K) or views.dtype != torch.uint8:
            raise RuntimeError('%s: views %s %s are not the [%s,K] uint8 masks of points %s' % (
                name, tuple(views.shape), views.dtype, batch, tuple(points.shape)))
        views = views.contiguous()
    return points, pmat, init, views, B, V, K


def _sorted(order, *tensors):
    """Every tensor (None stays None) with its samples in the order `order`, for a kernel that takes them sorted by a host table."""
    return tuple(None if t is None else t[order].contiguous() for t in tensors)


def _scatter(order, t):
    """The result t of such a kernel put back in the order given."""
    out = torch.empty_like(t)
    out[order] = t
    return out


def triangulate_refine(points, pmat, init, views=None, weighted=False, huber_px=0.0, max_iter=20, want=('resid',)):
    """Levenberg-Marquardt on the reprojection error from a triangulated point (xas_triangulate_refine).  points [B,V,K,3]
    (u, v, weight), pmat [B,V,3,4], init [B,K,4] (triangulate_dlt, or xyzw of triangulate_robust), views [B,K] uint8 (inliers of
    triangulate_robust) or None = all valid views.  `weighted`: every view's residual is scaled by its weight (1 / sigma in
    pixels makes the cost a likelihood and cov mm^2); `huber_px` > 0: Huber's loss, in the unit of the scaled residual.
    -> dict: xyzw [B,K,4] always; resid [B,K,2] (RMS pixel residual over the views used, before and after), cov [B,K,6] (upper
    triangle of the inverse Gauss-Newton Hessian), status [B,K] uint8 (0 converged, 1 out of trials, 2 passed through) as
    requested."""
    points, pmat, init, views, B, V, K = _solver_inputs('triangulate_refine', points, pmat, init, views)
    dev = points.device
    out = {'xyzw': torch.empty(B, K, 4, device=dev)}
    if 'resid' in want:
        out['resid'] = torch.empty(B, K, 2, device=dev)
    if 'cov' in want:
        out['cov'] = torch.empty(B, K, 6, device=dev)
    if 'status' in want:
        out['status'] = torch.empty(B, K, device=dev, dtype=torch.uint8)
    call('xas_triangulate_refine', ptr(points), ptr(pmat), ptr(init), ptr(views), B, V, K, REFINE_WEIGHTED if weighted else 0,
         float(huber_px), int(max_iter), ptr(out['xyzw']), ptr(out.get('resid')), ptr(out.get('cov')), ptr(out.get('status')))
    return out


# Left/right limb pairs (far_a, near_a, far_b, near_b) of the 18-joint skeleton: the limbs of the training loss's symmetry term
# (modules/base_losses/loss_func.py: _LIMB_FAR / _LIMB_NEAR, upper and lower arm and leg), each paired with its mirror.
SYM_LIMBS = ((16, 15, 13, 12), (15, 14, 12, 11), (3, 2, 6, 5), (2, 1, 5, 4))
SKEL_MAX_JOINTS, SKEL_MAX_LIMBS = 24, 16      # xas_hip.h XAS_SKEL_MAX_JOINTS, XAS_SKEL_MAX_LIMBS
TRI_SYM_W = 0.1          # default --tri-sym, px^2 per mm^2: at ~0.3 px per mm a 1 mm limb mismatch weighs about like a 1 px residual


def triangulate_skeleton(points, pmat, init, views=None, limbs=SYM_LIMBS, weighted=False, huber_px=0.0, sym_w=TRI_SYM_W, max_iter=20,
                         want=('resid',)):
    """triangulate_refine with the joints of a sample coupled by left/right limb symmetry (xas_triangulate_skeleton): one
    Levenberg-Marquardt problem per sample on  sum of rho(reprojection residuals) + sym_w * sum over the limb pairs of
    (|limb a| - |limb b|)^2.  points, pmat, init, views, weighted, huber_px as for triangulate_refine; limbs = rows
    (far_a, near_a, far_b, near_b) of joint indices; sym_w in px^2 per mm^2.  A joint that triangulate_refine would pass through
    is fixed (init bit for bit) and switches off every limb pair it belongs to.
    -> dict: xyzw [B,K,4] always; resid [B,K,2] (RMS pixel residual before and after; NaN for a fixed joint), sym [B,L,2]
    (|limb a| - |limb b| in mm before and after; NaN where the pair is off), cost [B,2], status [B,K] uint8 (0 the sample
    converged, 1 out of trials, 2 fixed joint) as requested."""
    points, pmat, init, views, B, V, K = _solver_inputs('triangulate_skeleton', points, pmat, init, views)
    limbs = [tuple(int(j) for j in row) for row in limbs]
    if any(len(row) != 4 for row in limbs):
        raise RuntimeError('triangulate_skeleton: every limb pair is (far_a, near_a, far_b, near_b); got %s' % (limbs,))
    L = len(limbs)
    table = (ctypes.c_int * max(4 * L, 1))(*[j for row in limbs for j in row])      # read by the host before the launch
    dev = points.device
    out = {'xyzw': torch.empty(B, K, 4, device=dev)}
    if 'resid' in want:
        out['resid'] = torch.empty(B, K, 2, device=dev)
    if 'sym' in want:
        out['sym'] = torch.empty(B, L, 2, device=dev)
    if 'cost' in want:
        out['cost'] = torch.empty(B, 2, device=dev)
    if 'status' in want:
        out['status'] = torch.empty(B, K, device=dev, dtype=torch.uint8)
    call('xas_triangulate_skeleton', ptr(points), ptr(pmat), ptr(init), ptr(views), table if L else None, B, V, K, L,
         REFINE_WEIGHTED if weighted else 0, float(huber_px), float(sym_w), int(max_iter), ptr(out['xyzw']), ptr(out.get('resid')),
         ptr(out.get('sym')), ptr(out.get('cost')), ptr(out.get('status')))
    return out


# Defaults of the volumetric fusion.  A starting point read off the cell size, NOT a tuned choice: at the shipped rig one
# heat-map cell is about 31 mm (2000 mm over 64 cells), so 800 mm over 16 voxels gives 50 mm voxels at the first level and 25 mm
# at the second.  No accuracy figure stands behind any of the three.
TRI_VOL_G = 16
TRI_VOL_LEVELS = 2
TRI_VOL_SIDE_MM = 800.0


def triangulate_volume(logits_by_view, chan, trans_image, k_mat, pelvis, rot_world, trans_world, init, views=None, weight=None,
                       G=TRI_VOL_G, levels=TRI_VOL_LEVELS, side_mm=TRI_VOL_SIDE_MM, beta=1.0, out_penalty=1.0, image_size=256.0,
                       rect_width=2000.0, want=()):
    """Volumetric fusion of the views' heat-map cubes round a triangulated point (xas_triangulate_volume): the product of the
    views' distributions over a G^3 voxel grid of side side_mm round `init`, refined `levels` times at half the side, and its
    soft-argmax in world mm.  logits_by_view: V tensors [B, K*D, D, D] with NHWC storage (a detector's forward_logits), which
    stay where they are: only their addresses are passed.  chan [V,B,K] int32 or None: the heat-map channel view v reads for
    joint k.  trans_image [V,B,2,3], k_mat [V,B,3,3], pelvis [V,B,3], rot_world [V,B,3,3], trans_world [V,B,3]; init [B,K,3]
    (or [B,K,4]: the first three); views [B,K] uint8 (bit v = view v takes part; None = all); weight [V,B,K] or None = 1.
    -> dict: xyz [B,K,3] always; cov [B,K,6] (mm^2: xx xy xz yy yz zz) and status [B,K] uint8 (0 fused, 1 passed through, 2
    fused with the mode on a face of the grid, 3 a logit that is not finite: passed through) as requested."""
    from .ops_head import _nhwc_storage
    V = len(logits_by_view)
    if not 1 <= V <= TRI_MAX_VIEWS:
        raise RuntimeError('triangulate_volume: V=%d views (needs 1 <= V <= XAS_TRI_MAX_VIEWS = %d)' % (V, TRI_MAX_VIEWS))
    init = _f32(init[..., :3])
    B, K, _ = init.shape
    cubes = []
    for v, t in enumerate(logits_by_view):
        if t.dim() != 4 or t.dtype != torch.float32 or t.shape[0] != B or t.shape[1] % K or not (t.shape[1] // K == t.shape[2] == t.shape[3]):
            raise RuntimeError('triangulate_volume: logits of view %d are %s %s, not float32 [B=%d, K*D, D, D] with K=%d' % (
                v, tuple(t.shape), t.dtype, B, K))
        cubes.append(_nhwc_storage(t.detach()))
    D = cubes[0].shape[2]
    if any(t.shape != cubes[0].shape for t in cubes):
        raise RuntimeError('triangulate_volume: the views\' logits differ in shape: %s' % ([tuple(t.shape) for t in cubes],))
    cams = [_f32(t) for t in (trans_image, k_mat, pelvis, rot_world, trans_world)]
    for t, tail, name in zip(cams, ((2, 3), (3, 3), (3,), (3, 3), (3,)), ('trans_image', 'k_mat', 'pelvis', 'rot_world', 'trans_world')):
        if t.shape != (V, B) + tail:
            raise RuntimeError('triangulate_volume: %s %s is not [V=%d, B=%d, %s]' % (name, tuple(t.shape), V, B, ', '.join(map(str, tail))))
    if chan is not None:
        if chan.shape != (V, B, K) or chan.dtype != torch.int32:
            raise RuntimeError('triangulate_volume: chan %s %s is not the [V,B,K] int32 channel table' % (tuple(chan.shape), chan.dtype))
        chan = chan.contiguous()
    if views is not None:
        if views.shape != (B, K) or views.dtype != torch.uint8:
            raise RuntimeError('triangulate_volume: views %s %s are not the [B,K] uint8 masks of init %s' % (
                tuple(views.shape), views.dtype, tuple(init.shape)))
        views = views.contiguous()
    if weight is not None:
        weight = _f32(weight)
        if weight.shape != (V, B, K):
            raise RuntimeError('triangulate_volume: weight %s is not [V,B,K]' % (tuple(weight.shape),))
    dev = init.device
    out = {'xyz': torch.empty(B, K, 3, device=dev)}
    if 'cov' in want:
        out['cov'] = torch.empty(B, K, 6, device=dev)
    if 'status' in want:
        out['status'] = torch.empty(B, K, device=dev, dtype=torch.uint8)
    table = (ctypes.c_void_p * V)(*[ptr(t) for t in cubes])           # read by the host before the launch
    call('xas_triangulate_volume', table, ptr(chan), *[ptr(t) for t in cams], ptr(init), ptr(views), ptr(weight), B, V, K, D, int(G),
         int(levels), float(side_mm), float(beta), float(out_penalty), float(image_size), float(rect_width), ptr(out['xyz']),
         ptr(out.get('cov')), ptr(out.get('status')))
    return out


def multiview_resolve(points, pmat, kps, world, pairs=SWITCH_PAIRS, gt=None, image_size=256.0,
                      want=('xyzw', 'swap', 'hyp', 'named')):
    """Left/right exchange and depth hypothesis of every view from the agreement of the views (xas_multiview_resolve).
    points [B,V,K,3] (u, v, weight; one per joint, the hypotheses share x and y), pmat [B,V,3,4], kps and world [B,V,Hy,K,3]
    (patch-normalised joints and their single-view world points), gt [B,V,K,3] patch pixels or None (only names the pair).
    -> dict: sel [B,V,K,3] always; xyzw [B,K,4], swap [B,K] uint8 (bit v = view v's joint was taken from its partner),
    hyp [B,V,K] uint8, named [B,K] uint8 (only with gt) as requested."""
    points, pmat, kps, world = _f32(points), _f32(pmat), _f32(kps), _f32(world)
    B, V, K, _ = points.shape
    if pmat.shape != (B, V, 3, 4):
        raise RuntimeError('multiview_resolve: projection matrices %s do not match points %s' % (tuple(pmat.shape), tuple(points.shape)))
    if kps.dim() != 5 or kps.shape[:2] != (B, V) or kps.shape[3:] != (K, 3):
        raise RuntimeError('multiview_resolve: kps %s do not match points %s' % (tuple(kps.shape), tuple(points.shape)))
    if world.shape != kps.shape:
        raise RuntimeError('multiview_resolve: world %s and kps %s differ' % (tuple(world.shape), tuple(kps.shape)))
    if gt is not None:
        gt = _f32(gt)
        if gt.shape != (B, V, K, 3):
            raise RuntimeError('multiview_resolve: labels %s do not match points %s' % (tuple(gt.shape), tuple(points.shape)))
    Hy, dev = kps.shape[2], points.device
    out = {'sel': torch.empty(B, V, K, 3, device=dev)}
    if 'xyzw' in want:
        out['xyzw'] = torch.empty(B, K, 4, device=dev)
    if 'swap' in want:
        out['swap'] = torch.empty(B, K, device=dev, dtype=torch.uint8)
    if 'hyp' in want:
        out['hyp'] = torch.empty(B, V, K, device=dev, dtype=torch.uint8)
    if 'named' in want and gt is not None:
        out['named'] = torch.empty(B, K, device=dev, dtype=torch.uint8)
    call('xas_multiview_resolve', ptr(points), ptr(pmat), ptr(kps), ptr(world), ptr(switch_perm(K, pairs, dev)), ptr(gt),
         B, V, Hy, K, float(image_size), ptr(out['sel']), ptr(out.get('xyzw')), ptr(out.get('swap')), ptr(out.get('hyp')),
         ptr(out.get('named')))
    return out


MV_DETACH_TARGET = 1     # xas_hip.h XAS_MV_DETACH_TARGET


class _MultiviewConsistency(torch.autograd.Function):
    """xas_multiview_consistency_fwd / _bwd: the one part of this module that training differentiates."""

    @staticmethod
    def forward(ctx, kps_xy, world, trans_image, pmat, weight, image_size, huber_px, flags):
        B, V, Hy, K = world.shape[:4]
        dev = kps_xy.device
        reproj, depth = torch.empty(B, K, device=dev), torch.empty(B, K, device=dev)
        xyz = torch.empty(B, K, 3, device=dev)
        hsel = torch.empty(B, V, K, device=dev, dtype=torch.int32)
        status = torch.empty(B, K, device=dev, dtype=torch.uint8)
        call('xas_multiview_consistency_fwd', ptr(kps_xy), ptr(trans_image), ptr(world), ptr(pmat), ptr(weight), B, V, Hy, K,
             image_size, huber_px, flags, ptr(reproj), ptr(depth), ptr(xyz), ptr(hsel), ptr(status))
        ctx.save_for_backward(kps_xy, world, trans_image, pmat, weight)
        ctx.scalars = (image_size, huber_px, flags)
        ctx.mark_non_differentiable(xyz, hsel, status)
        return reproj, depth, xyz, hsel, status

    @staticmethod
    def backward(ctx, g_reproj, g_depth, *_):
        kps_xy, world, trans_image, pmat, weight = ctx.saved_tensors
        B, V, Hy, K = world.shape[:4]
        zero = lambda g: torch.zeros(B, K, device=kps_xy.device) if g is None else g.contiguous().float()
        g_reproj, g_depth = zero(g_reproj), zero(g_depth)
        grad_xy, grad_world = torch.empty_like(kps_xy), torch.empty_like(world)      # the kernel writes every entry
        call('xas_multiview_consistency_bwd', ptr(kps_xy), ptr(trans_image), ptr(world), ptr(pmat), ptr(weight), ptr(g_reproj),
             ptr(g_depth), B, V, Hy, K, *ctx.scalars, ptr(grad_xy), ptr(grad_world))
        return grad_xy, grad_world, None, None, None, None, None, None


def multiview_consistency(kps_xy, trans_image, world, pmat, weight=None, image_size=256.0, huber_px=0.0, detach_target=False):
    """Multi-view consistency of the training step (xas_multiview_consistency_fwd / _bwd, two launches).  kps_xy [B,V,K,2]
    hypothesis 0's normalised patch x, y of every camera, trans_image [B,V,2,3], world [B,V,Hy,K,3] every hypothesis's single-view
    world point in mm, pmat [B,V,3,4], weight [B,V,K] or None = every view counts 1 (not finite or not positive: the view is
    invalid for that joint).  X = the DLT over the valid views.
    -> (reproj [B,K]: mean over the valid views of the squared (huber_px > 0: Huber's) pixel distance between X's reprojection
    and the view's point; depth [B,K]: mean squared distance in mm^2 between X and the view's nearest hypothesis; xyz [B,K,3] = X;
    status [B,K] uint8, 0 or 2 = passed through: fewer than two valid views, X not finite or behind a valid view - both terms and
    every gradient exactly 0, xyz NaN).  Gradients go to kps_xy and world only; with `detach_target` X is a constant of the
    backward pass."""
    kps_xy, world = kps_xy.contiguous().float(), world.contiguous().float()
    trans_image, pmat = _f32(trans_image), _f32(pmat)
    if kps_xy.dim() != 4 or kps_xy.shape[-1] != 2:
        raise RuntimeError('multiview_consistency: kps_xy %s is not [B,V,K,2]' % (tuple(kps_xy.shape),))
    B, V, K, _ = kps_xy.shape
    if world.dim() != 5 or world.shape[:2] != (B, V) or world.shape[3:] != (K, 3):
        raise RuntimeError('multiview_consistency: world %s does not match kps_xy %s' % (tuple(world.shape), tuple(kps_xy.shape)))
    if trans_image.shape != (B, V, 2, 3):
        raise RuntimeError('multiview_consistency: crop affines %s do not match kps_xy %s' % (tuple(trans_image.shape), tuple(kps_xy.shape)))
    if pmat.shape != (B, V, 3, 4):
        raise RuntimeError('multiview_consistency: projection matrices %s do not match kps_xy %s' % (tuple(pmat.shape), tuple(kps_xy.shape)))
    if weight is not None:
        weight = _f32(weight)
        if weight.shape != (B, V, K):
            raise RuntimeError('multiview_consistency: weights %s do not match kps_xy %s' % (tuple(weight.shape), tuple(kps_xy.shape)))
    reproj, depth, xyz, _, status = _MultiviewConsistency.apply(kps_xy, world, trans_image, pmat, weight, float(image_size),
                                                                float(huber_px), MV_DETACH_TARGET if detach_target else 0)
    return reproj, depth, xyz, status


def pose_metrics(pred, gt, mask=None, in_div=1.0, pck_align=0, pck_threshold=0.15,
                 want=('err', 'pck', 'auc_hits')):
    """pred, gt [N,K,3] -> dict: err [3,N,K] (none / scale / procrustes), aligned [2,N,K,3], pck [N,K],
    auc_hits [N,31] int32 (metrics.py:5-244)."""
    pred, gt = _f32(pred), _f32(gt)
    N, K, _ = pred.shape
    if gt.shape != pred.shape:
        raise RuntimeError('pose_metrics: pred %s and gt %s differ' % (tuple(pred.shape), tuple(gt.shape)))
    dev = pred.device
    m = None
    if mask is not None:
        m = torch.as_tensor(mask, device=dev).to(torch.uint8).contiguous()
    out = {}
    if 'err' in want:
        out['err'] = torch.empty(3, N, K, device=dev)
    if 'aligned' in want:
        out['aligned'] = torch.empty(2, N, K, 3, device=dev)
    if 'pck' in want:
        out['pck'] = torch.empty(N, K, device=dev)
    if 'auc_hits' in want:
        out['auc_hits'] = torch.empty(N, 31, device=dev, dtype=torch.int32)
    call('xas_pose_metrics', ptr(pred), ptr(gt), ptr(m), N, K, float(in_div), int(pck_align), float(pck_threshold),
         ptr(out.get('err')), ptr(out.get('aligned')), ptr(out.get('pck')), ptr(out.get('auc_hits')))
    return out
