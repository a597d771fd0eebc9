"""Soft-argmax head, patch->world / world->patch geometry and line-mask renderer as autograd ops over the C ABI."""
import torch

from . import _lib
from ._lib import call, ptr, query

HEAD_STATS = 16
peak_probe = None        # measurement hook (tests): called with the int64 depth-peak indices [B,K,Hy] of every head forward
GEO_NORM, GEO_MONO, GEO_PATCH = 1, 2, 4
GEO_IMAGE, GEO_WORLD = 8, 16


def _nhwc_storage(logits):
    """[B,C,H,W] logical tensor -> the same tensor with NHWC (channels_last) storage."""
    if logits.dim() != 4:
        raise RuntimeError('logits must be [B, K*D, H, W]')
    if not logits.is_contiguous(memory_format=torch.channels_last):
        logits = logits.contiguous(memory_format=torch.channels_last)
    return logits


def check_patch_size(x, depth_dim, who):
    """The detectors' heat-map is a quarter of the input patch per side and must be a cube: depth_dim == S / 4."""
    if x.dim() != 4 or x.shape[-1] != x.shape[-2] or x.shape[-1] != 4 * depth_dim:
        raise RuntimeError('%s(depth_dim=%d) takes square input patches of side 4 * depth_dim = %d, got input %s: build the '
                           'detector with depth_dim = patch size / 4 (a multiple of 4, at most 128: patches up to 512)'
                           % (who, depth_dim, 4 * depth_dim, tuple(x.shape)))


class _SoftArgmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, num_kp, num_hypo, neighbor, groups):
        from . import ops_nn
        logits_in = logits
        logits_tail = _nhwc_storage(logits)
        logits = ops_nn._full(logits_tail)               # prefix pass (ops_nn): prefix + graph images in one launch
        B, C, H, W = logits.shape
        D = C // num_kp
        if not (C == num_kp * D and D == H == W):
            raise RuntimeError('soft-argmax head needs a heat-map cube D == H == W with D a multiple of 4 in [4,128] '
                               '(got C=%d K=%d H=%d W=%d)' % (C, num_kp, H, W))
        dev = logits.device
        kps = torch.empty(B, num_hypo, num_kp, 3, device=dev, dtype=torch.float32)
        z_idx = torch.empty(B, num_kp, num_hypo, device=dev, dtype=torch.int64)
        dmap = torch.empty(groups, num_kp, D, device=dev, dtype=torch.float32)
        stats = torch.empty(B, num_kp, HEAD_STATS, device=dev, dtype=torch.float32)
        pre = getattr(logits_in, '_xas_head', None)      # first-pass records from the final convolution's epilogue (ops_nn._Conv2d)
        if pre is not None and pre[2] == logits_in._version and pre[0].shape[0] == B and pre[0].shape[2] == num_kp:
            ops_nn.head_stats['fused'] += 1
            call('xas_head_softargmax_from_partials', ptr(pre[0]), B, num_kp, D, pre[1], num_hypo, neighbor, ptr(kps), ptr(z_idx),
                 ptr(dmap), groups, ptr(stats))
        else:
            ops_nn.head_stats['separate'] += 1
            ws = torch.empty(query('xas_head_workspace_floats', B, num_kp, D), device=dev, dtype=torch.float32)
            call('xas_head_softargmax_fwd', ptr(logits), B, num_kp, D, num_hypo, neighbor, ptr(kps), ptr(z_idx),
                 ptr(dmap), groups, ptr(stats), ptr(ws))
        if peak_probe is not None:
            peak_probe(z_idx.clone())
        s = B - logits_tail.shape[0]                     # images of the no-grad prefix (0 outside a prefix pass)
        kps_prefix = kps[:s] if s else kps[:0]
        kps, z_idx_all = (kps[s:], z_idx) if s else (kps, z_idx)
        ctx.save_for_backward(logits_tail, stats[s:] if s else stats, z_idx[s:] if s else z_idx)
        ctx.cfg = (num_kp, D, num_hypo, neighbor)
        ctx.mark_non_differentiable(z_idx_all, dmap, kps_prefix)
        return kps, dmap, z_idx_all, kps_prefix

    @staticmethod
    def backward(ctx, g_kps, _g_dmap, _g_idx, _g_prefix=None):
        logits, stats, z_idx = ctx.saved_tensors
        K, D, Hy, nb = ctx.cfg
        B = logits.shape[0]
        g_kps = g_kps.contiguous()
        grad = torch.empty_like(logits)          # keeps the channels_last strides
        coef = torch.empty(B * K * (4 + D), device=logits.device, dtype=torch.float32)
        from . import ops_nn
        slot = ops_nn.grad_amax_slot(logits.device)          # max |grad|: the final conv's f16x3 gradient launches scale dy with it
        call('xas_head_softargmax_bwd_amax', ptr(logits), ptr(stats), ptr(z_idx), ptr(g_kps), B, K, D, Hy, nb,
             ptr(grad), ptr(coef), ptr(slot))
        if slot is not None:
            ops_nn.tag_grad_amax(grad, slot)
        return grad, None, None, None, None


def softargmax_multi(logits, num_kp, num_hypo, neighbor_size, groups=1):
    """-> kps [B,num_hypo,K,3], depth_prob_map [K,D] ([groups,K,D] for groups > 1: first sample of each sub-batch),
    z_idx [B,K,num_hypo] int64  (keypoint_detector_integral_multi.py:66-88)."""
    kps, dmap, idx, prefix = _SoftArgmax.apply(logits, num_kp, num_hypo, neighbor_size, groups)
    _last_prefix[0] = prefix
    return kps, (dmap[0] if groups == 1 else dmap), idx


_last_prefix = [None]          # joints of the no-grad prefix images of the latest call (prefix pass: KPDetector3DMulti.forward_groups)


def softargmax_single(logits, num_kp, groups=1):
    """-> kps [B,1,K,3], depth_prob_map [K,D] ([groups,K,D] for groups > 1)  (keypoint_detector_integral.py:45-65)."""
    kps, dmap, _, prefix = _SoftArgmax.apply(logits, num_kp, 1, 0, groups)
    _last_prefix[0] = prefix
    return kps, (dmap[0] if groups == 1 else dmap)


def flip_perm(flip_pairs, num_kp, device):
    """Left/right pair list ([[1, 4], [2, 5], ...], model_params.flip_pairs) -> device int32 [K] table for softargmax_flip:
    perm[a] = b and perm[b] = a for every pair, perm[k] = k for an unpaired joint.  Joints outside [0, K) and joints named
    twice are refused here, on the host: the kernel indexes the records with this table."""
    perm = list(range(num_kp))
    for pair in flip_pairs:
        a, b = (int(v) for v in pair)
        if not (0 <= a < num_kp and 0 <= b < num_kp) or a == b:
            raise RuntimeError('flip pair (%d, %d) does not name two of the %d joints' % (a, b, num_kp))
        if perm[a] != a or perm[b] != b:
            raise RuntimeError('flip pair (%d, %d): a joint has two partners' % (a, b))
        perm[a], perm[b] = b, a
    t = torch.tensor(perm, dtype=torch.int32, device=device)
    t._xas_perm_k = num_kp                            # checked: softargmax_flip does not read it back
    return t


def softargmax_flip(heatmap_2b, num_kp, num_hypo, neighbor_size, perm, groups=1):
    """Flip test: the head on the average of each image's heat-map and the mirrored, pair-swapped heat-map of its mirror.
    heatmap_2b: logits [2B, K*D, D, D] of images 0..B-1 followed by their horizontal mirrors; perm: flip_perm(...), or any
    int32 [K] tensor / sequence (checked here: every entry in [0, K)); num_hypo = 1 and neighbor_size = 0: the
    single-hypothesis head.  -> kps [B,num_hypo,K,3], depth_prob_map [K,D] ([groups,K,D] for groups > 1), z_idx [B,K,num_hypo]
    int64 (zeros for the single-hypothesis head).  Runs over the first-pass records of the final convolution's epilogue when
    the logits carry them, else over the logits.  Inference only: raises when autograd is recording."""
    from . import ops_nn
    if torch.is_grad_enabled() and heatmap_2b.requires_grad:
        raise RuntimeError('softargmax_flip is an inference path without a backward: call it under torch.no_grad()')
    if ops_nn._prefix[0]:
        raise RuntimeError('softargmax_flip does not run inside a prefix pass')
    logits = _nhwc_storage(heatmap_2b)
    B2, C, H, W = logits.shape
    D = C // num_kp
    if not (C == num_kp * D and D == H == W):
        raise RuntimeError('soft-argmax head needs a heat-map cube D == H == W with D a multiple of 4 in [4,128] '
                           '(got C=%d K=%d H=%d W=%d)' % (C, num_kp, H, W))
    if B2 < 2 or B2 % 2:
        raise RuntimeError('softargmax_flip takes the logits of B images followed by their B mirrors, got %d images' % B2)
    B = B2 // 2
    dev = logits.device
    if not isinstance(perm, torch.Tensor):
        perm = torch.as_tensor(perm)
    if getattr(perm, '_xas_perm_k', None) != num_kp:
        host = perm.detach().cpu().reshape(-1).tolist()
        if len(host) != num_kp or any(int(v) != v or not 0 <= v < num_kp for v in host):
            raise RuntimeError('softargmax_flip: perm must hold %d joint indices in [0, %d), got %s' % (num_kp, num_kp, host))
        perm = perm.to(device=dev, dtype=torch.int32).contiguous()
        perm._xas_perm_k = num_kp
    if perm.device != dev or perm.dtype != torch.int32 or not perm.is_contiguous():
        raise RuntimeError('softargmax_flip: perm must be a contiguous int32 tensor on %s' % dev)
    kps = torch.empty(B, num_hypo, num_kp, 3, device=dev, dtype=torch.float32)
    z_idx = torch.zeros(B, num_kp, num_hypo, device=dev, dtype=torch.int64)
    dmap = torch.empty(groups, num_kp, D, device=dev, dtype=torch.float32)
    pre = getattr(heatmap_2b, '_xas_head', None)     # first-pass records from the final convolution's epilogue (ops_nn._Conv2d)
    if pre is not None and pre[2] == heatmap_2b._version and pre[0].shape[0] == B2 and pre[0].shape[2] == num_kp:
        ops_nn.head_stats['fused'] += 1
        call('xas_head_softargmax_flip_from_partials', ptr(pre[0]), B, num_kp, D, pre[1], num_hypo, neighbor_size, ptr(perm),
             ptr(kps), ptr(z_idx), ptr(dmap), groups)
    else:
        ops_nn.head_stats['separate'] += 1
        ws = torch.empty(query('xas_head_workspace_floats', B2, num_kp, D), device=dev, dtype=torch.float32)
        call('xas_head_softargmax_fwd_flip', ptr(logits), B, num_kp, D, num_hypo, neighbor_size, ptr(perm), ptr(kps),
             ptr(z_idx), ptr(dmap), groups, ptr(ws))
    if peak_probe is not None:
        peak_probe(z_idx.clone())
    return kps, (dmap[0] if groups == 1 else dmap), z_idx


FLIP_MAX_IMAGES = 384      # images of one detector pass (originals + mirrors): the logit budget of modules/model.py


def detector_flip_input(det, x, flip_pairs, who):
    """What both detectors' forward_flip do before the network: the checks, the cached pair table and the mirrored pair stack.
    -> (channels_last batch [2B,C,S,S] of x and its mirrors, perm)."""
    from . import ops_nn
    check_patch_size(x, det.depth_dim, who)
    if det.training:
        raise RuntimeError('%s.forward_flip is a test-time pass: put the detector in eval() (batch norm must use its running '
                           'statistics for the mirrored images to share the batch)' % who)
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in det.parameters())):
        raise RuntimeError('%s.forward_flip is an inference path without a backward: call it under torch.no_grad()' % who)
    if 2 * x.shape[0] > FLIP_MAX_IMAGES:
        raise RuntimeError('%s.forward_flip: %d images and their mirrors exceed the %d images of one pass'
                           % (who, x.shape[0], FLIP_MAX_IMAGES))
    key = (tuple(tuple(int(v) for v in p) for p in flip_pairs), str(x.device))
    if getattr(det, '_flip_key', None) != key:         # uploaded once per (pairs, device), as GCNDiscriminator_base._bone_index
        det._flip_perm = flip_perm(flip_pairs, det.num_kp, x.device)
        det._flip_key = key
    return ops_nn.mirror_pair_nchw(x), det._flip_perm


HEAD_SPREAD = 5            # xas_hip.h XAS_HEAD_SPREAD: (E w, E h, Var w, Var h, Cov(w, h)) in heat-map cells


def heatmap_spread(logits, num_kp):
    """Mean and covariance of every joint's x-y soft-max marginal: logits [B, K*D, D, D] -> [B, K, 5] =
    (E w, E h, Var w, Var h, Cov(w, h)) in heat-map cells (xas_head_spread: one streaming pass, fixed reduction order).
    The spatial confidence of a view; no reference counterpart and no backward: the result records no graph."""
    logits = _nhwc_storage(logits.detach())
    B, C, H, W = logits.shape
    D = C // num_kp
    if not (C == num_kp * D and D == H == W):
        raise RuntimeError('soft-argmax head needs a heat-map cube D == H == W with D a multiple of 4 in [4,128] '
                           '(got C=%d K=%d H=%d W=%d)' % (C, num_kp, H, W))
    dev = logits.device
    spread = torch.empty(B, num_kp, HEAD_SPREAD, device=dev, dtype=torch.float32)
    ws = torch.empty(query('xas_head_spread_workspace_floats', B, num_kp, D), device=dev, dtype=torch.float32)
    call('xas_head_spread', ptr(logits), B, num_kp, D, ptr(spread), ptr(ws))
    return spread


def spread_flip(spread_2b, perm, W):
    """Spread of the flip test's averaged heat-map from the spreads [2B, K, 5] of the B images and their B mirrors
    (heatmap_spread of the batch softargmax_flip takes): the mirror turns E w into W - 1 - E w and Cov into -Cov and joint k
    takes joint perm[k]; the half-half mixture of two distributions has mean (ua + ub) / 2, variance
    (Va + Vb) / 2 + (ua - ub)^2 / 4 and covariance (Ca + Cb) / 2 + (uwa - uwb)(uha - uhb) / 4.  -> [B, K, 5]."""
    if spread_2b.dim() != 3 or spread_2b.shape[0] % 2 or spread_2b.shape[-1] != HEAD_SPREAD:
        raise RuntimeError('spread_flip takes the spreads [2B, K, 5] of B images followed by their B mirrors, got %s'
                           % (tuple(spread_2b.shape),))
    B = spread_2b.shape[0] // 2
    if not isinstance(perm, torch.Tensor):
        perm = torch.as_tensor(perm)
    a, m = spread_2b[:B], spread_2b[B:][:, perm.to(spread_2b.device).long()]
    uw_m = (W - 1) - m[..., 0]
    dw, dh = a[..., 0] - uw_m, a[..., 1] - m[..., 1]
    return torch.stack([0.5 * (a[..., 0] + uw_m), 0.5 * (a[..., 1] + m[..., 1]),
                        0.5 * (a[..., 2] + m[..., 2]) + 0.25 * dw * dw,
                        0.5 * (a[..., 3] + m[..., 3]) + 0.25 * dh * dh,
                        0.5 * (a[..., 4] - m[..., 4]) + 0.25 * dw * dh], dim=-1)


def detector_spread(det, heatmap, flip_pairs):
    """What both detectors' forward_spread do after the head: the spread of the heat-map the head ran on (with flip_pairs
    the 2B-image batch of forward_flip and its averaged heat-map)."""
    s = heatmap_spread(heatmap, det.num_kp)
    return s if flip_pairs is None else spread_flip(s, det._flip_perm, det.depth_dim)


class _PatchToWorld(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kps, ti, km, pv, rw, tw, image_size, rect_width, flags):
        kps = kps.contiguous()
        B, Hy, K, _ = kps.shape
        cams = [t.contiguous().float() for t in (ti, km, pv, rw, tw)]
        world = torch.empty_like(kps)
        call('xas_patch_to_world_fwd', ptr(kps), *[ptr(c) for c in cams], B, Hy, K, float(image_size),
             float(rect_width), flags, ptr(world))
        ctx.save_for_backward(kps, *cams)
        ctx.cfg = (float(image_size), float(rect_width), flags)
        return world

    @staticmethod
    def backward(ctx, gw):
        kps, *cams = ctx.saved_tensors
        B, Hy, K, _ = kps.shape
        S, rect, flags = ctx.cfg
        gk = torch.empty_like(kps)
        call('xas_patch_to_world_bwd', ptr(kps), ptr(gw.contiguous()), *[ptr(c) for c in cams], B, Hy, K, S, rect,
             flags, ptr(gk))
        return (gk,) + (None,) * 8


def patch_to_world(kps, trans_image, k_mat, pelvis, rot_world, trans_world, image_size=256, rect_width=2000.0,
                   is_norm=True, mono=False, patch=True):
    """kps [B,K,3] or [B,Hy,K,3] -> world coordinates of the same shape (modules/util.py:128-152)."""
    squeeze = kps.dim() == 3
    if squeeze:
        kps = kps.unsqueeze(1)
    flags = (GEO_NORM if is_norm else 0) | (GEO_MONO if mono else 0) | (GEO_PATCH if patch else 0)
    out = _PatchToWorld.apply(kps, trans_image, k_mat, pelvis, rot_world, trans_world, image_size, rect_width, flags)
    return out.squeeze(1) if squeeze else out


class _WorldToPatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, pre_rot, ti, km, pv, rw, tw, pre_scale, pelvis_origin, image_size, rect_width, flags):
        pts = pts.contiguous()
        B, Hy, K, _ = pts.shape
        rot = pre_rot.contiguous() if pre_rot is not None else None
        cams = [t.contiguous().float() for t in (ti, km, pv, rw, tw)]
        out = torch.empty_like(pts)
        call('xas_world_to_patch_fwd', ptr(pts), ptr(rot), float(pre_scale), int(pelvis_origin), *[ptr(c) for c in cams],
             B, Hy, K, float(image_size), float(rect_width), flags, ptr(out))
        ctx.save_for_backward(pts, *cams, *(() if rot is None else (rot,)))
        ctx.cfg = (float(pre_scale), int(pelvis_origin), float(image_size), float(rect_width), flags)
        return out

    @staticmethod
    def backward(ctx, go):
        pts, ti, km, pv, rw, tw, *rot = ctx.saved_tensors
        rot = rot[0] if rot else None
        B, Hy, K, _ = pts.shape
        scale, origin, S, rect, flags = ctx.cfg
        gp = torch.empty_like(pts)
        grot = torch.empty_like(rot) if rot is not None else None
        call('xas_world_to_patch_bwd', ptr(pts), ptr(go.contiguous()), ptr(rot), scale, origin, ptr(ti), ptr(km), ptr(pv),
             ptr(rw), ptr(tw), B, Hy, K, S, rect, flags, ptr(gp), ptr(grot))
        return (gp, grot) + (None,) * 10


def world_to_patch(points, params, mode, is_norm=True, RECT_WIDTH=2000, pre_rot=None, pre_scale=1.0, pelvis_origin=False,
                   stop_at_image=False, stop_at_world=False):
    """World mm -> patch coordinates of camera `mode` of the batch dict (modules/util.py:155-168), points [B,K,3] or
    [B,Hy,K,3].  With `pre_rot` [B,3,3] the points are first turned and scaled, (p . pre_rot) * pre_scale, and with
    `pelvis_origin` moved to the pelvis in world coordinates (the front of project_smpl_to_patch_kps, util.py:376-380) - all
    in the one launch.  `stop_at_image`: (u px, v px, depth mm) of util.py:116-125; `stop_at_world`: the world points
    themselves.  Differentiable in `points` and `pre_rot`; the camera arrays are constants."""
    squeeze = points.dim() == 3
    if squeeze:
        points = points.unsqueeze(1)
    if points.dim() != 4 or points.shape[-1] != 3:
        raise RuntimeError('world_to_patch: points must be [B,K,3] or [B,Hy,K,3]')
    if pre_rot is not None and tuple(pre_rot.shape) != (points.shape[0], 3, 3):
        raise RuntimeError('world_to_patch: pre_rot must be [B,3,3]')
    flags = (GEO_NORM if is_norm else 0) | (GEO_IMAGE if stop_at_image else 0) | (GEO_WORLD if stop_at_world else 0)
    key = lambda name: params['{}_{}'.format(mode, name)]
    out = _WorldToPatch.apply(points.float(), None if pre_rot is None else pre_rot.float(), key('trans_image'), key('k_mat'),
                              key('pelvis'), key('rot_world'), key('trans_world'), pre_scale, bool(pelvis_origin),
                              key('img').shape[-1], RECT_WIDTH, flags)
    return out.squeeze(1) if squeeze else out


_link_cache = {}


def _links(parents, children, device):
    key = (tuple(parents), tuple(children), str(device))
    if key not in _link_cache:
        _link_cache[key] = (torch.tensor(list(parents), dtype=torch.int32, device=device),
                            torch.tensor(list(children), dtype=torch.int32, device=device))
    return _link_cache[key]


class _DrawLinesMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kps2d, S, parents, children, body_width):
        kps2d = kps2d.contiguous()
        B, K, _ = kps2d.shape
        L = len(parents)
        par, chi = _links(parents, children, kps2d.device)
        fine = 0
        if L >= 21:                       # modules/util.py:50-53
            for l in (11, 12, 14, 15):
                fine |= 1 << l
        mask = torch.empty(B, 1, S, S, device=kps2d.device, dtype=torch.float32)
        call('xas_draw_lines_max_fwd', ptr(kps2d), K * 2, 2, B, K, ptr(par), ptr(chi), L, fine, float(body_width), S,
             ptr(mask))
        ctx.save_for_backward(kps2d, par, chi)
        ctx.cfg = (S, L, fine, float(body_width))
        return mask

    @staticmethod
    def backward(ctx, gmask):
        kps2d, par, chi = ctx.saved_tensors
        S, L, fine, width = ctx.cfg
        B, K, _ = kps2d.shape
        nblk = query('xas_lines_nblk', S)
        partial = torch.empty(B * nblk * K * 2, device=kps2d.device, dtype=torch.float32)
        g = torch.empty_like(kps2d)
        call('xas_draw_lines_max_bwd', ptr(kps2d), K * 2, 2, B, K, ptr(par), ptr(chi), L, fine, width, S,
             ptr(gmask.contiguous()), ptr(partial), ptr(g))
        return g, None, None, None, None


def draw_lines_max(kps2d, image_size, parents, children, body_width):
    """[B,K,2] -> max over line heat-maps [B,1,S,S]  (modules/util.py:21-59 + modules/model.py:94)."""
    return _DrawLinesMax.apply(kps2d, int(image_size), parents, children, body_width)
