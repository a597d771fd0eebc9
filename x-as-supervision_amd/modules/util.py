"""Geometry helpers of the training path on the MI355X kernels (reference: modules/util.py).

Built here: `draw_lines` (+ the fused `draw_lines_max` the model actually consumes),
`convert_patch_to_world` (all hypotheses in one launch, closed-form 2x2 / 3x3 inverses),
`make_coordinate_grid`, `smpl_to_h36m`, and for the evaluation path `convert_patch_to_image`,
`triangulation` / `batch_triangulate` (device DLT, no batched SVD), `resolve_views` (left/right exchange and depth hypothesis by
the cameras' agreement, no reference counterpart), `spread_weight` (heat-map spread -> per-view weight) with `triangulation_weighted` / `resolve_views_weighted` (opt-in, no
reference counterpart), and the SMPL side of the geometry:
`project_smpl_to_patch_kps`, `convert_pelvis_to_world` (one world->patch launch, ops_head.world_to_patch) and `flip_3D`.
`convert_world_to_patch` / `convert_world_to_image` / `convert_image_to_patch` stay the reference's (the device version is
ops_head.world_to_patch).  The reference's dead code (rule_transformation, my_truncated_normal) is not rebuilt
(SURVEY 2, row 6).
"""
import torch

from xas_amd import ops_eval, ops_head


def make_coordinate_grid(spatial_size, type):
    """[-1,1] x [-1,1] mesh, grid[i, j] = (2j/(w-1)-1, 2i/(h-1)-1)   (util.py:3-19)."""
    h, w = spatial_size
    xs = 2 * (torch.arange(w).type(type) / (w - 1)) - 1
    ys = 2 * (torch.arange(h).type(type) / (h - 1)) - 1
    return torch.stack([xs.view(1, w).expand(h, w), ys.view(h, 1).expand(h, w)], dim=2)


def draw_lines_max(keypoints, image_size, parent_ids, child_ids, body_width):
    """max over the line heat-maps of `draw_lines`, [B,1,S,S]: the only way the model uses them
    (model.py:91-96).  One fused kernel; nothing but the mask is written."""
    return ops_head.draw_lines_max(keypoints, image_size, parent_ids, child_ids, body_width)


def draw_lines(keypoints, image_size, parent_ids, child_ids, body_width):
    """Per-line heat-maps [B, L, S, S] (util.py:21-59).  The training step never materialises them
    (see draw_lines_max); this entry renders one line per launch for callers that want the stack."""
    maps = []
    fine = (11, 12, 14, 15) if len(parent_ids) >= 21 else ()
    for l, (p, c) in enumerate(zip(parent_ids, child_ids)):
        width = body_width / 2.0 if l in fine else body_width      # exponent x2 == width / 2
        maps.append(ops_head.draw_lines_max(keypoints, image_size, [p], [c], width))
    return torch.cat(maps, dim=1)


def convert_patch_to_world(keypoints, params, mode, is_norm=True, RECT_WIDTH=2000, mono=False, patch=True):
    """Patch coordinates -> world mm for camera `mode` of the batch dict (util.py:128-152).
    keypoints: [B,K,3] or, for all hypotheses at once, [B,Hy,K,3]."""
    size = params['{}_img'.format(mode)].shape[-1]
    return ops_head.patch_to_world(
        keypoints, params['{}_trans_image'.format(mode)], params['{}_k_mat'.format(mode)],
        params['{}_pelvis'.format(mode)], params['{}_rot_world'.format(mode)], params['{}_trans_world'.format(mode)],
        image_size=size, rect_width=RECT_WIDTH, is_norm=is_norm, mono=mono, patch=patch)


def convert_patch_to_image(kps, trans, image_depth, image_height, image_width, depth_scale, pelvis, is_norm=True):
    """Patch -> image (u px, v px, depth mm), util.py:61-83.  The kernel takes the square patch size and the
    metric box width; `depth_scale` is RECT_WIDTH / image size at every call site (util.py:180-182)."""
    if not (image_depth == image_height == image_width):
        raise RuntimeError('convert_patch_to_image: the patch must be a cube (D == H == W)')
    return ops_eval.patch_to_image(kps, trans, pelvis, image_size=image_width, rect_width=depth_scale * image_width,
                                   is_norm=is_norm)


def batch_triangulate(keypoints_, Pall, robust_px=None):
    """keypoints_ [B,V,K,3] = (u, v, weight), Pall [B,V,3,4] -> [B,K,4] (util.py:198-230).  With `robust_px` (pixels) the
    DLT runs over the largest set of views that agree within that threshold (ops_eval.triangulate_robust)."""
    if robust_px is None:
        return ops_eval.triangulate_dlt(keypoints_, Pall)
    return ops_eval.triangulate_robust(keypoints_, Pall, threshold_px=robust_px, want=())['xyzw']


def spread_weight(spread, trans_image, cell_px=4.0):
    """Heat-map spread [B,K,5] (ops_head.heatmap_spread) of one camera -> triangulation weight [B,K] = 1 / sigma in pixels of
    the full image, the unit of the DLT's residuals:
        w = 1 / sqrt((Var_w + Var_h + 2/12) * (cell_px * s)^2),   s = 1 / sqrt(|det trans_image[:, :2, :2]|)
    `s` is the image pixels per patch pixel of the sample's crop and `cell_px` the patch pixels per heat-map cell.  The 2/12 is
    the variance of a uniform distribution over one cell on each axis - the quantisation floor of a heat-map - and keeps a
    one-hot map finite.  No reference counterpart."""
    a = trans_image[:, :2, :2].to(spread.dtype)
    det = (a[:, 0, 0] * a[:, 1, 1] - a[:, 0, 1] * a[:, 1, 0]).abs()
    var_px = (spread[..., 2] + spread[..., 3] + 2.0 / 12.0) * (cell_px * cell_px / det).unsqueeze(-1)
    return var_px.rsqrt()


def _stack_points(pts, weights, modes):
    """(u, v, depth) of every camera stacked [B,V,K,3]; with `weights` ({cam_key: [B,K]}) those replace the third column."""
    pts = torch.stack(pts, dim=1)
    if weights is not None:
        pts = torch.cat([pts[..., :2], torch.stack([weights[m] for m in modes], dim=1).to(pts.dtype).unsqueeze(-1)], dim=-1)
    return pts


def triangulation(keypoints, params, cam_id_list, is_norm=True, RECT_WIDTH=2000, robust_px=None, return_inliers=False):
    """{cam_key: [B,K,3]} patch predictions of all cameras -> world joints [B,K,3] (util.py:171-196).  `robust_px`: as in
    batch_triangulate; with `return_inliers` also the [B,K] uint8 masks of the views used (bit i = cam_id_list[i];
    None without robust_px).  Every view weighs by the joint's depth in mm, as in the reference."""
    return triangulation_weighted(keypoints, params, cam_id_list, None, is_norm, RECT_WIDTH, robust_px, return_inliers)


def triangulation_weighted(keypoints, params, cam_id_list, weights, is_norm=True, RECT_WIDTH=2000, robust_px=None,
                           return_inliers=False, *, inputs=None):
    """triangulation with `weights`, {cam_key: [B,K]}: the weight of every view and joint (spread_weight) in place of the
    reference's, which is the joint's depth in mm.  A weight that is not finite or not positive marks the view invalid for that
    joint, by the kernels' rule for the third column.  None: the reference's weights, bit for bit.  `inputs`: the
    (points, projection matrices) of triangulation_inputs where the caller has them already.  No reference counterpart."""
    pts, pm = inputs or _triangulation_inputs(keypoints, params, cam_id_list, weights, is_norm, RECT_WIDTH)
    init, used = _triangulation_start(pts, pm, robust_px)
    return (init[..., :3], used) if return_inliers else init[..., :3]


def _triangulation_start(pts, pm, robust_px):
    """Where triangulation_weighted ends and the refinements begin: the DLT over all views, or with `robust_px` over the largest
    set of views that agree within it.  -> (init [B,K,4], used: the [B,K] uint8 masks of those views, None without robust_px)."""
    if robust_px is None:
        return batch_triangulate(pts, pm), None
    r = ops_eval.triangulate_robust(pts, pm, threshold_px=robust_px, want=('inliers',))
    return r['xyzw'], r['inliers']


def _triangulation_inputs(keypoints, params, cam_id_list, weights, is_norm, RECT_WIDTH):
    """What every triangulation starts from: points [B,V,K,3] = (u px, v px, weight) and projection matrices [B,V,3,4]."""
    pts, pm = [], []
    for cam_id in cam_id_list:
        mode = 'cam_{}'.format(cam_id)
        size = params['{}_img'.format(mode)].shape[-1]
        pts.append(ops_eval.patch_to_image(keypoints[mode], params['{}_trans_image'.format(mode)],
                                           params['{}_pelvis'.format(mode)], image_size=size, rect_width=RECT_WIDTH,
                                           is_norm=is_norm))
        pm.append(ops_eval.projection_matrix(params['{}_k_mat'.format(mode)], params['{}_rot_world'.format(mode)],
                                             params['{}_trans_world'.format(mode)]))
    return _stack_points(pts, weights, ['cam_{}'.format(c) for c in cam_id_list]), torch.stack(pm, dim=1)


def correction_matrix(delta):
    """delta [...,6] = (omega rad, tau mm) -> T [...,4,4] float64 = [exp([omega]x), tau; 0 1], the rigid motion of the world in
    front of a camera that xas_calibrate_bundle estimates (P T is the corrected matrix).  The exponential map as in
    include/xas_hip.h: its series I + K + K^2 / 2 for |omega|^2 < 1e-16."""
    delta = delta.double()
    w = delta[..., :3]
    th2 = (w * w).sum(-1)
    small = th2 < 1e-16
    t2 = torch.where(small, torch.ones_like(th2), th2)
    th = t2.sqrt()
    a = torch.where(small, torch.ones_like(th), torch.sin(th) / th)[..., None, None]
    b = torch.where(small, torch.full_like(th, 0.5), (1.0 - torch.cos(th)) / t2)[..., None, None]
    z = torch.zeros_like(th2)
    K = torch.stack([z, -w[..., 2], w[..., 1], w[..., 2], z, -w[..., 0], -w[..., 1], w[..., 0], z], -1).reshape(w.shape[:-1] + (3, 3))
    T = torch.zeros(w.shape[:-1] + (4, 4), dtype=torch.float64, device=delta.device)
    T[..., :3, :3] = torch.eye(3, dtype=torch.float64, device=delta.device) + a * K + b * (K @ K)
    T[..., :3, 3] = delta[..., 3:]
    T[..., 3, 3] = 1.0
    return T


def apply_calibration(params, cam_id_list, keys, delta):
    """A shallow copy of the batch dict with the corrections of xas_amd.ops_calib.calibrate_bundle applied: keys [R,V,3,4] are
    the rigs' projection matrices (ops_calib.rigs_of) and delta [R,V,6] their corrections.  A sample belongs to the rig whose
    matrices its own equal bit for bit; one that matches no rig raises.  With P = K [R | t] (projection_kernel) and T(delta) =
    [E, tau; 0 1], P T = K [R E | R tau + t]: cam_*_rot_world becomes R E and cam_*_trans_world R tau + t, formed in double and
    rounded once, so that ops_eval.projection_matrix of the copy is P T to fp32 rounding.  The original dict is untouched: the
    ground truth keeps reading it."""
    modes = ['cam_{}'.format(c) for c in cam_id_list]
    pm = torch.stack([ops_eval.projection_matrix(params[m + '_k_mat'], params[m + '_rot_world'], params[m + '_trans_world'])
                      for m in modes], dim=1)
    B, R = pm.shape[0], keys.shape[0]
    keys = keys.to(device=pm.device, dtype=torch.float32).contiguous()
    match = (pm.contiguous().view(torch.int32).reshape(B, 1, -1) == keys.view(torch.int32).reshape(1, R, -1)).all(dim=-1)
    if not bool(match.any(dim=1).all()):
        raise RuntimeError('apply_calibration: a sample whose cameras match none of the %d calibrated rigs bit for bit' % R)
    T = correction_matrix(delta.to(pm.device))[match.float().argmax(dim=1)]              # [B,V,4,4]
    out = dict(params)
    for i, m in enumerate(modes):
        rot, t = params[m + '_rot_world'].double().reshape(B, 3, 3), params[m + '_trans_world'].double().reshape(B, 3)
        out[m + '_rot_world'] = (rot @ T[:, i, :3, :3]).float().reshape(params[m + '_rot_world'].shape)
        out[m + '_trans_world'] = (torch.einsum('bij,bj->bi', rot, T[:, i, :3, 3]) + t).float().reshape(params[m + '_trans_world'].shape)
    return out


def triangulation_inputs(keypoints, params, cam_id_list, weights=None, is_norm=True, RECT_WIDTH=2000):
    """points [B,V,K,3] and projection matrices [B,V,3,4] as every triangulation above forms them: eval.py forms them once per
    batch, hands them to the solver that runs as its `inputs` and keeps them for --calibrate and --smooth."""
    return _triangulation_inputs(keypoints, params, cam_id_list, weights, is_norm, RECT_WIDTH)


def triangulation_refined(keypoints, params, cam_id_list, weights=None, is_norm=True, RECT_WIDTH=2000, robust_px=None,
                          huber_px=0.0, want=(), *, inputs=None):
    """triangulation_weighted, then Levenberg-Marquardt on the reprojection error in pixels from its point, over the views it
    used (ops_eval.triangulate_refine).  With `weights` every view's residual is scaled by its weight, so with spread_weight
    (1 / sigma in pixels) the cost is the detections' negative log-likelihood and `cov` the joint's covariance in mm^2; without,
    the residuals count in plain pixels (the depth in mm is no scale of a pixel error).  `huber_px` > 0: Huber's loss.
    `inputs`: as in triangulation_weighted.
    -> (world joints [B,K,3], dict of ops_eval.triangulate_refine: xyzw and the outputs in `want`, + `inliers` with
    robust_px).  No reference counterpart."""
    pts, pm = inputs or _triangulation_inputs(keypoints, params, cam_id_list, weights, is_norm, RECT_WIDTH)
    init, used = _triangulation_start(pts, pm, robust_px)
    out = ops_eval.triangulate_refine(pts, pm, init, views=used, weighted=weights is not None, huber_px=huber_px, want=want)
    if used is not None:
        out['inliers'] = used
    return out['xyzw'][..., :3], out


def triangulation_skeleton(keypoints, params, cam_id_list, weights=None, is_norm=True, RECT_WIDTH=2000, robust_px=None,
                           huber_px=0.0, sym_w=ops_eval.TRI_SYM_W, limbs=ops_eval.SYM_LIMBS, want=(), *,
                           inputs=None):
    """triangulation_refined with the joints of every sample refined together under left/right limb symmetry
    (ops_eval.triangulate_skeleton): the same inputs, the same start (the DLT, or the robust point and its inlier masks with
    robust_px), the same weights; `sym_w` px^2 per mm^2 on the squared difference of each limb pair's lengths.
    `inputs`: as in triangulation_weighted.
    -> (world joints [B,K,3], dict of ops_eval.triangulate_skeleton: xyzw and the outputs in `want`, + `inliers` with
    robust_px).  No reference counterpart."""
    pts, pm = inputs or _triangulation_inputs(keypoints, params, cam_id_list, weights, is_norm, RECT_WIDTH)
    init, used = _triangulation_start(pts, pm, robust_px)
    out = ops_eval.triangulate_skeleton(pts, pm, init, views=used, limbs=limbs, weighted=weights is not None, huber_px=huber_px,
                                        sym_w=sym_w, want=want)
    if used is not None:
        out['inliers'] = used
    return out['xyzw'][..., :3], out


def triangulation_volume(sel_or_init, logits, params, cam_id_list, chan=None, views=None, RECT_WIDTH=2000,
                         G=ops_eval.TRI_VOL_G, levels=ops_eval.TRI_VOL_LEVELS, side_mm=ops_eval.TRI_VOL_SIDE_MM, beta=1.0,
                         out_penalty=1.0, want=()):
    """Volumetric fusion of the cameras' heat-map cubes round a triangulated point (ops_eval.triangulate_volume).
    `sel_or_init`: the start, world joints [B,K,3] (or [B,K,4]) from any triangulation or refinement, or {cam_key: [B,K,3]}
    patch predictions, which are triangulated by the DLT first.  `logits`: {cam_key: [B,K*D,D,D]} of the detector's
    forward_logits; `chan` [V,B,K] int32 (V in cam_id_list's order) the heat-map channel every camera reads for every joint,
    None = the joint's own; `views` [B,K] uint8 (bit i = cam_id_list[i]) the cameras that take part, None = all.
    -> (world joints [B,K,3], dict of ops_eval.triangulate_volume: xyz and the outputs in `want`, + `init`).  No reference
    counterpart."""
    modes = ['cam_{}'.format(c) for c in cam_id_list]
    init = triangulation(sel_or_init, params, cam_id_list, RECT_WIDTH=RECT_WIDTH) if isinstance(sel_or_init, dict) else sel_or_init
    init = init[..., :3].contiguous()
    stack = lambda name: torch.stack([params['{}_{}'.format(m, name)].float() for m in modes], dim=0)
    out = ops_eval.triangulate_volume([logits[m] for m in modes], chan, stack('trans_image'), stack('k_mat'), stack('pelvis'),
                                      stack('rot_world'), stack('trans_world'), init, views=views, G=G, levels=levels,
                                      side_mm=side_mm, beta=beta, out_penalty=out_penalty,
                                      image_size=params['{}_img'.format(modes[0])].shape[-1], rect_width=RECT_WIDTH, want=want)
    out['init'] = init
    return out['xyz'], out


def resolve_views(kps_by_cam, params, cam_id_list, pairs, gt=True, RECT_WIDTH=2000):
    """{cam_key: [B,Hy,K,3]} raw detections of all cameras -> ({cam_key: [B,K,3]} resolved joints, the other outputs of
    ops_eval.multiview_resolve).  The left/right exchange of every view and the depth hypothesis of every view and joint are
    decided by the agreement of the cameras; with `gt` the labels (`<cam>_joints`) name each pair once for all views, and
    nothing else is read from them.  Bit i of `swap` is cam_id_list[i].  No reference counterpart."""
    return resolve_views_weighted(kps_by_cam, params, cam_id_list, pairs, None, gt, RECT_WIDTH)


def resolve_views_weighted(kps_by_cam, params, cam_id_list, pairs, weights, gt=True, RECT_WIDTH=2000):
    """resolve_views with `weights`, {cam_key: [B,K]}, in place of the depth in mm as every view's weight, as in
    triangulation_weighted (not finite or not positive: the view is invalid for that joint).  None: the depth, bit for bit."""
    modes = ['cam_{}'.format(c) for c in cam_id_list]
    pts, pm, world, kps = [], [], [], []
    for mode in modes:
        k = kps_by_cam[mode]
        size = params['{}_img'.format(mode)].shape[-1]
        pts.append(ops_eval.patch_to_image(k[:, 0], params['{}_trans_image'.format(mode)], params['{}_pelvis'.format(mode)],
                                           image_size=size, rect_width=RECT_WIDTH))
        pm.append(ops_eval.projection_matrix(params['{}_k_mat'.format(mode)], params['{}_rot_world'.format(mode)],
                                             params['{}_trans_world'.format(mode)]))
        world.append(convert_patch_to_world(k, params, mode, is_norm=True, RECT_WIDTH=RECT_WIDTH))
        kps.append(k)
    labels = torch.stack([params[mode + '_joints'] for mode in modes], dim=1) if gt else None
    pts = _stack_points(pts, weights, modes)
    r = ops_eval.multiview_resolve(pts, torch.stack(pm, dim=1), torch.stack(kps, dim=1),
                                   torch.stack(world, dim=1), pairs=pairs, gt=labels, image_size=size)
    sel = r.pop('sel')
    # the views that took part, [B,K] bit masks like `swap` (derived here, the kernel keeps it to itself): finite weight > 0
    # for the joint and for its partner
    w = pts[..., 2]
    ok = torch.isfinite(w) & (w > 0)
    ok = ok & ok[..., ops_eval.switch_perm(w.shape[-1], pairs, w.device).long()]
    bit = (1 << torch.arange(len(modes), device=w.device, dtype=torch.int32)).view(1, -1, 1)
    r['valid'] = (ok.int() * bit).sum(dim=1).to(torch.uint8)
    return {mode: sel[:, i] for i, mode in enumerate(modes)}, r


def multiview_consistency_loss(kps_by_cam, world_by_cam, params, cam_id_list, weight_2d, weight_3d, huber_px=0.0,
                               detach_target=False, weights=None):
    """Multi-view consistency term of the training step (ops_eval.multiview_consistency, called once).  {cam_key: [B,Hy,K,3]}
    raw detections of all cameras and their single-view world points (convert_patch_to_world, with its graph); `weights`
    {cam_key: [B,K]} as in triangulation_weighted, None: every view counts 1.
    -> ((weight_2d * sum of the reprojection terms in px^2 + weight_3d * sum of the depth terms in mm^2) / max(joints that were
    solved, 1) as a device scalar, the triangulated joints [B,K,3] without a graph (NaN where a joint was passed through)).
    Nothing here synchronises with the host.  No reference counterpart."""
    modes = ['cam_{}'.format(c) for c in cam_id_list]
    size = params['{}_img'.format(modes[0])].shape[-1]
    stack = lambda fmt: torch.stack([params[fmt.format(mode)] for mode in modes], dim=1)
    B, V = params['{}_k_mat'.format(modes[0])].shape[0], len(modes)
    pm = ops_eval.projection_matrix(stack('{}_k_mat').flatten(0, 1), stack('{}_rot_world').flatten(0, 1),
                                    stack('{}_trans_world').flatten(0, 1)).view(B, V, 3, 4)
    reproj, depth, xyz, status = ops_eval.multiview_consistency(
        torch.stack([kps_by_cam[mode][:, 0, :, :2] for mode in modes], dim=1), stack('{}_trans_image'),
        torch.stack([world_by_cam[mode] for mode in modes], dim=1), pm,
        weight=None if weights is None else torch.stack([weights[mode] for mode in modes], dim=1), image_size=size,
        huber_px=huber_px, detach_target=detach_target)
    solved = (status == 0).sum().clamp(min=1)
    return (weight_2d * reproj.sum() + weight_3d * depth.sum()) / solved, xyz.detach()


def smpl_to_h36m(verts, h36m_regressor):
    """17 regressed joints, L/R arms swapped, thorax appended, root centred (util.py:331-341)."""
    j = torch.einsum('bki,lk->bli', verts, h36m_regressor)
    j = j[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13]]
    j = torch.cat([j, j[:, [11, 14]].mean(dim=1, keepdim=True)], dim=1)
    return j - j[:, 0:1]


def convert_pelvis_to_world(x, mode):
    """Pelvis of camera `mode` in world coordinates, inv(rot_world) (pelvis - trans_world), [B,1,3] (util.py:343-352)."""
    pelvis = x['{}_pelvis'.format(mode)]
    zero = torch.zeros(pelvis.shape[0], 1, 3, device=pelvis.device, dtype=torch.float32)
    return ops_head.world_to_patch(zero, x, mode, pelvis_origin=True, stop_at_world=True)


def project_smpl_to_patch_kps(global_rot_params, pose_params, shape_params,
                              smpl_layer, h36m_regressor, x, mode, convert_verts=False):
    """SMPL parameters -> the 18 H36M joints in the patch of camera `mode`, pixels [B,18,3] (util.py:356-383); with
    `convert_verts` the vertices in world mm instead.  The global rotation is applied after the layer (row vector times
    `global_rot_params` [B,3,3]), so the layer runs with a zero root rotation.  SMPL skinning, the joint regression and
    one world->patch launch (rotation, m -> mm, pelvis shift, projection); differentiable in the three parameter sets."""
    full_pose = torch.cat([pose_params.new_zeros(pose_params.shape[0], 3), pose_params], dim=1)
    verts, _ = smpl_layer(full_pose, shape_params)
    if convert_verts:
        return ops_head.world_to_patch(verts, x, mode, pre_rot=global_rot_params, pre_scale=1000.0, pelvis_origin=True,
                                       stop_at_world=True)
    joints = smpl_to_h36m(verts, h36m_regressor)
    return ops_head.world_to_patch(joints, x, mode, is_norm=False, pre_rot=global_rot_params, pre_scale=1000.0,
                                   pelvis_origin=True)


def normalise_patch_joints(kps, size, RECT_WIDTH=2000):
    """Patch pixels [B,K,3] (project_smpl_to_patch_kps) -> the form the step expects of `<cam>_pseudo_joints`: x, y in [-1, 1]
    over the pixel centres 0 .. size - 1, z in units of RECT_WIDTH (depth px * (RECT_WIDTH / size) mm / RECT_WIDTH = px / size:
    what the reference's loader makes of a depth in metres, dataloader.py:227)."""
    xy = kps[..., :2] / (size - 1.0) * 2.0 - 1.0
    return torch.cat([xy, kps[..., 2:3] / float(size)], dim=-1)


RENDER_LOOKS = ('shade', 'parts')     # untextured shaded body (smpl_pseudo_img) / pure body-part colours (smpl_part_seg_img)
RENDER_AMBIENT = 0.35                 # untuned: no rendering of the authors' to match


def render_smpl_to_patch(global_rot_params, pose_params, shape_params, smpl_layer, h36m_regressor, x, mode, look='shade',
                         size=256):
    """SMPL parameters -> a rendering of the body in the patch of camera `mode` and its joints:
    (img [B,3,S,S] in [0,1], mask [B,1,S,S], joints [B,18,3] normalised by normalise_patch_joints).  No reference counterpart
    (its pseudo-images are read from disk); no graph is kept.
    The SMPL layer runs once.  The joints are project_smpl_to_patch_kps's, launch for launch; the vertices take its
    convert_verts path to world mm and one more world->patch launch to patch pixels (x, y) and depth relative to the pelvis in
    the patch's depth unit (RECT_WIDTH / size mm, about what a pixel spans at the pelvis), so depth_scale = 1 makes the three
    axes of the shading normal commensurate.  Vertices at or behind the camera plane become NaN: the renderer drops their faces.
    `look`: 'shade' = white faces, ambient RENDER_AMBIENT, lit from the viewer; 'parts' = ops_render.part_colours, ambient 1."""
    from xas_amd import ops_render
    if look not in RENDER_LOOKS:
        raise ValueError('render_smpl_to_patch: look=%r (known: %s)' % (look, ', '.join(RENDER_LOOKS)))
    faces = smpl_layer.th_faces
    if faces.numel() == 0:
        raise RuntimeError('render_smpl_to_patch: the SMPL layer has no faces (th_faces is empty)')
    S_img = x['{}_img'.format(mode)].shape[-1]
    with torch.no_grad():
        full_pose = torch.cat([pose_params.new_zeros(pose_params.shape[0], 3), pose_params], dim=1)
        verts, _ = smpl_layer(full_pose, shape_params)
        if verts.shape[0] * verts.shape[1] > 0x7fffffff // 3:            # xas_world_to_patch_fwd: one thread per point, any K
            raise RuntimeError('render_smpl_to_patch: %d x %d vertices exceed one world->patch launch' % tuple(verts.shape[:2]))
        joints = ops_head.world_to_patch(smpl_to_h36m(verts, h36m_regressor), x, mode, is_norm=False,
                                         pre_rot=global_rot_params, pre_scale=1000.0, pelvis_origin=True)
        world = ops_head.world_to_patch(verts, x, mode, pre_rot=global_rot_params, pre_scale=1000.0, pelvis_origin=True,
                                        stop_at_world=True)
        pix = ops_head.world_to_patch(world, x, mode, is_norm=False)
        unit = 2000.0 / S_img                                            # mm per depth unit (world_to_patch's RECT_WIDTH)
        cam_z = pix[..., 2] * unit + x['{}_pelvis'.format(mode)][:, 2:3].float()
        pix = torch.where((cam_z > 0).unsqueeze(-1), pix, pix.new_full((), float('nan')))
        if size != S_img:                                                # pixel centres 0 .. S_img - 1 onto 0 .. size - 1
            pix = pix * pix.new_tensor([(size - 1.0) / (S_img - 1.0), (size - 1.0) / (S_img - 1.0), float(size) / S_img])
        if look == 'parts':
            rgb, ambient = ops_render.part_colours(smpl_layer.th_weights, faces), 1.0
        else:
            rgb, ambient = None, RENDER_AMBIENT
        r = ops_render.render_mesh(pix, faces, face_rgb=rgb, ambient=ambient, depth_scale=1.0, size=size)
    return r['img'], r['mask'], normalise_patch_joints(joints, S_img)


def random_rotation_3D(keypoints):
    """Random rotation about z in [-pi/4, pi/4] per sample (util.py:389-407; only with use_aug).  The angles are drawn
    from the CPU generator exactly as the reference does (torch.rand(B, 1)): same seed, same augmentation."""
    B = keypoints.shape[0]
    ang = ((torch.rand(B, 1) - 0.5) * 0.5 * torch.pi).squeeze(1).to(keypoints.device)
    c, s, z, o = torch.cos(ang), torch.sin(ang), torch.zeros_like(ang), torch.ones_like(ang)
    rot = torch.stack([c, -s, z, s, c, z, z, z, o], dim=1).view(B, 3, 3)
    return torch.bmm(keypoints, rot.to(keypoints.dtype))


def flip_3D(keypoints):
    """Swap left and right of the legs (joints 1-3 / 4-6) or of the arms (11-13 / 14-16), chosen by one torch.rand(1) of the
    CPU generator as the reference does (util.py:409-416)."""
    order = list(range(keypoints.shape[1]))
    if torch.rand(1) < 0.5:
        order[1:7] = [4, 5, 6, 1, 2, 3]
    else:
        order[11:17] = [14, 15, 16, 11, 12, 13]
    return keypoints[:, order]


# names this mirror does not replace resolve, lazily, to the reference module behind it on sys.path
from xas_amd._next import fallthrough as _fallthrough  # noqa: E402

__getattr__ = _fallthrough(__name__, __file__)
