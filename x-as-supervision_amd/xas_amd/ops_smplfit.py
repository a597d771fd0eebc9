"""SMPL parameters from 18 world joints on the device (csrc/smplfit.hip, xas_smpl_fit): the inverse of
modules.util.project_smpl_to_patch_kps' model, Y = R(omega) (1000 smpl_to_h36m(layer((0, theta), beta))) + t, solved by a
double-precision Levenberg-Marquardt, one workgroup per sample.  include/xas_hip.h states the residual order and the schedule.
Nothing here keeps state between calls or synchronises with the host.  No reference counterpart."""
import torch

from xas_amd._lib import call, ptr, query

# Weights of the priors sqrt(w) theta_i (per radian^2, against mm^2 of the joint rows) and sqrt(w) beta_i.  UNTUNED GUESSES:
# there is neither a dataset nor a checkpoint here to tune them on.  They keep the 85 unknowns determined by 54 joint rows.
POSE_PRIOR = 100.0
SHAPE_PRIOR = 25.0

STATUS_CONVERGED, STATUS_LIMIT, STATUS_PASSED = 0, 1, 2
STATUS_NAMES = ('converged', 'iteration limit', 'passed through')


def _layer_arrays(smpl_layer, dev):
    bufs = tuple(t.to(device=dev, dtype=torch.float32).contiguous() for t in (
        smpl_layer.th_v_template.reshape(-1, 3), smpl_layer.th_shapedirs, smpl_layer.th_posedirs, smpl_layer.th_J_regressor,
        smpl_layer.th_weights))
    parents = smpl_layer._parents.to(device=dev, dtype=torch.int32).contiguous()
    center = -1 if smpl_layer.center_idx is None else int(smpl_layer.center_idx)
    return bufs, parents, center


def compact_regressor(h36m_regressor):
    """[17,V] -> (reg_verts [V] int32: the vertices with a non-zero column first, ascending; reg_count [1] int32), on the
    regressor's device and without a host synchronisation (no nonzero())."""
    used = (h36m_regressor != 0).any(dim=0)
    order = torch.argsort((~used).to(torch.int32), stable=True).to(torch.int32).contiguous()
    return order, used.sum().to(torch.int32).reshape(1)


def _expmap_log(R):
    """Rotation matrices [B,3,3] -> axis-angle [B,3] (angle in [0, pi); ill-conditioned towards pi, good enough for a start)."""
    cos = ((R.diagonal(dim1=1, dim2=2).sum(1) - 1.0) * 0.5).clamp(-1.0, 1.0)
    th = torch.acos(cos)
    v = torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], dim=1)
    s = v.norm(dim=1)
    return v * (th / s.clamp(min=1e-12)).unsqueeze(1)


def default_init(targets, weights, smpl_layer, h36m_regressor):
    """Zero body pose and betas, t = the target pelvis (where it is not usable: what the rigid alignment gives), omega from the
    weighted rigid (Kabsch) alignment of the zero-pose joints to the targets.  torch on the device, float64; not a hot path.
    -> dict(pose [B,72], betas [B,10], trans [B,3]) float32."""
    from modules.util import smpl_to_h36m
    dev, B = targets.device, targets.shape[0]
    with torch.no_grad():
        verts, _ = smpl_layer.to(dev)(torch.zeros(1, 72, device=dev), torch.zeros(1, 10, device=dev))
        src = smpl_to_h36m(verts, h36m_regressor.to(dev)).double() * 1000.0              # [1,18,3], root centred
        w = torch.where(weights > 0, weights, torch.zeros_like(weights)).double()       # NaN and negative weights: 0
        tgt = torch.where((w > 0).unsqueeze(-1), targets.double(), torch.zeros((), device=dev, dtype=torch.float64))
        wn = w / w.sum(dim=1, keepdim=True).clamp(min=1e-300)
        ca, cb = (wn.unsqueeze(-1) * src).sum(1, keepdim=True), (wn.unsqueeze(-1) * tgt).sum(1, keepdim=True)
        M = torch.einsum('bk,bki,bkj->bij', wn, tgt - cb, src - ca)                      # sum w (b - cb)(a - ca)^T
        U, _, Vh = torch.linalg.svd(M)
        d = torch.sign(torch.linalg.det(U @ Vh))
        D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=1))
        R = U @ D @ Vh
        omega = _expmap_log(R)
        t_rigid = cb[:, 0] - torch.einsum('bij,bj->bi', R, ca[:, 0].expand(B, 3))
        pelvis_ok = (w[:, 0] > 0) & torch.isfinite(targets[:, 0]).all(dim=1)
        t = torch.where(pelvis_ok.unsqueeze(1), tgt[:, 0], t_rigid)
        pose = torch.cat([omega, torch.zeros(B, 69, device=dev, dtype=torch.float64)], dim=1)
    return {'pose': pose.float(), 'betas': torch.zeros(B, 10, device=dev), 'trans': t.float()}


def _prepare(targets, weights, smpl_layer, h36m_regressor, init, workspace=True):
    if targets.dim() != 3 or tuple(targets.shape[1:]) != (18, 3) or tuple(weights.shape) != (targets.shape[0], 18):
        raise RuntimeError('smpl fit: targets must be [B,18,3] and weights [B,18], got %s and %s'
                           % (tuple(targets.shape), tuple(weights.shape)))
    dev, B = targets.device, targets.shape[0]
    targets = targets.detach().float().contiguous()
    weights = weights.detach().to(device=dev, dtype=torch.float32).contiguous()
    bufs, parents, center = _layer_arrays(smpl_layer, dev)
    V = bufs[0].shape[0]
    reg = h36m_regressor.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(reg.shape) != (17, V):
        raise RuntimeError('smpl fit: h36m_regressor must be [17,%d], got %s' % (V, tuple(reg.shape)))
    if init is None:
        init = default_init(targets, weights, smpl_layer, reg)
    pose, betas, trans = (init[k].detach().to(device=dev, dtype=torch.float32).contiguous() for k in ('pose', 'betas', 'trans'))
    if tuple(pose.shape) != (B, 72) or tuple(betas.shape) != (B, 10) or tuple(trans.shape) != (B, 3):
        raise RuntimeError('smpl fit: init needs pose [B,72], betas [B,10] and trans [B,3]')
    rverts, rcount = compact_regressor(reg)
    ws = None
    if workspace:                                      # xas_smpl_fit's own; the track solver sizes another
        nbytes = query('xas_smpl_fit_workspace_bytes', B, V)
        ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    head = (ptr(pose), ptr(betas), ptr(trans), *(ptr(t) for t in bufs), ptr(parents), ptr(reg), ptr(rverts), ptr(rcount),
            ptr(targets), ptr(weights))
    keep = (pose, betas, trans, bufs, parents, reg, rverts, rcount, targets, weights)
    return head, keep, ws, B, V, center, dev


TRACK_STATUS_CONVERGED, TRACK_STATUS_LIMIT, TRACK_STATUS_NO_FRAME = 0, 1, 2
TRACK_STATUS_NAMES = ('converged', 'trial limit', 'no usable frame')


def _prepare_tracks(targets, weights, track, frame, smpl_layer, h36m_regressor, init):
    """_prepare plus the track table: tracks renumbered 0..S-1 in ascending order of their id (as ops_track.track_bone_lengths
    numbers them).  The one host read is S, the number of distinct ids."""
    head, keep, _, N, V, center, dev = _prepare(targets, weights, smpl_layer, h36m_regressor, init, workspace=False)
    track = torch.as_tensor(track).to(device=dev, dtype=torch.int64).reshape(-1)
    frame = torch.as_tensor(frame).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if track.numel() != N or frame.numel() != N:
        raise RuntimeError('smpl fit tracks: track and frame must hold one entry per sample (%d), got %d and %d'
                           % (N, track.numel(), frame.numel()))
    ids, inv = torch.unique(track, return_inverse=True)
    S = int(ids.numel())
    inv = inv.to(torch.int32).contiguous()
    nbytes = query('xas_smpl_fit_tracks_workspace_bytes', N, V, S)
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    return head + (ptr(inv), ptr(frame)), keep + (inv, frame), ws, N, V, S, center, dev, ids


def linearise_smpl_tracks(targets, weights, track, frame, smpl_layer, h36m_regressor, init=None, lam=1e-3,
                          pose_prior=POSE_PRIOR, shape_prior=SHAPE_PRIOR, workspace=None):
    """One trial of fit_smpl_tracks at the damping `lam` from the start (xas_smpl_fit_tracks_linearise) -> dict: reduced
    [S,10,10], rhs [S,10], d_y [N,75], d_beta [S,10], cost [S] (float64), track_ids [S] (row s belongs to this id)."""
    head, keep, ws, N, V, S, center, dev, ids = _prepare_tracks(targets, weights, track, frame, smpl_layer, h36m_regressor, init)
    ws = _given_workspace(workspace, ws)
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    out = {'reduced': f64(S, 10, 10), 'rhs': f64(S, 10), 'd_y': f64(N, 75), 'd_beta': f64(S, 10), 'cost': f64(S), 'track_ids': ids}
    call('xas_smpl_fit_tracks_linearise', *head, float(pose_prior), float(shape_prior), N, V, S, center, float(lam),
         ptr(out['reduced']), ptr(out['rhs']), ptr(out['d_y']), ptr(out['d_beta']), ptr(out['cost']), ptr(ws))
    return out


def _given_workspace(workspace, ws):
    if workspace is None:
        return ws
    if workspace.dtype != torch.uint8 or workspace.numel() < ws.numel() or workspace.device != ws.device:
        raise RuntimeError('smpl fit tracks: the workspace must be %d bytes (uint8) on %s' % (ws.numel(), ws.device))
    return workspace


def tracks_workspace_bytes(N, V, S):
    return query('xas_smpl_fit_tracks_workspace_bytes', int(N), int(V), int(S))


def fit_smpl_tracks(targets, weights, track, frame, smpl_layer, h36m_regressor, init=None, iters=30, pose_prior=POSE_PRIOR,
                    shape_prior=SHAPE_PRIOR, workspace=None):
    """fit_smpl with one beta vector per track (xas_smpl_fit_tracks; the semantics are those of include/xas_hip.h).  targets
    [N,18,3], weights [N,18]; track [N] any integer ids, frame [N] integers (ops_track.tracks_of), the samples in any order.
    -> dict: pose [N,72], betas [N,10] (each row its track's; a frame passed through keeps its init betas), trans [N,3],
    joints [N,18,3], cost [N,2], all float64; status [N] uint8 (STATUS_CONVERGED = fitted, STATUS_PASSED); track [N] int32
    (0..S-1, ascending id), track_ids [S], track_betas [S,10], track_cost [S,2] float64, track_trials [S] int32, track_status
    [S] uint8 (TRACK_STATUS_*).  workspace: None, or a uint8 tensor of tracks_workspace_bytes to use."""
    head, keep, ws, N, V, S, center, dev, ids = _prepare_tracks(targets, weights, track, frame, smpl_layer, h36m_regressor, init)
    ws = _given_workspace(workspace, ws)
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    out = {'pose': f64(N, 72), 'trans': f64(N, 3), 'joints': f64(N, 18, 3), 'cost': f64(N, 2),
           'status': torch.empty(N, device=dev, dtype=torch.uint8), 'track_betas': f64(S, 10), 'track_cost': f64(S, 2),
           'track_trials': torch.empty(S, device=dev, dtype=torch.int32), 'track_status': torch.empty(S, device=dev, dtype=torch.uint8)}
    call('xas_smpl_fit_tracks', *head, float(pose_prior), float(shape_prior), N, V, S, center, int(iters), ptr(out['pose']),
         ptr(out['trans']), ptr(out['joints']), ptr(out['cost']), ptr(out['status']), ptr(out['track_betas']),
         ptr(out['track_cost']), ptr(out['track_trials']), ptr(out['track_status']), ptr(ws))
    inv, init_betas = keep[-2], keep[1]
    rows = out['track_betas'][inv.long()] if S else f64(N, 10)
    fitted = (out['status'] != STATUS_PASSED).unsqueeze(1)
    out['betas'] = torch.where(fitted, rows, init_betas.double())
    out['track'], out['track_ids'] = inv, ids
    return out


# Weights of the acceleration prior of fit_smpl_tracks_smooth on the 72 angles (mm^2 per rad^2) and on the translation: a second
# difference of 0.01 rad, or of 1 mm, per frame^2 weighs like 1 mm of joint error.  UNTUNED GUESSES, as the priors above.
FIT_SMOOTH_ROT = 1e4
FIT_SMOOTH_TRANS = 1.0


def _prepare_tracks_smooth(targets, weights, track, frame, smpl_layer, h36m_regressor, init, workspace):
    head, keep, _, N, V, S, center, dev, ids = _prepare_tracks(targets, weights, track, frame, smpl_layer, h36m_regressor, init)
    ws = torch.empty(max(tracks_smooth_workspace_bytes(N, V, S), 16), device=dev, dtype=torch.uint8) if workspace is None else None
    if ws is None:
        need = tracks_smooth_workspace_bytes(N, V, S)
        if workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != dev:
            raise RuntimeError('smpl fit tracks: the workspace must be %d bytes (uint8) on %s' % (need, dev))
        ws = workspace
    return head, keep, ws, N, V, S, center, dev, ids


def tracks_smooth_workspace_bytes(N, V, S):
    return query('xas_smpl_fit_tracks_smooth_workspace_bytes', int(N), int(V), int(S))


def linearise_smpl_tracks_smooth(targets, weights, track, frame, smpl_layer, h36m_regressor, init=None, lam=1e-3,
                                 rot_w=FIT_SMOOTH_ROT, trans_w=FIT_SMOOTH_TRANS, pose_prior=POSE_PRIOR, shape_prior=SHAPE_PRIOR,
                                 workspace=None):
    """One trial of fit_smpl_tracks_smooth at the damping `lam` from the start (xas_smpl_fit_tracks_smooth_linearise) -> dict:
    hdiag [N,75,75], hoff [N,2], border [N,10,75], corner [S,10,10], g_y [N,75], g_beta [S,10], d_y [N,75], d_beta [S,10],
    cost [S] (float64), track_ids [S]."""
    head, keep, ws, N, V, S, center, dev, ids = _prepare_tracks_smooth(targets, weights, track, frame, smpl_layer, h36m_regressor,
                                                                         init, workspace)
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    out = {'hdiag': f64(N, 75, 75), 'hoff': f64(N, 2), 'corner': f64(S, 10, 10), 'border': f64(N, 10, 75), 'g_y': f64(N, 75),
           'g_beta': f64(S, 10), 'd_y': f64(N, 75), 'd_beta': f64(S, 10), 'cost': f64(S), 'track_ids': ids}
    call('xas_smpl_fit_tracks_smooth_linearise', *head, float(pose_prior), float(shape_prior), float(rot_w), float(trans_w), N, V, S,
         center, float(lam), *(ptr(out[k]) for k in ('hdiag', 'hoff', 'corner', 'border', 'g_y', 'g_beta', 'd_y', 'd_beta', 'cost')),
         ptr(ws))
    return out


def fit_smpl_tracks_smooth(targets, weights, track, frame, smpl_layer, h36m_regressor, init=None, iters=30, rot_w=FIT_SMOOTH_ROT,
                           trans_w=FIT_SMOOTH_TRANS, pose_prior=POSE_PRIOR, shape_prior=SHAPE_PRIOR, workspace=None):
    """fit_smpl_tracks with an acceleration prior on pose and translation over the frames of a track (xas_smpl_fit_tracks_smooth;
    include/xas_hip.h).  The same dict as fit_smpl_tracks; `cost` [N,2] holds the data cost of a frame alone, `track_cost` the
    whole cost with the prior, and `pose` the root vectors unwrapped along the track.  A usable frame that repeats the frame
    number of the one before it in its track is passed through.  workspace: None, or tracks_smooth_workspace_bytes of uint8."""
    head, keep, ws, N, V, S, center, dev, ids = _prepare_tracks_smooth(targets, weights, track, frame, smpl_layer, h36m_regressor,
                                                                         init, workspace)
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    out = {'pose': f64(N, 72), 'trans': f64(N, 3), 'joints': f64(N, 18, 3), 'cost': f64(N, 2),
           'status': torch.empty(N, device=dev, dtype=torch.uint8), 'track_betas': f64(S, 10), 'track_cost': f64(S, 2),
           'track_trials': torch.empty(S, device=dev, dtype=torch.int32), 'track_status': torch.empty(S, device=dev, dtype=torch.uint8)}
    call('xas_smpl_fit_tracks_smooth', *head, float(pose_prior), float(shape_prior), float(rot_w), float(trans_w), N, V, S, center,
         int(iters), ptr(out['pose']), ptr(out['trans']), ptr(out['joints']), ptr(out['cost']), ptr(out['status']),
         ptr(out['track_betas']), ptr(out['track_cost']), ptr(out['track_trials']), ptr(out['track_status']), ptr(ws))
    inv, init_betas = keep[-2], keep[1]
    rows = out['track_betas'][inv.long()] if S else f64(N, 10)
    fitted = (out['status'] != STATUS_PASSED).unsqueeze(1)
    out['betas'] = torch.where(fitted, rows, init_betas.double())
    out['track'], out['track_ids'] = inv, ids
    return out


def linearise_smpl(targets, weights, smpl_layer, h36m_regressor, init, pose_prior=POSE_PRIOR, shape_prior=SHAPE_PRIOR):
    """Residual r [B,133] and Jacobian J [B,133,85] (float64) at the parameters `init` (xas_smpl_fit_linearise); the unknowns
    are ordered omega 3, t 3, body pose 69, betas 10."""
    head, keep, ws, B, V, center, dev = _prepare(targets, weights, smpl_layer, h36m_regressor, init)
    r = torch.empty(B, 133, device=dev, dtype=torch.float64)
    J = torch.empty(B, 133, 85, device=dev, dtype=torch.float64)
    call('xas_smpl_fit_linearise', *head, float(pose_prior), float(shape_prior), B, V, center, ptr(r), ptr(J), ptr(ws))
    return r, J


def fit_smpl(targets, weights, smpl_layer, h36m_regressor, init=None, iters=30, pose_prior=POSE_PRIOR,
             shape_prior=SHAPE_PRIOR):
    """targets [B,18,3] world mm, weights [B,18] >= 0 (0 = the joint is not used, its target may be anything) -> dict:
    pose [B,72] (root axis-angle first: a PseudoSynth bank row), betas [B,10], trans [B,3] mm, joints [B,18,3] mm, cost [B,2]
    (start, result), all float64; iters [B] int32; status [B] uint8 (STATUS_*).  init: dict(pose, betas, trans) or None =
    default_init.  The semantics are those of include/xas_hip.h."""
    head, keep, ws, B, V, center, dev = _prepare(targets, weights, smpl_layer, h36m_regressor, init)
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    out = {'pose': f64(B, 72), 'betas': f64(B, 10), 'trans': f64(B, 3), 'joints': f64(B, 18, 3), 'cost': f64(B, 2),
           'iters': torch.empty(B, device=dev, dtype=torch.int32), 'status': torch.empty(B, device=dev, dtype=torch.uint8)}
    call('xas_smpl_fit', *head, float(pose_prior), float(shape_prior), B, V, center, int(iters), ptr(out['pose']),
         ptr(out['betas']), ptr(out['trans']), ptr(out['joints']), ptr(out['cost']), ptr(out['iters']), ptr(out['status']),
         ptr(ws))
    return out


# ---- the data term in pixels (csrc/smplfit_views.hip, xas_smpl_fit_views) ------------------------------------------------------
# Weights of the priors against px^2: the mm^2 priors above times 0.1, since roughly 0.3 px per mm (README) gives 0.09 px^2
# per mm^2.  UNTUNED GUESSES, like them.
VIEWS_POSE_PRIOR = 10.0
VIEWS_SHAPE_PRIOR = 2.5
USED_ANCHOR = 0x80                                     # the anchor's bit of `used`; the low bits are the joint's views


def views_workspace_bytes(B, V):
    return query('xas_smpl_fit_views_workspace_bytes', int(B), int(V))


def _prepare_views(points, P, smpl_layer, h36m_regressor, init, views, anchor, info, weighted, huber, anchor_huber, workspace):
    if anchor_huber is None:                           # the smoothers' default, read where it lives and only when a fit asks for it
        from xas_amd.ops_track import TRACK_ANCHOR_HUBER as anchor_huber
    if init is None:
        raise RuntimeError('smpl fit views: init is required (dict(pose, betas, trans)): there is no start from pixels')
    if points.dim() != 4 or tuple(points.shape[2:]) != (18, 3) or tuple(P.shape) != tuple(points.shape[:2]) + (3, 4):
        raise RuntimeError('smpl fit views: points must be [B,C,18,3] and P [B,C,3,4], got %s and %s' % (tuple(points.shape), tuple(P.shape)))
    if (anchor is None) != (info is None):
        raise RuntimeError('smpl fit views: anchor and info come together')
    dev, B, C = points.device, points.shape[0], points.shape[1]
    f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
    points, P = f32(points), f32(P)
    bufs, parents, center = _layer_arrays(smpl_layer, dev)
    V = bufs[0].shape[0]
    reg = f32(h36m_regressor)
    if tuple(reg.shape) != (17, V):
        raise RuntimeError('smpl fit views: h36m_regressor must be [17,%d], got %s' % (V, tuple(reg.shape)))
    pose, betas, trans = (f32(init[k]) for k in ('pose', 'betas', 'trans'))
    if tuple(pose.shape) != (B, 72) or tuple(betas.shape) != (B, 10) or tuple(trans.shape) != (B, 3):
        raise RuntimeError('smpl fit views: init needs pose [B,72], betas [B,10] and trans [B,3]')
    if views is not None:
        views = views.detach().to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(views.shape) != (B, 18):
            raise RuntimeError('smpl fit views: views must be [B,18] bytes, got %s' % (tuple(views.shape),))
    if anchor is not None:
        anchor, info = f32(anchor), f32(info)
        if tuple(anchor.shape) != (B, 18, 3) or tuple(info.shape) != (B, 18, 6):
            raise RuntimeError('smpl fit views: anchor must be [B,18,3] and info [B,18,6], got %s and %s'
                               % (tuple(anchor.shape), tuple(info.shape)))
    rverts, rcount = compact_regressor(reg)
    need = max(views_workspace_bytes(B, V), 16)
    if workspace is None:
        workspace = torch.empty(need, device=dev, dtype=torch.uint8)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != dev:
        raise RuntimeError('smpl fit views: the workspace must be %d bytes (uint8) on %s' % (need, dev))
    head = (ptr(pose), ptr(betas), ptr(trans), *(ptr(t) for t in bufs), ptr(parents), ptr(reg), ptr(rverts), ptr(rcount),
            ptr(points), ptr(P), ptr(views), ptr(anchor), ptr(info), 1 if weighted else 0,      # 1 = XAS_REFINE_WEIGHTED
            float(huber), float(anchor_huber))
    keep = (pose, betas, trans, bufs, parents, reg, rverts, rcount, points, P, views, anchor, info)
    return head, keep, workspace, B, V, C, center, dev


def linearise_smpl_views(points, P, smpl_layer, h36m_regressor, init, views=None, anchor=None, info=None, weighted=False,
                         huber=0.0, anchor_huber=None, pose_prior=VIEWS_POSE_PRIOR, shape_prior=VIEWS_SHAPE_PRIOR, workspace=None):
    """The Gauss-Newton system of fit_smpl_views at `init` (xas_smpl_fit_views_linearise) -> dict: H [B,85,85] (symmetric,
    undamped, priors in), g [B,85], cost [B], joint_blocks [B,18,9] = A_k (xx xy xz yy yz zz) and b_k, float64; used [B,18] uint8."""
    head, keep, ws, B, V, C, center, dev = _prepare_views(points, P, smpl_layer, h36m_regressor, init, views, anchor, info, weighted,
                                                          huber, anchor_huber, workspace)
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    out = {'H': f64(B, 85, 85), 'g': f64(B, 85), 'cost': f64(B), 'joint_blocks': f64(B, 18, 9),
           'used': torch.empty(B, 18, device=dev, dtype=torch.uint8)}
    call('xas_smpl_fit_views_linearise', *head, float(pose_prior), float(shape_prior), B, V, C,
         center, ptr(out['H']), ptr(out['g']), ptr(out['cost']), ptr(out['joint_blocks']), ptr(out['used']), ptr(ws))
    return out


def fit_smpl_views(points, P, smpl_layer, h36m_regressor, init, views=None, anchor=None, info=None, weighted=False, huber=0.0,
                   anchor_huber=None, iters=30, pose_prior=VIEWS_POSE_PRIOR, shape_prior=VIEWS_SHAPE_PRIOR, workspace=None):
    """fit_smpl with the data term in pixels (xas_smpl_fit_views; the semantics are those of include/xas_hip.h): points
    [B,C,18,3] = (u, v, weight) and P [B,C,3,4] as ops_eval's refinement takes them, views [B,18] bytes or None, anchor
    [B,18,3] mm with info [B,18,6] (ops_track.ray_information / covariance_information) or both None; weighted: a view's
    residual is scaled by its weight; huber, anchor_huber (None = ops_track.TRACK_ANCHOR_HUBER): Huber's deltas, 0 = squared.
    init: dict(pose, betas, trans), required.  -> fit_smpl's dict (cost in px^2) plus used [B,18] uint8: the views a joint
    used | USED_ANCHOR."""
    head, keep, ws, B, V, C, center, dev = _prepare_views(points, P, smpl_layer, h36m_regressor, init, views, anchor, info, weighted,
                                                          huber, anchor_huber, workspace)
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    out = {'pose': f64(B, 72), 'betas': f64(B, 10), 'trans': f64(B, 3), 'joints': f64(B, 18, 3), 'cost': f64(B, 2),
           'iters': torch.empty(B, device=dev, dtype=torch.int32), 'status': torch.empty(B, device=dev, dtype=torch.uint8),
           'used': torch.empty(B, 18, device=dev, dtype=torch.uint8)}
    call('xas_smpl_fit_views', *head, float(pose_prior), float(shape_prior), B, V, C, center,
         int(iters), ptr(out['pose']), ptr(out['betas']), ptr(out['trans']), ptr(out['joints']), ptr(out['cost']), ptr(out['iters']),
         ptr(out['status']), ptr(out['used']), ptr(ws))
    return out
