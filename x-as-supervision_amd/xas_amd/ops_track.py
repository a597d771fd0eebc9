"""Temporal smoothing of triangulated joint tracks on the device (csrc/track_smooth.hip, xas_track_smooth): per (track, joint)
the reprojection cost of ops_eval.triangulate_refine in every frame that has data plus a penalty on the acceleration, by a
double-precision Levenberg-Marquardt over all frames of the track at once (block-pentadiagonal Cholesky); frames without data
are filled in from their neighbours.  include/xas_hip.h states the problem and the schedule.  Below it, the same smoother with a
3-D anchor and its information matrix per frame and joint, for one camera or after a volume fusion (csrc/track_anchor.hip,
xas_track_anchor_smooth), that smoother for all joints of a track at once, coupled by the lengths of the bones
(csrc/track_skeleton.hip, xas_track_skeleton_smooth), and one camera's depth hypothesis and left/right exchange chosen over the
frames of a track (csrc/track_resolve.hip, xas_track_resolve).  Imported only when eval.py is given --smooth or --resolve-track.  No reference
counterpart."""
import ctypes
import os
import re

import numpy as np
import torch

from xas_amd._lib import call, ptr, query
from xas_amd.ops_eval import SWITCH_PAIRS, _scatter, _solver_inputs, _sorted, switch_perm

# Weight of the squared acceleration, in px^2 per (mm^2 / frame^3): about 4 mm / frame^2 of acceleration on the scale of a 1 px
# residual (0.05 * 4.5^2 = 1).  AN UNTUNED GUESS: there is neither a dataset nor a checkpoint here to tune it on.
TRACK_ACC_W = 0.05
# Consecutive frames of a sequence further apart than this start a new track.  Untuned as well.
TRACK_MAX_GAP = 8
REFINE_WEIGHTED = 1      # xas_hip.h XAS_REFINE_WEIGHTED

STATUS_SMOOTHED, STATUS_FILLED, STATUS_PASSED = 0, 1, 2
STATUS_NAMES = ('smoothed', 'gap filled', 'passed through')
TRACK_STATUS_NAMES = ('converged', 'trial limit', 'passed through')

_LAST_DIGITS = re.compile(r'(\d+)(?!.*\d)', re.S)


def tracks_of(paths, max_gap=TRACK_MAX_GAP, count=None):
    """paths: one image path per sample, or None with `count` samples -> (track [N] int64, frame [N] int64), numpy.
    The sequence key of a path is the path with the last run of digits of its basename removed, the frame that run as an
    integer (H36M: ..._ca_01_000123.jpg -> frame 123).  Consecutive frames of a key more than `max_gap` apart start a new track.
    Tracks are numbered by the first appearance of their key, then by frame.  A frame that a key holds twice is an error.
    Without paths all samples form one key and the frame is the running index."""
    if paths is None:
        keys, frames = [''] * int(count), list(range(int(count)))
    else:
        keys, frames = [], []
        for p in paths:
            head, base = os.path.split(str(p))
            m = _LAST_DIGITS.search(base)
            if m is None:
                raise RuntimeError('tracks_of: no frame number in %r' % (p,))
            keys.append(os.path.join(head, base[:m.start(1)] + base[m.end(1):]))
            frames.append(int(m.group(1)))
    by_key = {}
    for i, k in enumerate(keys):
        by_key.setdefault(k, []).append(i)
    track, frame, next_id = np.zeros(len(keys), np.int64), np.asarray(frames, np.int64).reshape(-1), 0
    for k, idx in by_key.items():                                      # dicts keep the order of first appearance
        idx.sort(key=lambda i: frames[i])
        for j, i in enumerate(idx):
            if j:
                step = frames[i] - frames[idx[j - 1]]
                if step == 0:
                    raise RuntimeError('tracks_of: frame %d of %r is there twice' % (frames[i], k))
                if step > max_gap:
                    next_id += 1
            track[i] = next_id
        next_id += 1
    return track, frame


def _by_track(name, track, frame):
    """track, frame [N] int64 on the device -> (order [N]: the samples by (track, frame); frame[order] as int32; the track
    numbers, ascending; start [S+1] as the HOST array the kernels take; S).  A frame twice in a track is an error."""
    N = track.shape[0]
    order = torch.argsort(frame, stable=True)
    order = order[torch.argsort(track[order], stable=True)]            # by (track, frame)
    ts, fs = track[order], frame[order]
    if N > 1 and bool(((ts[1:] == ts[:-1]) & (fs[1:] <= fs[:-1])).any()):
        raise RuntimeError('%s: a track holds a frame twice (frame numbers must differ inside a track)' % name)
    if int(fs.abs().max()) >= 1 << 31:
        raise RuntimeError('%s: frame numbers must fit 32 bits' % name)
    ids, counts = torch.unique_consecutive(ts, return_counts=True)     # the host reads: start is a host array
    start = [0]
    for c in counts.tolist():
        start.append(start[-1] + int(c))
    S = len(start) - 1
    return order, fs.to(torch.int32).contiguous(), ids, (ctypes.c_int * (S + 1))(*start), S


def _prepare(name, points, pmat, init, track, frame, views, workspace_of='xas_track_smooth_workspace_bytes'):
    if points.dim() != 4 or points.shape[-1] != 3:
        raise RuntimeError('%s: points must be [N,V,K,3], got %s' % (name, tuple(points.shape)))
    points, pmat, init, views, N, V, K = _solver_inputs(name, points, pmat, init, views, 'N')
    dev = points.device
    track, frame = (torch.as_tensor(t).to(device=dev, dtype=torch.int64) for t in (track, frame))
    if track.shape != (N,) or frame.shape != (N,):
        raise RuntimeError('%s: track %s and frame %s are not one number per sample of points %s' % (
            name, tuple(track.shape), tuple(frame.shape), tuple(points.shape)))
    order, frame, ids, table, S = _by_track(name, track, frame)
    points, pmat, init, views = _sorted(order, points, pmat, init, views)
    ws = torch.empty(max(query(workspace_of, N, K), 16), device=dev, dtype=torch.uint8)
    return points, pmat, init, views, frame, order, ids, table, ws, N, V, K, S


def track_linearise(points, pmat, init, track, frame, views=None, weighted=False, huber_px=0.0, acc_w=TRACK_ACC_W, lam=0.0,
                    workspace=None):
    """One linearisation at the points of init (gap frames filled) with damping `lam` (xas_track_linearise) -> dict, float64:
    band [N,K,3,9] (entry [n,k,c,o] = element (3 t + c, 3 t + c - o) of H + lam diag H, t = the position of sample n in its
    track) and g [N,K,3] in the order given, C [S,K] and tracks [S] (the track numbers, ascending)."""
    points, pmat, init, views, frame, order, ids, table, ws, N, V, K, S = _prepare('track_linearise', points, pmat, init, track,
                                                                                  frame, views)
    dev = points.device
    band = torch.empty(N, K, 3, 9, device=dev, dtype=torch.float64)
    g = torch.empty(N, K, 3, device=dev, dtype=torch.float64)
    C = torch.empty(S, K, device=dev, dtype=torch.float64)
    call('xas_track_linearise', ptr(points), ptr(pmat), ptr(init), ptr(views), table, ptr(frame), N, V, K, S,
         REFINE_WEIGHTED if weighted else 0, float(huber_px), float(acc_w), float(lam), ptr(band), ptr(g), ptr(C),
         ptr(ws if workspace is None else workspace))
    return {'band': _scatter(order, band), 'g': _scatter(order, g), 'C': C, 'tracks': ids}


def track_smooth(points, pmat, init, track, frame, views=None, weighted=False, huber_px=0.0, acc_w=TRACK_ACC_W, max_iter=30,
                 want=('status', 'resid', 'track_status', 'cost', 'trials'), workspace=None):
    """points [N,V,K,3] (u, v, weight), pmat [N,V,3,4], init [N,K,4] and views [N,K] uint8 (or None) as for
    ops_eval.triangulate_refine, over the whole evaluation set; track [N] and frame [N] integers in any order (tracks_of): the
    samples are sorted by (track, frame) for the kernel and the per-sample results put back in the order given.  A frame twice in
    a track is an error.  acc_w: weight of the squared acceleration, px^2 per (mm^2 / frame^3) (TRACK_ACC_W is an untuned guess).
    `workspace`: a uint8 tensor of xas_track_smooth_workspace_bytes(N, K) bytes to use instead of a fresh one (tests).
    -> dict: xyzw [N,K,4]; tracks [S] int64 (the track numbers, ascending: the rows of the per-track outputs); status [N,K]
    uint8 (STATUS_*), resid [N,K,2] (px, before and after; NaN where there is no data), track_status [S,K] uint8, cost [S,K,2]
    float64, trials [S,K] int32 as requested.  The semantics are those of include/xas_hip.h."""
    points, pmat, init, views, frame, order, ids, table, ws, N, V, K, S = _prepare('track_smooth', points, pmat, init, track,
                                                                                  frame, views)
    dev = points.device
    sorted_out = torch.empty(N, K, 4, device=dev)
    per_sample, out = {}, {'tracks': ids}
    if 'status' in want:
        per_sample['status'] = torch.empty(N, K, device=dev, dtype=torch.uint8)
    if 'resid' in want:
        per_sample['resid'] = torch.empty(N, K, 2, device=dev)
    if 'track_status' in want:
        out['track_status'] = torch.empty(S, K, device=dev, dtype=torch.uint8)
    if 'cost' in want:
        out['cost'] = torch.empty(S, K, 2, device=dev, dtype=torch.float64)
    if 'trials' in want:
        out['trials'] = torch.empty(S, K, device=dev, dtype=torch.int32)
    call('xas_track_smooth', ptr(points), ptr(pmat), ptr(init), ptr(views), table, ptr(frame), N, V, K, S,
         REFINE_WEIGHTED if weighted else 0, float(huber_px), float(acc_w), int(max_iter), ptr(sorted_out),
         ptr(per_sample.get('status')), ptr(per_sample.get('resid')), ptr(out.get('track_status')), ptr(out.get('cost')),
         ptr(out.get('trials')), ptr(ws if workspace is None else workspace))
    out['xyzw'] = _scatter(order, sorted_out)
    for k, v in per_sample.items():
        out[k] = _scatter(order, v)
    return out


# ---- smoothing on 3-D anchors (csrc/track_anchor.hip, xas_track_anchor_smooth) ------------------------------------------------
# The smoother above with one more observation per frame and joint: a 3-D point with a 3x3 information matrix.
# Information along the ray of a single camera's point, in px^2 per mm^2: a depth error of 50 mm weighs like a residual of 1 px
# (4e-4 * 50^2 = 1).  AN UNTUNED GUESS: there is neither a dataset nor a checkpoint here to tune it on.
TRACK_DEPTH_W = 4e-4
# Huber delta of the anchor term, in the unit of sqrt(e^T W e): with TRACK_DEPTH_W an anchor 150 mm down its ray, and a fused
# point 3 sigma away, are where the pull stops growing.  Untuned as well.
TRACK_ANCHOR_HUBER = 3.0


def ray_information(pmat, anchor, depth_w=TRACK_DEPTH_W):
    """pmat [N,3,4] (one view's projection matrices) and anchor [N,K,3] (world mm) -> info [N,K,6] float32, the entries xx, xy,
    xz, yy, yz, zz of depth_w r r^T with r the unit vector from the camera centre (-M^-1 p4 of P = [M | p4], in float64) to the
    anchor: what a point on that camera's ray says about its own depth.  Rows of non-finite anchors (or centres) are NaN."""
    P = pmat.detach().double()
    centre = -torch.linalg.solve(P[:, :, :3], P[:, :, 3:])[..., 0]                                  # [N,3]
    r = anchor.detach().double() - centre.unsqueeze(1)
    r = r / r.norm(dim=-1, keepdim=True)
    rows, cols = (0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2)
    info = float(depth_w) * r[..., rows] * r[..., cols]
    bad = ~torch.isfinite(info).all(-1, keepdim=True)
    return torch.where(bad, torch.full_like(info, float('nan')), info).float().contiguous()


def covariance_information(cov):
    """cov [N,K,3,3] (mm^2) -> info [N,K,6] float32: the upper triangle of its inverse in float64, NaN rows where cov is not
    finite or not positive definite."""
    c = cov.detach().double()
    finite = torch.isfinite(c).all(-1).all(-1)
    c = torch.where(finite[..., None, None], 0.5 * (c + c.transpose(-1, -2)), torch.eye(3, dtype=c.dtype, device=c.device))
    L, fail = torch.linalg.cholesky_ex(c)
    ok = finite & (fail == 0)
    L = torch.where(ok[..., None, None], L, torch.eye(3, dtype=c.dtype, device=c.device))
    inv = torch.cholesky_inverse(L)
    rows, cols = (0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2)
    info = inv[..., rows, cols]
    return torch.where(ok.unsqueeze(-1), info, torch.full_like(info, float('nan'))).float().contiguous()


def _anchors(name, anchor, info, order, N, K):
    if (anchor is None) != (info is None):
        raise RuntimeError('%s: anchor and info come together (both given, or both None)' % name)
    if anchor is None:
        return None, None
    anchor, info = (t.detach().float() for t in (anchor, info))
    if anchor.shape != (N, K, 3) or info.shape != (N, K, 6):
        raise RuntimeError('%s: anchor %s and info %s are not [N,K,3] and [N,K,6] of %d samples and %d joints' % (
            name, tuple(anchor.shape), tuple(info.shape), N, K))
    return _sorted(order, anchor, info)


def track_anchor_linearise(points, pmat, init, track, frame, anchor=None, info=None, views=None, weighted=False, huber_px=0.0,
                           anchor_huber=TRACK_ANCHOR_HUBER, acc_w=TRACK_ACC_W, lam=0.0, workspace=None):
    """track_linearise with anchors (xas_track_anchor_linearise): the same dict."""
    name = 'track_anchor_linearise'
    points, pmat, init, views, frame, order, ids, table, ws, N, V, K, S = _prepare(name, points, pmat, init, track, frame, views)
    anchor, info = _anchors(name, anchor, info, order, N, K)
    dev = points.device
    band = torch.empty(N, K, 3, 9, device=dev, dtype=torch.float64)
    g = torch.empty(N, K, 3, device=dev, dtype=torch.float64)
    C = torch.empty(S, K, device=dev, dtype=torch.float64)
    call('xas_track_anchor_linearise', ptr(points), ptr(pmat), ptr(init), ptr(views), ptr(anchor), ptr(info), table, ptr(frame),
         N, V, K, S, REFINE_WEIGHTED if weighted else 0, float(huber_px), float(anchor_huber), float(acc_w), float(lam),
         ptr(band), ptr(g), ptr(C), ptr(ws if workspace is None else workspace))
    return {'band': _scatter(order, band), 'g': _scatter(order, g), 'C': C, 'tracks': ids}


def track_anchor_smooth(points, pmat, init, track, frame, anchor=None, info=None, views=None, weighted=False, huber_px=0.0,
                        anchor_huber=TRACK_ANCHOR_HUBER, acc_w=TRACK_ACC_W, max_iter=30,
                        want=('status', 'resid', 'track_status', 'cost', 'trials'), workspace=None):
    """track_smooth with a 3-D anchor per frame and joint (xas_track_anchor_smooth), for one camera or more (V >= 1): anchor
    [N,K,3] (world mm) and info [N,K,6] (xx, xy, xz, yy, yz, zz of the anchor's information matrix; ray_information,
    covariance_information), or neither: then and with V >= 2 this is track_smooth bit for bit.  A frame with a usable anchor
    (finite, trace > 0) is a data frame whatever its views say, and starts at the anchor where init is not finite; the anchor
    term is Huber's loss of sqrt(e^T W e) with delta anchor_huber (0 = squared; TRACK_ANCHOR_HUBER is an untuned guess).  A
    zero `views` byte stands for all valid views, as in track_smooth: to smooth on the anchors alone give weights of 0.
    Everything else, the sorting by (track, frame) and the dict returned included, as track_smooth; resid is NaN where a frame
    uses no view.  The semantics are those of include/xas_hip.h."""
    name = 'track_anchor_smooth'
    points, pmat, init, views, frame, order, ids, table, ws, N, V, K, S = _prepare(name, points, pmat, init, track, frame, views)
    anchor, info = _anchors(name, anchor, info, order, N, K)
    dev = points.device
    sorted_out = torch.empty(N, K, 4, device=dev)
    per_sample, out = {}, {'tracks': ids}
    if 'status' in want:
        per_sample['status'] = torch.empty(N, K, device=dev, dtype=torch.uint8)
    if 'resid' in want:
        per_sample['resid'] = torch.empty(N, K, 2, device=dev)
    if 'track_status' in want:
        out['track_status'] = torch.empty(S, K, device=dev, dtype=torch.uint8)
    if 'cost' in want:
        out['cost'] = torch.empty(S, K, 2, device=dev, dtype=torch.float64)
    if 'trials' in want:
        out['trials'] = torch.empty(S, K, device=dev, dtype=torch.int32)
    call('xas_track_anchor_smooth', ptr(points), ptr(pmat), ptr(init), ptr(views), ptr(anchor), ptr(info), table, ptr(frame),
         N, V, K, S, REFINE_WEIGHTED if weighted else 0, float(huber_px), float(anchor_huber), float(acc_w), int(max_iter),
         ptr(sorted_out), ptr(per_sample.get('status')), ptr(per_sample.get('resid')), ptr(out.get('track_status')),
         ptr(out.get('cost')), ptr(out.get('trials')), ptr(ws if workspace is None else workspace))
    out['xyzw'] = _scatter(order, sorted_out)
    for k, v in per_sample.items():
        out[k] = _scatter(order, v)
    return out


# ---- all joints of a track at once, coupled by bone lengths (csrc/track_skeleton.hip, xas_track_skeleton_smooth) -------------
# Weight of a squared bone-length error, in px^2 per mm^2: 3 mm of length error weigh like a residual of 1 px (0.1 * 3.2^2 = 1),
# the reasoning of ops_eval.TRI_SYM_W.  AN UNTUNED GUESS: there is neither a dataset nor a checkpoint here to tune it on.
TRACK_BONE_W = 0.1
TRACK_MAX_BONES = 32     # xas_hip.h XAS_TRACK_MAX_BONES
SKELETON_TRACK_STATUS_NAMES = ('converged', 'trial limit', 'no free joint')


def bones_of(parent_ids):
    """parent_ids [K] (model_params.parent_ids) -> the rows (k, parent_ids[k]) of the joints that have a parent other than
    themselves (parent_ids[k] >= 0 and != k), as an int32 numpy array [Bn,2]."""
    rows = [(k, int(p)) for k, p in enumerate(parent_ids) if int(p) >= 0 and int(p) != k]
    return np.asarray(rows, np.int32).reshape(-1, 2)


def track_bone_lengths(init, track, frame, bones, usable=None):
    """init [N,K,>=3] (mm), track [N] and frame [N] integers (frame is not read: the argument list is the smoothers'), bones
    [Bn,2] -> length [S,Bn] float32 on init's device, row s for the s-th track number in ascending order: the median of
    |init_i - init_j| over the track's frames where both joints are finite (and `usable` [N,K] holds for both, if given), the
    mean of the two middle values for an even count; NaN where no frame qualifies.  Set-up in plain torch, not hot path."""
    x = init.detach()[..., :3].double()
    bones = torch.as_tensor(np.asarray(bones, np.int64).reshape(-1, 2), device=x.device)
    track = torch.as_tensor(track).to(device=x.device, dtype=torch.int64)
    ids, inv = torch.unique(track, return_inverse=True)
    ok = torch.isfinite(x).all(-1)
    if usable is not None:
        ok = ok & usable.to(x.device).bool()
    okb = ok[:, bones[:, 0]] & ok[:, bones[:, 1]]                                                  # [N,Bn]
    length = (x[:, bones[:, 0]] - x[:, bones[:, 1]]).norm(dim=-1)
    length = torch.where(okb, length, torch.full_like(length, float('nan')))
    out = torch.full((len(ids), bones.shape[0]), float('nan'), dtype=torch.float64, device=x.device)
    for s in range(len(ids)):
        rows, cnt = torch.sort(length[inv == s], dim=0).values, okb[inv == s].sum(0)                 # NaN sorts last
        lo, hi = ((cnt - 1).clamp(min=0) // 2).unsqueeze(0), (cnt // 2).clamp(max=rows.shape[0] - 1).unsqueeze(0)
        mid = 0.5 * (rows.gather(0, lo) + rows.gather(0, hi))[0]
        out[s] = torch.where(cnt > 0, mid, torch.full_like(mid, float('nan')))
    return out.float().contiguous()


def _skeleton(name, init, track, bones, length, S):
    """The bones as the HOST array the kernel takes, and length [S,Bn] float32 in the order of `ids`."""
    bones = np.ascontiguousarray(np.asarray(bones, np.int64).reshape(-1, 2))
    Bn = bones.shape[0]
    if Bn > TRACK_MAX_BONES:
        raise RuntimeError('%s: %d bones (at most XAS_TRACK_MAX_BONES = %d)' % (name, Bn, TRACK_MAX_BONES))
    if length is None:
        length = track_bone_lengths(init, track, None, bones)
    length = torch.as_tensor(length).detach().to(device=init.device, dtype=torch.float32).contiguous()
    if length.shape != (S, Bn):
        raise RuntimeError('%s: length %s is not [S,Bn] = [%d,%d]' % (name, tuple(length.shape), S, Bn))
    return (ctypes.c_int * max(2 * Bn, 1))(*bones.reshape(-1).tolist()), length, Bn


def _own_workspace(name, ws, workspace):
    """The caller's workspace in place of the fresh one `ws`, if it is given and holds at least as many bytes."""
    if workspace is None:
        return ws
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < ws.numel():
        raise RuntimeError('%s: workspace must be a contiguous uint8 tensor of at least %d bytes (xas_track_skeleton_workspace_bytes), '
                           'got %s of %d' % (name, ws.numel(), workspace.dtype, workspace.numel()))
    return workspace


def track_skeleton_linearise(points, pmat, init, track, frame, bones, length=None, anchor=None, info=None, views=None,
                             weighted=False, huber_px=0.0, anchor_huber=TRACK_ANCHOR_HUBER, acc_w=TRACK_ACC_W,
                             bone_w=TRACK_BONE_W, lam=0.0, workspace=None):
    """One linearisation of track_skeleton_smooth's problem at the start with damping `lam` (xas_track_skeleton_linearise) ->
    dict, float64, per-sample entries in the order given: g [N,K,3], hdiag [N,3K,3K], hoff [N,2], d [N,K,3] (the trial step),
    C [S] and tracks [S]."""
    name = 'track_skeleton_linearise'
    raw_init, raw_track = init, torch.as_tensor(track)
    points, pmat, init, views, frame, order, ids, table, ws, N, V, K, S = _prepare(name, points, pmat, init, track, frame, views,
                                                                                  'xas_track_skeleton_workspace_bytes')
    anchor, info = _anchors(name, anchor, info, order, N, K)
    host_bones, length, Bn = _skeleton(name, raw_init, raw_track, bones, length, S)
    dev = points.device
    ws = _own_workspace(name, ws, workspace)
    g = torch.empty(N, K, 3, device=dev, dtype=torch.float64)
    hdiag = torch.empty(N, 3 * K, 3 * K, device=dev, dtype=torch.float64)
    hoff = torch.empty(N, 2, device=dev, dtype=torch.float64)
    d = torch.empty(N, K, 3, device=dev, dtype=torch.float64)
    C = torch.empty(S, device=dev, dtype=torch.float64)
    call('xas_track_skeleton_linearise', ptr(points), ptr(pmat), ptr(init), ptr(views), ptr(anchor), ptr(info), host_bones,
         ptr(length), table, ptr(frame), N, V, K, S, Bn, REFINE_WEIGHTED if weighted else 0, float(huber_px), float(anchor_huber),
         float(acc_w), float(bone_w), float(lam), ptr(g), ptr(hdiag), ptr(hoff), ptr(d), ptr(C), ptr(ws))
    return {'g': _scatter(order, g), 'hdiag': _scatter(order, hdiag), 'hoff': _scatter(order, hoff), 'd': _scatter(order, d),
            'C': C, 'tracks': ids}


def track_skeleton_smooth(points, pmat, init, track, frame, bones, length=None, anchor=None, info=None, views=None,
                          weighted=False, huber_px=0.0, anchor_huber=TRACK_ANCHOR_HUBER, acc_w=TRACK_ACC_W, bone_w=TRACK_BONE_W,
                          max_iter=30, want=('status', 'resid', 'bone', 'track_status', 'cost', 'trials'), workspace=None):
    """track_anchor_smooth for all joints of a track at once, coupled in every frame (gap frames included) by the lengths of
    the bones (xas_track_skeleton_smooth): bones [Bn,2] joint indices (bones_of), length [S,Bn] mm per track in ascending track
    number, or None: track_bone_lengths of init; bone_w in px^2 per mm^2 (TRACK_BONE_W is an untuned guess).  Everything else,
    the sorting by (track, frame) included, as track_anchor_smooth.  A (track, joint) with fewer than two data frames is fixed:
    it leaves as init and its bones are switched off.
    -> dict: xyzw [N,K,4]; tracks [S]; status [N,K] uint8, resid [N,K,2], bone [N,Bn,2] (the bone's length error in mm before
    and after; NaN where it is not active), track_status [S] uint8 (SKELETON_TRACK_STATUS_NAMES), cost [S,2] float64, trials
    [S] int32 as requested; length [S,Bn], the lengths used.  The semantics are those of include/xas_hip.h."""
    name = 'track_skeleton_smooth'
    raw_init, raw_track = init, torch.as_tensor(track)
    points, pmat, init, views, frame, order, ids, table, ws, N, V, K, S = _prepare(name, points, pmat, init, track, frame, views,
                                                                                  'xas_track_skeleton_workspace_bytes')
    anchor, info = _anchors(name, anchor, info, order, N, K)
    host_bones, length, Bn = _skeleton(name, raw_init, raw_track, bones, length, S)
    dev = points.device
    ws = _own_workspace(name, ws, workspace)
    sorted_out = torch.empty(N, K, 4, device=dev)
    per_sample, out = {}, {'tracks': ids, 'length': length}
    if 'status' in want:
        per_sample['status'] = torch.empty(N, K, device=dev, dtype=torch.uint8)
    if 'resid' in want:
        per_sample['resid'] = torch.empty(N, K, 2, device=dev)
    if 'bone' in want:
        per_sample['bone'] = torch.empty(N, Bn, 2, device=dev)
    if 'track_status' in want:
        out['track_status'] = torch.empty(S, device=dev, dtype=torch.uint8)
    if 'cost' in want:
        out['cost'] = torch.empty(S, 2, device=dev, dtype=torch.float64)
    if 'trials' in want:
        out['trials'] = torch.empty(S, device=dev, dtype=torch.int32)
    call('xas_track_skeleton_smooth', ptr(points), ptr(pmat), ptr(init), ptr(views), ptr(anchor), ptr(info), host_bones,
         ptr(length), table, ptr(frame), N, V, K, S, Bn, REFINE_WEIGHTED if weighted else 0, float(huber_px), float(anchor_huber),
         float(acc_w), float(bone_w), int(max_iter), ptr(sorted_out), ptr(per_sample.get('status')), ptr(per_sample.get('resid')),
         ptr(per_sample.get('bone')), ptr(out.get('track_status')), ptr(out.get('cost')), ptr(out.get('trials')), ptr(ws))
    out['xyzw'] = _scatter(order, sorted_out)
    for k, v in per_sample.items():
        out[k] = _scatter(order, v)
    return out


# ---- depth hypothesis and left/right exchange over time (csrc/track_resolve.hip, xas_track_resolve) --------------------------
# One camera, no labels: per track and unit (a left/right pair, or a joint without partner) the exact minimum over all
# labellings of a motion cost in world mm plus priors towards hypothesis 0 and towards "not exchanged".  The weights: one rank
# step or one exchange costs what a jump of 20 mm between consecutive frames costs (400 = 20^2).  UNTUNED GUESSES from a
# synthetic float64 experiment (decoys 250-600 mm along the ray, 5 mm noise): there is neither a dataset nor a checkpoint here.
TRACK_VEL_W = 1.0
TRACK_HYP_W = 400.0
TRACK_SWAP_W = 400.0
TRACK_MAX_HYPO = 5       # xas_hip.h XAS_TRACK_MAX_HYPO
RESOLVE_RESOLVED, RESOLVE_PASSED = 0, 1
RESOLVE_STATUS_NAMES = ('resolved', 'passed through')


def resolved_gather(x, hyp, swap, perm):
    """x [N,Hy,K,C] -> [N,K,C]: joint k from hypothesis hyp[n,k] of channel perm[k] where swap[n,k], else of channel k."""
    N, _, K, _ = x.shape
    own = torch.arange(K, device=x.device)
    chan = torch.where(swap.bool(), perm.long().unsqueeze(0), own.unsqueeze(0))
    return x[torch.arange(N, device=x.device).unsqueeze(1), hyp.long(), chan]


def track_resolve(kps, world, track, frame, pairs=SWITCH_PAIRS, unary=None, vel_w=TRACK_VEL_W, hyp_w=TRACK_HYP_W,
                  swap_w=TRACK_SWAP_W, gt=None, image_size=256.0, want=('hyp', 'swap', 'status', 'cost'), workspace=None):
    """kps [N,Hy,K,3] (one camera's patch-normalised joints) and world [N,Hy,K,3] (their single-view world points, mm) over the
    whole evaluation set, unary [N,Hy,K] an extra cost per candidate or None; track [N] and frame [N] integers in any order
    (tracks_of): the samples are sorted by (track, frame) for the kernel and the per-sample results put back in the order
    given.  A frame twice in a track is an error.  The cost, the states and the rules are those of include/xas_hip.h.
    gt [N,K,>=2] labels in patch pixels or None.  They only NAME each pair, once per track: if the track's summed |dx| + |dy|
    of both joints against the labels (normalised with image_size as eval_select does; the measure of switch_points) is
    strictly smaller with every exchange bit of the track flipped, all are flipped (passed-through frames too) and
    named[s, a] = named[s, b] = 1.  Flipped means the mirror labelling, which costs the same motion: the two curves stay as
    chosen and trade their names, so sel and hyp of a and b trade places.  One bit per (track, pair), never per frame; a
    few torch ops on the device.
    `workspace`: a uint8 tensor of xas_track_resolve_workspace_bytes(N, Hy, K) bytes to use instead of a fresh one (tests).
    -> dict: sel [N,K,3]; tracks [S] int64 (the track numbers, ascending: the rows of the per-track outputs); hyp, swap, status
    [N,K] uint8 (RESOLVE_*) and cost [S,K] float64 as requested; named [S,K] uint8 with gt."""
    kps, world = (t.detach().float().contiguous() for t in (kps, world))
    if kps.dim() != 4 or kps.shape[-1] != 3:
        raise RuntimeError('track_resolve: kps must be [N,Hy,K,3], got %s' % (tuple(kps.shape),))
    N, Hy, K, _ = kps.shape
    if world.shape != kps.shape:
        raise RuntimeError('track_resolve: world %s and kps %s differ' % (tuple(world.shape), tuple(kps.shape)))
    if unary is not None and unary.shape != (N, Hy, K):
        raise RuntimeError('track_resolve: unary %s is not one value per candidate of kps %s' % (tuple(unary.shape), tuple(kps.shape)))
    if gt is not None and (gt.dim() != 3 or gt.shape[:2] != (N, K) or gt.shape[2] < 2):
        raise RuntimeError('track_resolve: labels %s do not match kps %s' % (tuple(gt.shape), tuple(kps.shape)))
    dev = kps.device
    track, frame = (torch.as_tensor(t).to(device=dev, dtype=torch.int64) for t in (track, frame))
    if track.shape != (N,) or frame.shape != (N,):
        raise RuntimeError('track_resolve: track %s and frame %s are not one number per sample of kps %s' % (
            tuple(track.shape), tuple(frame.shape), tuple(kps.shape)))
    order, frame, ids, table, S = _by_track('track_resolve', track, frame)
    kps, world = kps[order].contiguous(), world[order].contiguous()
    unary = None if unary is None else unary.detach().float()[order].contiguous()
    perm = switch_perm(K, pairs, dev)
    host_perm = (ctypes.c_int * K)(*perm.tolist())                     # a HOST array, like start (xas_hip.h)
    ws = workspace
    if ws is None:
        ws = torch.empty(max(query('xas_track_resolve_workspace_bytes', N, Hy, K), 16), device=dev, dtype=torch.uint8)
    sel = torch.empty(N, K, 3, device=dev)
    byte = lambda name: torch.empty(N, K, device=dev, dtype=torch.uint8) if name in want or (gt is not None and name != 'status') else None
    hyp, swap, status = byte('hyp'), byte('swap'), byte('status')
    cost = torch.empty(S, K, device=dev, dtype=torch.float64) if 'cost' in want else None
    call('xas_track_resolve', ptr(kps), ptr(world), ptr(unary), host_perm, table, ptr(frame), N, Hy, K, S, float(vel_w),
         float(hyp_w), float(swap_w), ptr(sel), ptr(hyp), ptr(swap), ptr(status), ptr(cost), ptr(ws))
    out = {'tracks': ids}
    if gt is not None:
        g = gt.detach().float()[order][..., :2] / (float(image_size) - 1.0) * 2.0 - 1.0
        paired = (perm.long() != torch.arange(K, device=dev)).unsqueeze(0)                           # [1,K]
        flipped = sel[:, perm.long()]
        l1 = lambda p: (p[..., :2] - g).abs().sum(-1).double()
        d = l1(flipped) - l1(sel)                                       # [N,K] < 0: the flipped frame lies closer
        d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
        d = d + d[:, perm.long()]                                       # both joints of the pair, the same sum on either
        run = torch.cat([torch.zeros(1, K, device=dev, dtype=torch.float64), d.cumsum(0)])
        start = torch.tensor(list(table), device=dev)
        named = ((run[start[1:]] - run[start[:-1]]) < 0) & paired      # [S,K]
        rows = torch.repeat_interleave(named, start[1:] - start[:-1], dim=0)                          # [N,K]
        swap = swap ^ rows.to(torch.uint8)
        sel, hyp = torch.where(rows.unsqueeze(-1), flipped, sel), torch.where(rows, hyp[:, perm.long()], hyp)
        out['named'] = named.to(torch.uint8)
    out['sel'] = _scatter(order, sel)
    for name, t in (('hyp', hyp), ('swap', swap), ('status', status)):
        if name in want:
            out[name] = _scatter(order, t)
    if cost is not None:
        out['cost'] = cost
    return out
