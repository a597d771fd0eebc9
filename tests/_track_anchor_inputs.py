"""Synthetic joint tracks with 3-D anchors for the tests of xas_track_anchor_smooth and for tools/bench_track_anchor.py: numpy
only, seeded.  The tracks, cameras and detections are _track_inputs.build's; this adds, per frame and joint, an anchor and its
information matrix:
  'ray'   a point on the ray of camera 0 through the true point, off by depth noise along the ray and 2 mm across it, with
          info = depth_w r r^T (rank one; numpy's float64 restatement of ops_track.ray_information, rounded to float32)
  'full'  the true point plus noise of a random covariance (axes of 5-30 mm), with info = its inverse (full rank)
With one camera the start (init) is the anchor itself, as eval.py hands it over."""
import numpy as np

import _track_inputs as ti

DEPTH_W = 4e-4
ANCHOR_HUBER = 3.0
TRI = ((0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2))


def centres(P):
    """Camera centres [N,V,3] of P [N,V,3,4], float64."""
    P = np.asarray(P, np.float64)
    return -np.linalg.solve(P[..., :3], P[..., 3:])[..., 0]


def ray_info(P0, anchor, depth_w):
    """depth_w r r^T as [N,K,6] float32, r from the centre of P0 [N,3,4] to anchor [N,K,3]; NaN rows for non-finite anchors."""
    r = np.asarray(anchor, np.float64) - centres(P0[:, None])[:, 0][:, None]
    with np.errstate(all='ignore'):
        r = r / np.linalg.norm(r, axis=-1, keepdims=True)
        info = depth_w * r[..., TRI[0]] * r[..., TRI[1]]
    info[~np.isfinite(info).all(-1)] = np.nan
    return np.ascontiguousarray(info, np.float32)                      # an index list on the last axis leaves it strided


def build(lengths, K, V, seed, kind='ray', depth_w=DEPTH_W, depth_mm=30.0, anchor_huber=0.0, off=False, anchor_nan=(), zero_trace=(),
          decoy=(), shift=0.0, **base):
    """_track_inputs.build(lengths, K, V, seed, **base) plus `anchor` [N,K,3], `info` [N,K,6] and `anchor_huber`.
    off: the reprojection term switched off (every weight 0, every `views` byte 0).  anchor_nan / zero_trace / decoy: (track,
    position, joint) triples: that anchor NaN; its info all zero; the anchor moved 400 mm down its ray.  shift: every world
    coordinate moved by this much (mm), the cameras with them, so the pixels stay.  The triples `nan` and `behind` of the base
    act on init as there (with one camera after init was set to the anchor)."""
    nan, behind = base.pop('nan', ()), base.pop('behind', ())
    c = ti.build(lengths, K, V, seed, **base)
    rng = np.random.Generator(np.random.PCG64(seed + 7000))
    first = np.concatenate([[0], np.cumsum(lengths)])
    N, truth, P = c['N'], c['truth'].astype(np.float64), c['P']
    if shift:
        d = np.full(3, float(shift))
        P = P.astype(np.float64)
        P[..., 3] -= P[..., :3] @ d
        P = P.astype(np.float32)
        truth = truth + d
        c['init'][..., :3] += d.astype(np.float32)
        c['P'], c['truth'] = P, truth.astype(np.float32)
    r = truth - centres(P)[:, 0][:, None]
    r /= np.linalg.norm(r, axis=-1, keepdims=True)
    if kind == 'ray':
        anchor = truth + r * rng.normal(0.0, depth_mm, (N, K, 1)) + rng.normal(0.0, 2.0, (N, K, 3))
    else:
        Q = np.linalg.qr(rng.normal(size=(N, K, 3, 3)))[0]
        sd = rng.uniform(5.0, 30.0, (N, K, 3))
        anchor = truth + np.einsum('nkij,nkj->nki', Q, sd * rng.normal(size=(N, K, 3)))
        W = np.einsum('nkij,nkj,nklj->nkil', Q, 1.0 / sd ** 2, Q)
    for s, t, k in decoy:
        anchor[first[s] + t, k] += 400.0 * r[first[s] + t, k]
    anchor = anchor.astype(np.float32)
    info = ray_info(P[:, 0], anchor, depth_w) if kind == 'ray' else W[..., TRI[0], TRI[1]].astype(np.float32)
    for s, t, k in anchor_nan:
        anchor[first[s] + t, k, rng.integers(0, 3)] = np.nan
    for s, t, k in zero_trace:
        info[first[s] + t, k] = 0.0
    if V == 1:
        c['init'] = np.concatenate([anchor, np.ones((N, K, 1), np.float32)], -1)
    if off:
        c['points'][..., 2] = 0.0
        c['views'] = np.zeros((N, K), np.uint8)
    for s, t, k in nan:
        c['init'][first[s] + t, k, :3] = np.nan
    for s, t, k in behind:
        n = first[s] + t
        cen = centres(P[n:n + 1])[0, 0]
        c['init'][n, k, :3] = (cen + 0.5 * (cen - truth[n, k])).astype(np.float32)
    c.update(anchor=anchor, info=info, anchor_huber=float(anchor_huber))
    return c


# Every T at which the lanes' stride changes, both ends of K and V, each kind of anchor, every rule of the header once.
# One camera and a rank-one anchor are three equations for a frame's three unknowns: where the prior adds none (T = 2, acc_w =
# 0, or as many gap frames as stencils) the minimum has cost 0, the trials near it change the cost by rounding alone, and no
# oracle can say which of them an implementation accepts.  Those shapes take two cameras here; with T >= 3 the prior
# overdetermines the problem and one camera is the rule.
CASES = {
    'T1_V1': dict(lengths=[1], K=1, V=1, seed=41),                                                   # one data frame: passed through
    'T2_V2': dict(lengths=[2], K=3, V=2, seed=42, kind='full'),
    'T3_V2_full': dict(lengths=[3], K=1, V=2, seed=43, kind='full', huber=1.0),                      # Huber on the pixels alone
    'T4_V1_gaps': dict(lengths=[4], K=3, V=1, seed=44, anchor_nan=[(0, 0, 0), (0, 3, 1), (0, 1, 2)]),
    'T63_V1_decoys': dict(lengths=[63], K=1, V=1, seed=45, anchor_huber=3.0, decoy=[(0, 5, 0), (0, 30, 0), (0, 31, 0), (0, 62, 0)]),
    # anchors alone, full rank: F is empty in every frame; NaN anchors at either end and in the middle are gap frames
    'T64_V4_anchors_only': dict(lengths=[64], K=3, V=4, seed=46, kind='full', off=True, anchor_huber=3.0,
                                anchor_nan=[(0, 0, 0), (0, 1, 0), (0, 63, 1), (0, 20, 2), (0, 21, 2), (0, 40, 2)]),
    # K = 18, weighted, init NaN beside a usable anchor (the start is the anchor), zero-trace info (not usable: a gap with one view)
    'T65_V1_K18': dict(lengths=[65], K=18, V=1, seed=47, weighted=True, nan=[(0, 0, 4), (0, 33, 4), (0, 64, 17)],
                       zero_trace=[(0, 10, 9), (0, 11, 9), (0, 64, 9)]),
    # two views and anchors, both Hubers active, coordinates of 1e4 mm, a start behind camera 0 beside a usable anchor, a frame
    # without an anchor that is a data frame by its views, one without either
    'T130_V2_1e4': dict(lengths=[130], K=3, V=2, seed=48, kind='full', huber=2.5, anchor_huber=1.0, shift=1e4, behind=[(0, 50, 1)],
                        anchor_nan=[(0, 70, 2), (0, 90, 2)], gaps=[(0, 90, 2)], max_iter=10),
    'several_V1': dict(lengths=[1, 3, 4, 7, 20, 66, 130], K=3, V=1, seed=49, views=True, anchor_huber=3.0,
                       anchor_nan=[(3, 0, 0), (4, 8, 1), (4, 9, 1), (4, 19, 2), (5, 0, 0), (5, 65, 0), (6, 64, 1)],
                       decoy=[(4, 3, 0), (5, 40, 1), (6, 100, 2)], nan=[(5, 10, 2)], zero_trace=[(1, 0, 0), (1, 1, 0), (1, 2, 0)]),
    'acc_w_0_V2': dict(lengths=[6, 3], K=3, V=2, seed=50, acc_w=0.0, max_iter=12),
}


def make(name):
    return dict(build(**CASES[name]), name=name)


def planted(seed=61):
    """The monocular effect case: one 130-frame track, one camera, K = 18, 2 px of pixel noise, 30 mm of depth noise, and 10 % of
    the frames of every third joint on a decoy 250-600 mm along the ray."""
    T, K = 130, 18
    c = build([T], K, 1, seed, uniform=True, sigma=2.0, anchor_huber=ANCHOR_HUBER)
    rng = np.random.Generator(np.random.PCG64(seed + 9000))
    cen = centres(c['P'])[:, 0]
    anchor = c['anchor'].astype(np.float64)
    decoys = np.zeros((T, K), bool)
    for k in range(0, K, 3):
        t = rng.choice(T, T // 10, replace=False)
        r = anchor[t, k] - cen[t]
        r /= np.linalg.norm(r, axis=-1, keepdims=True)
        anchor[t, k] += r * (rng.uniform(250.0, 600.0, (len(t), 1)) * rng.choice([-1.0, 1.0], (len(t), 1)))
        decoys[t, k] = True
    c['anchor'] = anchor.astype(np.float32)
    c['info'] = ray_info(c['P'][:, 0], c['anchor'], DEPTH_W)
    c['init'] = np.concatenate([c['anchor'], np.ones((T, K, 1), np.float32)], -1)
    return dict(c, name='planted', decoys=decoys)
