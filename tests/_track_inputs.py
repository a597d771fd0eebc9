"""Synthetic joint tracks for the tests of xas_track_smooth and for tools/bench_track_smooth.py: numpy only, seeded.  Cameras
from _refine_inputs.ring_rig (one rig per track, the same in all its frames), joints on smooth sinusoidal trajectories,
detections with _refine_inputs.noisy's pixel noise, the start from the float64 DLT (_refine_oracle.dlt_start)."""
import numpy as np

import _refine_inputs as ri

ACC_W = 0.05


def trajectory(frames, K, rng):
    """Smooth world tracks [T,K,3] in mm: per joint and axis a base point plus a sinusoid of 100-300 mm with a period of 40-120
    frames: at most ~7 mm / frame^2 of acceleration."""
    base = rng.normal(0.0, 350.0, (K, 3))
    amp, per, ph = rng.uniform(100, 300, (K, 3)), rng.uniform(40, 120, (K, 3)), rng.uniform(0, 2 * np.pi, (K, 3))
    return (base + amp * np.sin(2 * np.pi * np.asarray(frames, np.float64)[:, None, None] / per + ph)).astype(np.float32)


def build(lengths, K, V, seed, weighted=False, huber=0.0, views=False, acc_w=ACC_W, uniform=False, sigma=ri.SIGMA_PX, gaps=(), nan=(),
          behind=(), max_iter=8):
    """Tracks of the given lengths, sorted by (track, frame).  gaps / nan / behind: (track, position, joint) triples: every
    weight of that joint 0; its start NaN; its start behind camera 0."""
    from _refine_oracle import dlt_start
    rng = np.random.Generator(np.random.PCG64(seed))
    pts, P, truth, track, frame = [], [], [], [], []
    for s, T in enumerate(lengths):
        steps = np.ones(T, np.int64) if uniform else rng.integers(1, 4, T)
        fr = 100 * s + np.cumsum(steps)
        _, Ps, _ = ri.ring_rig(1, V, K, seed * 1000 + s)
        Pt = np.repeat(Ps, T, 0)
        world = trajectory(fr, K, rng)
        p, _, _ = ri.noisy((ri.project(Pt, world), Pt, world), seed * 1000 + 500 + s, sigma)
        if weighted:
            p[..., 2] = rng.uniform(0.3, 1.0, p.shape[:3]).astype(np.float32)
        pts.append(p); P.append(Pt); truth.append(world); track.append(np.full(T, s)); frame.append(fr)
    pts, P, truth = np.concatenate(pts), np.concatenate(P), np.concatenate(truth)
    track, frame = np.concatenate(track).astype(np.int64), np.concatenate(frame).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(lengths)])
    for s, t, k in gaps:
        pts[first[s] + t, :, k, 2] = 0.0
    vw = None
    if views:                                                   # a byte per joint: all views, or all but one, or none (= all)
        vw = rng.choice(np.array([0, (1 << V) - 1, ((1 << V) - 1) & ~2], np.uint8), (len(track), K)).astype(np.uint8)
        if V == 2:
            vw[:] = np.where(vw == 1, 3, vw)
    init = dlt_start(pts, P, vw)
    for s, t, k in nan:
        init[first[s] + t, k, :3] = np.nan
    for s, t, k in behind:
        n = first[s] + t
        M, p4 = P[n, 0, :, :3].astype(np.float64), P[n, 0, :, 3].astype(np.float64)
        c = -np.linalg.solve(M, p4)
        init[n, k, :3] = (c + 0.5 * (c - truth[n, k])).astype(np.float32)
    return dict(points=pts, P=P, init=init, views=vw, track=track, frame=frame, truth=truth, weighted=weighted, huber=float(huber),
                acc_w=float(acc_w), max_iter=max_iter, N=len(track), V=V, K=K, S=len(lengths), lengths=list(lengths))


# the linearise cases: every T at which the lanes' stride or the band's shape changes, both ends of V and K, every option
LINEARISE = {
    'T3': dict(lengths=[3], K=1, V=2, seed=11),
    'T5': dict(lengths=[5], K=18, V=6, seed=12, weighted=True),
    'T64': dict(lengths=[64], K=1, V=4, seed=13, huber=2.5),
    'T65': dict(lengths=[65], K=2, V=2, seed=14, views=True, gaps=[(0, 30, 1)]),
    'T130': dict(lengths=[130], K=2, V=3, seed=15, views=True, weighted=True, huber=1.0),
}

# the smoothing cases
SMOOTH = {
    'T1': dict(lengths=[1], K=2, V=3, seed=21, nan=[(0, 0, 1)]),
    'one_data_frame': dict(lengths=[4], K=2, V=3, seed=22, gaps=[(0, 0, 0), (0, 2, 0), (0, 3, 0)], nan=[(0, 1, 1), (0, 2, 1), (0, 3, 1)]),
    'T2': dict(lengths=[2], K=2, V=3, seed=23),
    'T3': dict(lengths=[3], K=2, V=2, seed=24),
    'T5': dict(lengths=[5], K=18, V=6, seed=25, weighted=True, huber=1.5),
    'several': dict(lengths=[1, 2, 3, 7, 20, 66], K=3, V=4, seed=26, views=True,
                    gaps=[(3, 0, 0), (4, 8, 1), (4, 9, 1), (4, 10, 1), (4, 19, 2), (5, 0, 0), (5, 1, 0), (5, 65, 0)],
                    nan=[(4, 3, 0), (5, 40, 1)], behind=[(4, 5, 2), (5, 20, 2)]),
    'acc_w_0': dict(lengths=[6, 3], K=3, V=4, seed=27, acc_w=0.0, max_iter=30),
}


def make(table, name):
    return dict(build(**table[name]), name=name)


def planted(seed=31):
    """The effect case: one 130-frame track, V = 4, K = 18, sigma = 2 px, three consecutive frames of joint 5 without data."""
    return dict(build([130], 18, 4, seed, uniform=True, gaps=[(0, 60, 5), (0, 61, 5), (0, 62, 5)]), name='planted')
