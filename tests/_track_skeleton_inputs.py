"""Synthetic skeleton tracks for the tests of xas_track_skeleton_smooth and for tools/bench_track_skeleton.py: numpy only,
seeded.  The tracks, cameras, detections and anchors are _track_anchor_inputs.build's; this adds `bones` [Bn,2], `length` [S,Bn]
(numpy's restatement of ops_track.track_bone_lengths: the per-track median over the frames where both joints of init are finite)
and `bone_w`.  The joints of those tracks move independently, so their bones are not rigid: that is what the solver cases need,
a bone term that is far from zero.  `planted` builds a skeleton with truly rigid bones instead."""
import numpy as np

import _refine_inputs as ri
import _track_anchor_inputs as ai

BONE_W = 0.1
PARENTS18 = [0, 0, 1, 2, 0, 4, 5, 0, 17, 8, 9, 17, 11, 12, 17, 14, 15, 7]       # model_params.parent_ids of the shipped configs
WRIST, ELBOW = 10, 9


def bones_of(parents):
    return np.asarray([(k, p) for k, p in enumerate(parents) if p >= 0 and p != k], np.int32).reshape(-1, 2)


def chain(K):
    return np.asarray([(k, k - 1) for k in range(1, K)], np.int32).reshape(-1, 2)


def tree(K):
    return np.asarray([(k, (k - 1) // 2) for k in range(1, K)], np.int32).reshape(-1, 2)


def median_lengths(init, track, bones):
    ids = np.unique(track)
    out = np.full((len(ids), len(bones)), np.nan)
    for s, tr in enumerate(ids):
        x = init[track == tr][..., :3].astype(np.float64)
        for b, (i, j) in enumerate(bones):
            ok = np.isfinite(x[:, i]).all(-1) & np.isfinite(x[:, j]).all(-1)
            if ok.any():
                out[s, b] = np.median(np.linalg.norm(x[ok, i] - x[ok, j], axis=-1))
    return out.astype(np.float32)


def build(lengths, K, V, seed, bones, bone_w=BONE_W, no_anchor=False, coincide=(), set_length=(), **kw):
    """_track_anchor_inputs.build plus the bones.  coincide: (track, position, i, j): init of joint j put on joint i's in that
    frame.  set_length: (track, bone, value) after the medians were taken."""
    c = ai.build(lengths, K, V, seed, **kw)
    if no_anchor:
        c['anchor'] = c['info'] = None
    first = np.concatenate([[0], np.cumsum(lengths)])
    for s, t, i, j in coincide:
        c['init'][first[s] + t, j, :3] = c['init'][first[s] + t, i, :3]
    bones = np.asarray(bones, np.int32).reshape(-1, 2)
    length = median_lengths(c['init'], c['track'], bones)
    for s, b, v in set_length:
        length[s, b] = v
    c.update(bones=bones, length=length, bone_w=float(bone_w))
    return c


# Every T at which the frame loop changes shape (no stencil under 3, one at 3, the strides of 64), both ends of K (n = 72 is the
# LDS limit) and V, every rule of the header once.  One camera with a rank-one anchor and no prior has a minimum of cost 0 whose
# trials no oracle can decide (see _track_anchor_inputs): T = 2 and acc_w = 0 take two cameras.  max_iter stops the small cases
# before they converge: the last trials of a converged track change the cost by rounding alone, and those are ties too.
CASES = {
    'T1_K1_nothing_free': dict(lengths=[1], K=1, V=2, seed=71, bones=[], no_anchor=True),
    'T5_K1_no_bones': dict(lengths=[5], K=1, V=2, seed=79, bones=[], no_anchor=True, max_iter=2),                  # n = 3, Bn = 0, the joint free
    'T2_K2': dict(lengths=[2], K=2, V=2, seed=72, bones=chain(2), kind='full', max_iter=2),
    'T3_K3_chain': dict(lengths=[3], K=3, V=2, seed=73, bones=chain(3), no_anchor=True, max_iter=6),
    'T5_K24': dict(lengths=[5], K=24, V=4, seed=74, bones=tree(24), no_anchor=True, weighted=True, huber=1.5),
    # one camera, ray anchors, the config's bones; joint 9 has one usable frame: it is fixed, NaN in init, and its bones switch
    # off; joint 10 has gap frames in the middle and at both ends beside neighbours with data; a NaN and a zero length
    'T65_K18_V1': dict(lengths=[65], K=18, V=1, seed=75, bones=bones_of(PARENTS18), anchor_huber=3.0,
                       anchor_nan=[(0, t, 9) for t in range(65) if t != 7] + [(0, t, 10) for t in (0, 1, 30, 31, 32, 64)],
                       set_length=[(0, 2, np.nan), (0, 4, 0.0)]),
    # coordinates of 1e4 mm, both Hubers, two joints on one point at the start
    'T130_K3_1e4': dict(lengths=[130], K=3, V=2, seed=76, bones=chain(3), kind='full', huber=2.5, anchor_huber=1.0, shift=1e4,
                        coincide=[(0, 40, 0, 1)], gaps=[(0, 90, 2)], anchor_nan=[(0, 90, 2)]),
    'several_V4': dict(lengths=[1, 2, 130], K=3, V=4, seed=77, bones=chain(3), no_anchor=True, views=True, max_iter=3,
                       gaps=[(2, 0, 0), (2, 1, 0), (2, 64, 1), (2, 65, 1), (2, 129, 2)]),
    'bone_w_0': dict(lengths=[6, 3], K=3, V=2, seed=78, bones=chain(3), no_anchor=True, bone_w=0.0, max_iter=2),
}


def make(name):
    return dict(build(**CASES[name]), name=name)


def rigid_world(frames, parents, rng):
    """World tracks [T,K,3] of a skeleton with constant bone lengths (150-450 mm): the root on a smooth path, every bone's
    direction a smoothly turning unit vector.  -> world and the lengths [Bn] of bones_of(parents)."""
    t = np.asarray(frames, np.float64)[:, None]
    K = len(parents)
    wave = lambda amp: amp * np.sin(2 * np.pi * t / rng.uniform(40, 120, 3) + rng.uniform(0, 2 * np.pi, 3))
    world, done = np.zeros((len(t), K, 3)), {}
    length = {}

    def place(k):
        if k in done:
            return
        p = parents[k]
        if p == k or p < 0:
            world[:, k] = rng.normal(0.0, 200.0, 3) + wave(rng.uniform(100, 300, 3))
        else:
            place(p)
            d = rng.normal(size=3) + wave(0.6)
            length[k] = rng.uniform(150.0, 450.0)
            world[:, k] = world[:, p] + length[k] * d / np.linalg.norm(d, axis=-1, keepdims=True)
        done[k] = True
    for k in range(K):
        place(k)
    return world.astype(np.float32), np.asarray([length[k] for k, _ in bones_of(parents)])


def planted(seed=81):
    """The effect case: one 130-frame track, V = 4, K = 18, truly rigid bones, 2 px of noise, the wrist (joint 10) without any
    detection for three frames.  The start is the float64 DLT, as in _track_inputs."""
    from _refine_oracle import dlt_start
    T, K, V = 130, 18, 4
    rng = np.random.Generator(np.random.PCG64(seed))
    frame = np.arange(1, T + 1, dtype=np.int64)
    world, true_len = rigid_world(frame, PARENTS18, rng)
    _, Ps, _ = ri.ring_rig(1, V, K, seed * 1000)
    P = np.repeat(Ps, T, 0)
    pts, _, _ = ri.noisy((ri.project(P, world), P, world), seed * 1000 + 500, 2.0)
    gap = [60, 61, 62]
    pts[gap, :, WRIST, 2] = 0.0
    init = dlt_start(pts, P, None)
    bones = bones_of(PARENTS18)
    track = np.zeros(T, np.int64)
    return dict(points=pts, P=P, init=init, views=None, track=track, frame=frame, truth=world, weighted=False, huber=0.0, acc_w=0.05,
                max_iter=3, N=T, V=V, K=K, S=1, lengths=[T], anchor=None, info=None, anchor_huber=0.0, bones=bones,
                length=median_lengths(init, track, bones), bone_w=BONE_W, true_length=true_len, gap=gap, name='planted')


def monocular(seed=61):
    """_track_anchor_inputs.planted (one camera, K = 18, a tenth of the frames of every third joint on a decoy down the ray) with
    the config's bones."""
    c = ai.planted(seed)
    bones = bones_of(PARENTS18)
    return dict(c, bones=bones, length=median_lengths(c['init'], c['track'], bones), bone_w=BONE_W, name='monocular')
