"""Seeded cases of the tests of xas_smpl_fit_views on the synthetic bodies of tests/_smplfit_inputs.py: a planted body per
sample, cameras on a ring round it (f = 1150 px at about 4 m: roughly 0.3 px per mm), detections = the projected planted joints
plus 2 px of noise with weights in [0.5, 2], a start a little off the planted parameters.  Each case switches on the edges its
name says; CASES lists them.  numpy and the CPU oracles only.  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np
import torch

import _smplfit_inputs as si
import _smplfit_oracle as so
import _smplfit_views_oracle as vo
import _track_anchor_inputs as tai

WP, WS = 10.0, 2.5                # ops_smplfit.VIEWS_POSE_PRIOR, VIEWS_SHAPE_PRIOR
FIT_ITERS = 4                     # the fit cases stop here, before they converge
DEPTH_W = tai.DEPTH_W
TRI = tai.TRI
_models, _built, _samples = {}, {}, {}


def model(V, reg='dense'):
    if (V, reg) not in _models:
        a = si.arrays(V, reg)
        _models[(V, reg)] = (a, so.model_arrays(a))
    return _models[(V, reg)]


def look_at(centre, target, f=1150.0, c=(500.0, 500.0)):
    """-> P [3,4] float64 of a camera at `centre` that looks at `target` (y up)."""
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    K = np.array([[f, 0.0, c[0]], [0.0, f, c[1]], [0.0, 0.0, 1.0]])
    return K @ np.concatenate([R, -(R @ centre)[:, None]], 1)


def project(P, Y):
    """P [C,3,4], Y [18,3] float64 -> pixels [C,18,2]."""
    h = np.einsum('cij,kj->cki', P[:, :, :3], Y) + P[:, None, :, 3]
    return h[..., :2] / h[..., 2:]


def sample(m, C, seed, center=0, shift=0.0, close_up=False):
    """One planted sample -> dict(x0 [85], points [C,18,3], P [C,3,4] float32, clean [18,3], behind = (view, joint) or None)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    xp = si.random_params(1, seed + 7, pose_amp=0.3)[0]
    xp[3:6] += shift
    xp = xp.astype(np.float32).astype(np.float64)
    cen = None if center < 0 else center
    Y = so.joints(torch.as_tensor(xp), m, center_idx=cen).numpy()
    mid = Y.mean(0)
    P = np.stack([look_at(mid + 4000.0 * np.array([np.sin(a), 0.15 * (i % 3 - 1), -np.cos(a)]), mid)
                  for i, a in enumerate(2 * np.pi * (np.arange(C) / C) + rng.uniform(0, 0.3))])
    x0 = xp.copy()
    x0[:3] += 0.05 * rng.standard_normal(3)
    x0[3:6] += 20.0 * rng.standard_normal(3)
    x0[6:75] *= 0.8
    x0[75:] *= 0.5
    x0 = x0.astype(np.float32).astype(np.float64)
    Y0 = so.joints(torch.as_tensor(x0), m, center_idx=cen).numpy()
    behind = None
    w = rng.uniform(0.5, 2.0, (C, 18))
    if close_up:                                                      # the last view: a camera between the first joint along its axis and the rest
        d = np.array([0.0, 0.0, 1.0])
        order = np.argsort(Y0 @ d)
        k0, gap = int(order[0]), float((Y0 @ d)[order[1]] - (Y0 @ d)[order[0]])
        centre = Y0[k0] + d * gap / 2 + np.array([300.0, 0.0, 0.0])   # off the axis: no joint sits on the optical centre
        P[C - 1] = look_at(centre, centre + d * 1000.0)
        far = [int(k) for k in order[-3:]]
        w[C - 1] = 0.0                                                # the close-up sees the joint behind it and the three farthest
        w[C - 1, [k0] + far] = 1.0
        behind = (C - 1, k0)
    P = P.astype(np.float32)
    uv = project(P.astype(np.float64), Y) + 2.0 * rng.standard_normal((C, 18, 2))
    points = np.concatenate([uv, w[..., None]], -1).astype(np.float32)
    return dict(x0=x0, points=points, P=P, clean=Y, behind=behind, planted=xp)


def ray_anchor(s, rng, depth_mm=30.0, decoys=()):
    """Anchors on the rays of camera 0 through the planted joints, off by depth noise (a decoy: 400 mm down the ray), with the
    rank-one information of ops_track.ray_information (numpy's restatement, _track_anchor_inputs.ray_info)."""
    centre = tai.centres(s['P'][None])[0, 0]
    r = s['clean'] - centre
    r = r / np.linalg.norm(r, axis=-1, keepdims=True)
    anchor = s['clean'] + r * rng.normal(0.0, depth_mm, (18, 1))
    for k in decoys:
        anchor[k] += 400.0 * r[k]
    anchor = anchor.astype(np.float32)
    return anchor, tai.ray_info(s['P'][None, 0], anchor[None], DEPTH_W)[0]


def full_anchor(s, rng):
    """The planted joints plus noise of a random covariance (axes of 5 to 30 mm) with its inverse as the information."""
    Q = np.linalg.qr(rng.normal(size=(18, 3, 3)))[0]
    sd = rng.uniform(5.0, 30.0, (18, 3))
    anchor = s['clean'] + np.einsum('kij,kj->ki', Q, sd * rng.normal(size=(18, 3)))
    W = np.einsum('kij,kj,klj->kil', Q, 1.0 / sd ** 2, Q)
    return anchor.astype(np.float32), W[..., TRI[0], TRI[1]].astype(np.float32)


def _stack(samples, **kw):
    c = {k: np.stack([s[k] for s in samples]) for k in ('x0', 'points', 'P', 'clean')}
    c.update(views=None, anchor=None, info=None, weighted=False, huber=0.0, anchor_huber=0.0, center=0, reg='dense', behind=[s['behind'] for s in samples])
    c.update(kw)
    return c


def _one_camera(seed):
    """C = 1, ray anchors (rank one) under Huber with two decoys on the tail; sample 1: NaN anchors, a zero-trace info, and a
    joint with neither view nor anchor whose pixels, anchor and info are NaN."""
    _, m = model(70)
    rng = np.random.Generator(np.random.PCG64(seed))
    ss = [sample(m, 1, seed + i) for i in range(3)]
    an = [ray_anchor(s, rng, decoys=(4, 11)) for s in ss]
    anchor, info = np.stack([a for a, _ in an]), np.stack([i for _, i in an])
    anchor[1, 2, 1] = np.nan                                          # joint 2: pixels alone
    info[1, 5] = 0.0                                                  # joint 5: a zero trace, pixels alone
    c = _stack(ss, V=70, anchor=anchor, info=info, anchor_huber=tai.ANCHOR_HUBER)
    c['points'][1, 0, 7] = (np.nan, np.nan, 0.0)                      # joint 7: NaN pixels under weight 0 and a NaN anchor: not used
    c['anchor'][1, 7], c['info'][1, 7] = np.nan, np.nan
    c['points'][2, 0, 9, 2] = 0.0                                     # joint 9 of sample 2: the anchor alone
    return c


def _two_cameras(seed):
    """C = 2, weighted, Huber with outliers on the tail, `views` bytes that exclude a valid view and zero bytes, center_idx -1."""
    _, m = model(70)
    rng = np.random.Generator(np.random.PCG64(seed))
    ss = [sample(m, 2, seed + i, center=-1) for i in range(2)]
    c = _stack(ss, V=70, weighted=True, huber=3.0, center=-1)
    for b, v, k in ((0, 0, 3), (0, 1, 12), (1, 1, 6)):
        c['points'][b, v, k, :2] += (40.0, -25.0)
    views = np.full((2, 18), 3, np.uint8)
    views[0, 1], views[0, 8], views[1, 4] = 1, 2, 2                   # a valid view left out
    views[0, 10], views[1, 0] = 0, 0                                  # zero: all valid views
    views[1, 13] = 4                                                  # a view that does not exist: none left, the joint is not used
    c['views'] = views
    return c


def _four_cameras(seed):
    """C = 4, V = 513 (two vertex passes and one vertex), the compacted regressor list ('nine'), full-rank anchors without Huber."""
    _, m = model(513, 'nine')
    rng = np.random.Generator(np.random.PCG64(seed))
    ss = [sample(m, 4, seed + i) for i in range(2)]
    an = [full_anchor(s, rng) for s in ss]
    c = _stack(ss, V=513, reg='nine', weighted=True, anchor=np.stack([a for a, _ in an]), info=np.stack([i for _, i in an]))
    c['anchor'][0, 3] = np.nan
    c['points'][1, 2, :, 2] = np.inf                                  # a view of invalid weights
    return c


def _six_cameras(seed):
    """C = 6, Huber, not weighted; sample 0 has a close-up view with one joint behind it at the start (dropped for that joint);
    sample 1 stands at coordinates of 1e4 mm."""
    _, m = model(70)
    ss = [sample(m, 6, seed, close_up=True), sample(m, 6, seed + 1, shift=1e4)]
    c = _stack(ss, V=70, huber=3.0)
    c['points'][1, 4, 2, :2] += (-30.0, 30.0)
    return c


def _passed(seed):
    """C = 2: sample 0 has 5 joints used (the rest: weight 0 and NaN pixels), sample 1 a start that is not finite, sample 2 is
    fitted."""
    _, m = model(70)
    ss = [sample(m, 2, seed + i) for i in range(3)]
    c = _stack(ss, V=70)
    c['points'][0, :, 5:] = (np.nan, np.nan, 0.0)
    c['x0'][1, 4] = np.nan
    return c


CASES = {'one_camera_ray_V70': (_one_camera, 11), 'two_cameras_huber_V70': (_two_cameras, 21), 'four_cameras_full_V513': (_four_cameras, 31),
         'six_cameras_behind_V70': (_six_cameras, 41), 'passed_V70': (_passed, 51)}


def build(name):
    if name not in _built:
        fn, seed = CASES[name]
        _built[name] = fn(seed)
    return _built[name]


def oracle_samples(name):
    """-> [vo.Sample] of the case."""
    if name not in _samples:
        c = build(name)
        _, m = model(c['V'], c['reg'])
        _samples[name] = [vo.Sample(m, c['x0'][b], c['points'][b], c['P'][b], None if c['views'] is None else c['views'][b],
                                    None if c['anchor'] is None else c['anchor'][b], None if c['info'] is None else c['info'][b],
                                    c['weighted'], c['huber'], c['anchor_huber'], WP, WS, c['center']) for b in range(len(c['x0']))]
    return _samples[name]


# The planted monocular sequence: 12 samples, one camera, 2 px of pixel noise, 30 mm of depth noise, a tenth of the joints on a
# decoy 250 to 600 mm down the ray.  The single-view world points (the noisy pixel's ray at the noisy depth) are the joint fit's
# targets and the pixel fit's anchors; the joint fit (default priors, from the rigid start) is the pixel fit's warm start, rounded
# to fp32 as the device receives it.  Default weights everywhere, 30 trials.
PLANTED = dict(V=70, N=12, seed=71, pixel_px=2.0, depth_mm=30.0, decoy_share=0.1, decoy_mm=(250.0, 600.0), iters=30,
               joints_priors=(100.0, 25.0), views_priors=(WP, WS), depth_w=DEPTH_W, anchor_huber=tai.ANCHOR_HUBER)
PLANTED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'smplfit_views_planted.npz')


def planted_inputs():
    """-> dict(x0 [N,85] the rigid start, points [N,1,18,3], P [N,1,3,4], anchor [N,18,3], info [N,18,6], clean [N,18,3], decoy [N,18])."""
    p = PLANTED
    _, m = model(p['V'])
    rng = np.random.Generator(np.random.PCG64(p['seed']))
    ss = [sample(m, 1, p['seed'] + 1 + i) for i in range(p['N'])]
    clean, P = np.stack([s['clean'] for s in ss]), np.stack([s['P'] for s in ss])
    uv = np.stack([project(s['P'].astype(np.float64), s['clean']) for s in ss]) + p['pixel_px'] * rng.standard_normal((p['N'], 1, 18, 2))
    points = np.concatenate([uv, np.ones((p['N'], 1, 18, 1))], -1).astype(np.float32)
    decoy = np.zeros(p['N'] * 18, bool)
    decoy[rng.choice(p['N'] * 18, size=int(round(p['decoy_share'] * p['N'] * 18)), replace=False)] = True
    decoy = decoy.reshape(p['N'], 18)
    anchor = np.zeros((p['N'], 18, 3))
    for b in range(p['N']):
        Pd = P[b, 0].astype(np.float64)
        centre = tai.centres(P[b][None])[0, 0]
        ray = np.linalg.solve(Pd[:, :3], np.concatenate([points[b, 0, :, :2].astype(np.float64), np.ones((18, 1))], 1).T).T   # through the noisy pixel
        ray = ray / np.linalg.norm(ray, axis=1, keepdims=True)
        ray = ray * np.sign(((clean[b] - centre) * ray).sum(1, keepdims=True))
        depth = ((clean[b] - centre) * ray).sum(1) + p['depth_mm'] * rng.standard_normal(18)
        depth = depth + np.where(decoy[b], rng.uniform(*p['decoy_mm'], 18), 0.0)
        anchor[b] = centre + ray * depth[:, None]
    anchor = anchor.astype(np.float32)
    info = tai.ray_info(P[:, 0], anchor, p['depth_w'])
    w = torch.ones(18, dtype=torch.float64)
    x0 = np.stack([so.kabsch_init(m, torch.as_tensor(anchor[b]).double(), w).numpy() for b in range(p['N'])])
    return dict(x0=x0, points=points, P=P, anchor=anchor, info=info, clean=clean, decoy=decoy)


def planted_figures(joints_fit, views_fit, clean):
    """-> the mean distance (mm) of the fitted joints [N,18,3] to the noise-free joints: of the joint fit, of the pixel fit."""
    d = lambda J: float(np.linalg.norm(np.asarray(J) - clean, axis=-1).mean())
    return d(joints_fit), d(views_fit)


def generate_planted():
    """`python tests/_smplfit_views_cases.py`: the oracle's two fits of the planted sequence -> PLANTED_PATH (CPU, a few minutes)."""
    p, q = PLANTED, planted_inputs()
    _, m = model(p['V'])
    w = torch.ones(18, dtype=torch.float64)
    out = {k: [] for k in ('joints_x', 'joints_joints', 'joints_iters', 'joints_status', 'warm', 'views_x', 'views_joints', 'views_iters',
                           'views_status', 'views_cost', 'spread', 'margin', 'used', 'joints_spread', 'joints_margin')}
    for b in range(p['N']):
        a = so.lm(torch.as_tensor(q['x0'][b]), m, torch.as_tensor(q['anchor'][b]).double(), w, *p['joints_priors'], p['iters'])
        warm = a['x'].float().double()
        # the joint fit a second time, as the pixel oracle's problem where the two coincide (no view, anchors = targets, info = I, no
        # Huber): its two assemblies' step spread and the distance of the two oracles' results are the joint fit's own spread
        twin = vo.Sample(m, q['x0'][b], np.zeros((1, 18, 3), np.float32), q['P'][b], None, q['anchor'][b],
                         np.tile(np.float32([1, 0, 0, 1, 0, 1]), (18, 1)), False, 0.0, 0.0, *p['joints_priors'], 0).lm(p['iters'])
        assert twin['iters'] == a['iters'] and twin['status'] == a['status']
        out['joints_spread'].append(max(twin['spread'], vo.rel(twin['x'], a['x'])))
        out['joints_margin'].append(twin['margin'])
        s = vo.Sample(m, warm.numpy(), q['points'][b], q['P'][b], None, q['anchor'][b], q['info'][b], False, 0.0, p['anchor_huber'],
                      *p['views_priors'], 0)
        r = s.lm(p['iters'])
        print('planted sample %d: joint fit %d trials status %d (spread %.2e, margin %.2e); pixel fit %d trials status %d, cost %.3f -> %.3f, spread %.2e, margin %.2e'
              % (b, a['iters'], a['status'], out['joints_spread'][-1], out['joints_margin'][-1], r['iters'], r['status'], *r['cost'], r['spread'], r['margin']), flush=True)
        for k, v in (('joints_x', a['x'].numpy()), ('joints_joints', so.joints(a['x'], m).numpy()), ('joints_iters', a['iters']),
                     ('joints_status', a['status']), ('warm', warm.numpy()), ('views_x', r['x'].numpy()),
                     ('views_joints', s.joints(r['x']).detach().numpy()), ('views_iters', r['iters']), ('views_status', r['status']),
                     ('views_cost', np.asarray(r['cost'])), ('spread', r['spread']), ('margin', r['margin']), ('used', s.used)):
            out[k].append(v)
    out = {k: np.asarray(v) for k, v in out.items()}
    fig = planted_figures(out['joints_joints'], out['views_joints'], q['clean'])
    np.savez(PLANTED_PATH, figures=np.asarray(fig), **{k: q[k] for k in ('x0', 'points', 'P', 'anchor', 'info', 'clean', 'decoy')}, **out)
    print('planted, oracle alone: mean distance to the noise-free joints %.3f mm (joint fit on the single-view points) vs %.3f mm (pixel '
          'fit with ray anchors)' % fig)


def load_planted():
    with np.load(PLANTED_PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    generate_planted()
