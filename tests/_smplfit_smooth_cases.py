"""Seeded cases of the smoothed SMPL track fit's tests on the synthetic bodies of tests/_smplfit_inputs.py: every track has one
planted beta and a pose and translation that vary smoothly over its frame numbers, targets with a little noise, and starts from
the per-frame rigid alignment with small random betas.  The tracks lie INTERLEAVED and shuffled in N.  The track lengths are the
smallest at which the block recurrence can go wrong: 3 (one stencil), 4 (L_i,i-1 first filled by L_i,i-2), 5 (the border filled
from two predecessors), 7 with uneven frame steps, 1 and 2 (no prior).  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np
import torch

import _smplfit_inputs as si
import _smplfit_oracle as so
import _smplfit_smooth_oracle as sm
import _smplfit_tracks_cases as tc

WP, WS = tc.WP, tc.WS
from xas_amd.ops_smplfit import FIT_SMOOTH_ROT as ROT, FIT_SMOOTH_TRANS as TRANS   # the defaults (the planted file was made with 1e4, 1.0)
FIT_ITERS = tc.FIT_ITERS          # the fit cases stop here, before they converge
STEPS = (1, 3, 2)                 # the frame steps of an uneven track, repeated
# name -> (V, track lengths, seed, rot_w, trans_w, options)
CASES = {'mixed_V70': (70, (3, 4, 5, 7, 1, 2), 1, ROT, TRANS, ('extras', 'uneven3')),
         'rot_only_V70': (70, (5, 3), 2, ROT, 0.0, ()),
         'trans_only_V70': (70, (4, 2), 3, 0.0, TRANS, ()),
         'zero_V70': (70, (3, 2), 4, 0.0, 0.0, ()),
         'wrap_V70': (70, (5, 3), 5, ROT, TRANS, ('wrap0',)),
         'two_pass_V513': (513, (4,), 6, ROT, TRANS, ())}
_built, _fits = {}, {}
model = tc.model


def smooth_track(m, frames, seed, noise_mm=5.0, wrap=False, beta=None, amp=1.0):
    """-> x0 [T,85] (fp32-representable), tgt [T,18,3] float32, planted x [T,85], clean joints [T,18,3].  The planted parameters
    are a quadratic in the frame number; wrap: the root angle passes pi on the way."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = len(frames)
    base = si.random_params(1, seed + 7, pose_amp=0.3)[0]
    scale = np.concatenate([np.full(3, 0.04), np.full(3, 15.0), np.full(69, 0.02), np.zeros(10)]) * amp
    vel, acc = scale * rng.standard_normal(85), 0.05 * scale * rng.standard_normal(85)
    tt = (np.asarray(frames, np.float64) - frames[0])[:, None]
    xp = base[None] + vel[None] * tt + 0.5 * acc[None] * tt ** 2
    if beta is not None:
        xp[:, 75:] = beta
    if wrap:
        u = base[:3] / np.linalg.norm(base[:3])
        xp[:, :3] = np.linspace(2.9, 3.4, T)[:, None] * u[None]
    clean = torch.stack([so.joints(torch.as_tensor(x), m) for x in xp])
    tgt = (clean + noise_mm * torch.as_tensor(rng.standard_normal((T, 18, 3)))).float()
    w = torch.ones(18, dtype=torch.float64)
    x0 = torch.stack([so.kabsch_init(m, tgt[t].double(), w) for t in range(T)]).numpy()
    x0[:, 75:] = 0.1 * rng.standard_normal((T, 10))
    return x0.astype(np.float32).astype(np.float64), tgt.numpy(), xp, clean.numpy()


def frames_of(T, uneven):
    f = [10]
    for t in range(T - 1):
        f.append(f[-1] + (STEPS[t % 3] if uneven else 2))
    return f


def build(name):
    """-> dict(V, x0, tgt, w, track, frame, rot_w, trans_w) numpy, the samples shuffled within N.  extras: track 1 gains a frame
    with 5 joints used in its middle (passed through), track 2 a usable frame that repeats a frame number (passed through when a
    weight is positive), a last track has only frames of 5 joints, and joint 3 of every sample has weight 0 and a NaN target."""
    if name in _built:
        return _built[name]
    V, lengths, seed, rot_w, trans_w, opts = CASES[name]
    _, m = model(V)
    x0, tgt, w, track, frame = [], [], [], [], []
    for s, T in enumerate(lengths):
        f = frames_of(T, 'uneven%d' % s in opts)
        a, b, _, _ = smooth_track(m, f, 100 * seed + s, wrap='wrap%d' % s in opts)
        x0.append(a), tgt.append(b), w.append(np.ones((T, 18), np.float32))
        track += [s] * T
        frame += f
    x0, tgt, w = np.concatenate(x0), np.concatenate(tgt), np.concatenate(w)
    if 'extras' in opts:
        S = len(lengths)
        five = np.zeros((4, 18), np.float32)
        five[:, :5] = 1
        five[1] = 1                                                   # the repeated frame is usable by itself
        src = [3, 8, 0, 1]                                            # a frame of track 1, one of track 2, two of track 0
        x0, tgt, w = np.concatenate([x0, x0[src]]), np.concatenate([tgt, tgt[src]]), np.concatenate([w, five])
        track += [1, 2, S, S]
        frame += [13, frame[8], 0, 1]                                 # 13 lies between two frames of track 1
        w[:, 3] = 0
        tgt[w == 0] = np.nan
    rng = np.random.Generator(np.random.PCG64(seed + 50))
    order = rng.permutation(len(track))
    _built[name] = dict(V=V, x0=x0[order], tgt=tgt[order], w=w[order], track=np.asarray(track, np.int64)[order],
                        frame=np.asarray(frame, np.int64)[order], rot_w=rot_w, trans_w=trans_w)
    return _built[name]


def tracks_of_case(c, rot_w=None, trans_w=None):
    """-> [(track id, sample rows in the track's order, sm.SmoothTrack)] in ascending id."""
    _, m = model(c['V'])
    rot_w, trans_w = c['rot_w'] if rot_w is None else rot_w, c['trans_w'] if trans_w is None else trans_w
    out = []
    for s in sorted(set(c['track'].tolist())):
        rows = np.nonzero(c['track'] == s)[0]
        rows = rows[np.argsort(c['frame'][rows], kind='stable')]
        out.append((s, rows, sm.SmoothTrack(torch.as_tensor(c['x0'][rows]), torch.as_tensor(c['tgt'][rows]), torch.as_tensor(c['w'][rows]),
                                            c['frame'][rows], m, WP, WS, rot_w, trans_w)))
    return out


def oracle_fit(name, iters=FIT_ITERS):
    """The oracle's LM of every track of the case (computed once) -> [(track id, rows, SmoothTrack, sm.lm's dict)]."""
    if (name, iters) not in _fits:
        _fits[(name, iters)] = [(s, rows, trk, sm.lm(trk, iters)) for s, rows, trk in tracks_of_case(build(name))]
    return _fits[(name, iters)]


# The planted sequence: one true beta, 12 frames of a pose that varies smoothly in time, Gaussian noise of 10 mm on the joints.
PLANTED = dict(V=70, T=12, seed=41, noise_mm=10.0, iters=30, rot_w=ROT, trans_w=TRANS)
PLANTED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'smplfit_smooth_planted.npz')


def planted_inputs():
    _, m = model(PLANTED['V'])
    frames = list(range(PLANTED['T']))
    x0, tgt, xp, clean = smooth_track(m, frames, PLANTED['seed'], noise_mm=PLANTED['noise_mm'])
    x0[:, 75:] = 0                                                   # the default start: zero betas
    return dict(x0=x0, tgt=tgt, beta=xp[0, 75:], clean=clean, frames=np.asarray(frames))


def accel_mm(joints, frames):
    """Mean over the inner frames and the 18 joints of the norm of the stencil's second difference of joints [T,18,3], mm."""
    J = torch.as_tensor(np.asarray(joints))
    a = [sum(c * J[k + o] for c, o in zip(sm.stencil(frames, k)[:3], (-1, 0, 1))).norm(dim=-1).mean() for k in range(1, len(J) - 1)]
    return float(torch.stack(a).mean())


def planted_figures(joints_smooth, joints_track, p):
    """-> (mean joint distance to the noise-free joints of the smoothed fit, of the unsmoothed track fit, mean joint acceleration of
    the smoothed fit, of the unsmoothed track fit), mm."""
    jd = lambda J: float(np.linalg.norm(np.asarray(J) - p['clean'], axis=-1).mean())
    return jd(joints_smooth), jd(joints_track), accel_mm(joints_smooth, p['frames']), accel_mm(joints_track, p['frames'])


def generate_planted():
    """`python tests/_smplfit_smooth_cases.py`: the oracle's results of the planted sequence -> PLANTED_PATH (CPU)."""
    p = planted_inputs()
    _, m = model(PLANTED['V'])
    T = PLANTED['T']
    mk = lambda rw, tw: sm.SmoothTrack(torch.as_tensor(p['x0']), torch.as_tensor(p['tgt']), torch.ones(T, 18), p['frames'], m, WP, WS, rw, tw)
    r, r0 = sm.lm(mk(PLANTED['rot_w'], PLANTED['trans_w']), PLANTED['iters']), sm.lm(mk(0.0, 0.0), PLANTED['iters'])
    J = lambda X: np.stack([so.joints(v, m).numpy() for v in X])
    X = lambda q: torch.cat([q['y'], q['beta'].expand(T, 10)], 1)
    np.savez(PLANTED_PATH, x=X(r).numpy(), joints=J(X(r)), cost=np.asarray(r['cost']), trials=r['trials'], status=r['status'],
             spread=r['spread'], margin=r['margin'], track_x=X(r0).numpy(), track_joints=J(X(r0)), track_trials=r0['trials'],
             track_spread=r0['spread'], track_margin=r0['margin'])
    z = load_planted()
    print('planted, oracle alone: joints from the noise-free joints %.3f mm (smoothed) vs %.3f mm (track fit); mean joint acceleration '
          '%.3f vs %.3f mm / frame^2' % planted_figures(z['joints'], z['track_joints'], p))


def load_planted():
    with np.load(PLANTED_PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    generate_planted()
