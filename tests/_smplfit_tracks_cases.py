"""Seeded cases of the track-level SMPL-fit tests on the synthetic bodies of tests/_smplfit_inputs.py: every track has one planted
beta, a planted pose per frame, targets with a little noise, and starts from the rigid alignment with small random betas (so the
starting mean is not trivial).  The tracks lie INTERLEAVED in N.  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np
import torch

import _smplfit_inputs as si
import _smplfit_oracle as so
import _smplfit_tracks_oracle as to

WP, WS = 1000.0, 100.0            # the priors of tests/_smplfit_cases.py
FIT_ITERS = 4                     # the full-fit cases stop here, before they converge
# name -> (V, track lengths, seed)
CASES = {'mixed_V70': (70, (3, 7, 2), 1), 'singles_V70': (70, (1, 1, 1), 2), 'tail_V300': (300, (2, 1), 3), 'two_pass_V513': (513, (1, 2), 4)}
_models, _built, _fits = {}, {}, {}


def model(V, reg='dense'):
    if (V, reg) not in _models:
        a = si.arrays(V, reg)
        _models[(V, reg)] = (a, so.model_arrays(a))
    return _models[(V, reg)]


def planted_track(m, T, seed, noise_mm=5.0, pose_amp=0.3, beta=None):
    """-> x0 [T,85], tgt [T,18,3] float32, planted x [T,85], clean joints [T,18,3]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    xp = si.random_params(T, seed + 7, pose_amp=pose_amp)
    xp[:, 75:] = xp[0, 75:] if beta is None else beta
    clean = torch.stack([so.joints(torch.as_tensor(x), m) for x in xp])
    tgt = (clean + noise_mm * torch.as_tensor(rng.standard_normal((T, 18, 3)))).float()
    w = torch.ones(18, dtype=torch.float64)
    x0 = torch.stack([so.kabsch_init(m, tgt[t].double(), w) for t in range(T)])
    x0[:, 75:] = torch.as_tensor((0.1 * rng.standard_normal((T, 10))).astype(np.float32)).double()
    return x0.numpy(), tgt.numpy(), xp, clean.numpy()


def build(name, extras=False):
    """-> dict(V, x0 [N,85], tgt [N,18,3], w [N,18], track [N], frame [N]) numpy, the samples shuffled within N.
    extras (the linearise test): track 0 gains a frame with 5 joints used (passed through), a last track has only such
    frames, and joint 3 of every sample has weight 0 and a NaN target."""
    key = (name, extras)
    if key in _built:
        return _built[key]
    V, lengths, seed = CASES[name]
    _, m = model(V)
    x0, tgt, w, track, frame = [], [], [], [], []
    for s, T in enumerate(lengths):
        a, b, _, _ = planted_track(m, T, 100 * seed + s)
        x0.append(a), tgt.append(b), w.append(np.ones((T, 18), np.float32))
        track += [s] * T
        frame += [10 + 3 * t for t in range(T)]                      # gaps in the frame numbers: only their order counts
    x0, tgt, w = np.concatenate(x0), np.concatenate(tgt), np.concatenate(w)
    if extras:
        five = np.zeros((3, 18), np.float32)
        five[:, :5] = 1
        x0, tgt, w = np.concatenate([x0, x0[:3]]), np.concatenate([tgt, tgt[:3]]), np.concatenate([w, five])
        track += [0, len(lengths), len(lengths)]
        frame += [11, 0, 1]                                           # the first lies between two frames of track 0
        w[:, 3] = 0
        tgt[w == 0] = np.nan
    rng = np.random.Generator(np.random.PCG64(seed + 50))
    order = rng.permutation(len(track))
    _built[key] = dict(V=V, x0=x0[order], tgt=tgt[order], w=w[order], track=np.asarray(track, np.int64)[order],
                       frame=np.asarray(frame, np.int64)[order])
    return _built[key]


def tracks_of_case(c):
    """-> [(track id, sample rows in ascending frame order, to.Track)] in ascending id."""
    _, m = model(c['V'])
    out = []
    for s in sorted(set(c['track'].tolist())):
        rows = np.nonzero(c['track'] == s)[0]
        rows = rows[np.argsort(c['frame'][rows], kind='stable')]
        out.append((s, rows, to.Track(torch.as_tensor(c['x0'][rows]), torch.as_tensor(c['tgt'][rows]), torch.as_tensor(c['w'][rows]), m, WP, WS)))
    return out


def oracle_fit(name, iters=FIT_ITERS):
    """The oracle's LM of every track of the case (computed once) -> [(track id, rows, Track, to.lm's dict)]."""
    if (name, iters) not in _fits:
        _fits[(name, iters)] = [(s, rows, trk, to.lm(trk, iters)) for s, rows, trk in tracks_of_case(build(name))]
    return _fits[(name, iters)]


# The planted sequence: one true beta, 12 frames of different poses, Gaussian noise of 10 mm on the joints.
PLANTED = dict(V=70, T=12, seed=31, noise_mm=10.0, iters=30)
_planted = {}


def planted():
    """-> dict(x0, tgt, beta [10], clean [T,18,3], track = the oracle's track fit, frames = its per-frame fits)."""
    if not _planted:
        _, m = model(PLANTED['V'])
        x0, tgt, xp, clean = planted_track(m, PLANTED['T'], PLANTED['seed'], noise_mm=PLANTED['noise_mm'])
        x0[:, 75:] = 0                                               # the default start: zero betas
        trk = to.Track(torch.as_tensor(x0), torch.as_tensor(tgt), torch.ones(PLANTED['T'], 18), m, WP, WS)
        w = torch.ones(18, dtype=torch.float64)
        frames = [so.lm(torch.as_tensor(x0[t]), m, torch.as_tensor(tgt[t]).double(), w, WP, WS, PLANTED['iters']) for t in range(PLANTED['T'])]
        _planted.update(x0=x0, tgt=tgt, beta=xp[0, 75:], clean=clean, trk=trk, track=to.lm(trk, PLANTED['iters']), frames=frames)
    return _planted


PLANTED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'smplfit_tracks_planted.npz')


def generate_planted():
    """`python tests/_smplfit_tracks_cases.py`: the oracle's results of the planted sequence -> PLANTED_PATH (CPU, ~15 s)."""
    p = planted()
    _, m = model(PLANTED['V'])
    r = p['track']
    x = torch.cat([r['y'], r['beta'].expand(PLANTED['T'], 10)], 1)
    xf = torch.stack([f['x'] for f in p['frames']])
    J = lambda X: np.stack([so.joints(v, m).numpy() for v in X])
    np.savez(PLANTED_PATH, x=x.numpy(), joints=J(x), cost=np.asarray(r['cost']), trials=r['trials'], status=r['status'], spread=r['spread'],
             margin=r['margin'], frames_x=xf.numpy(), frames_joints=J(xf), frames_iters=np.asarray([f['iters'] for f in p['frames']]),
             frames_status=np.asarray([f['status'] for f in p['frames']]))
    z = load_planted()
    print('planted, oracle alone: |beta - truth| %.4f (track) vs %.4f (mean of the per-frame fits); joints from the noise-free joints '
          '%.3f mm (track) vs %.3f mm (per frame)' % planted_figures(z['x'][0, 75:], z['joints'], z['frames_x'][:, 75:], z['frames_joints'], p))


def load_planted():
    with np.load(PLANTED_PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def planted_inputs():
    """The inputs of the planted sequence alone (cheap: no fit)."""
    _, m = model(PLANTED['V'])
    x0, tgt, xp, clean = planted_track(m, PLANTED['T'], PLANTED['seed'], noise_mm=PLANTED['noise_mm'])
    x0[:, 75:] = 0
    return dict(x0=x0, tgt=tgt, beta=xp[0, 75:], clean=clean)


def planted_figures(beta_track, joints_track, betas_frames, joints_frames, p):
    """-> (|beta_track - truth|, mean |beta_frame - truth|, mean joint distance to the clean joints of the track fit, of the
    per-frame fits), mm for the joints."""
    b = np.asarray(p['beta'])
    jd = lambda J: float(np.linalg.norm(np.asarray(J) - p['clean'], axis=-1).mean())
    return (float(np.linalg.norm(np.asarray(beta_track) - b)), float(np.linalg.norm(np.asarray(betas_frames) - b, axis=1).mean()),
            jd(joints_track), jd(joints_frames))


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    generate_planted()
