"""Planted cases of the SMPL-fit tests and their oracle results (tests/golden/smplfit_cases.npz).  `python tests/_smplfit_cases.py`
regenerates the file on the CPU: targets from planted parameters (body-pose angles within +-0.4 rad at most, non-zero betas,
any omega and t), fitted by tests/_smplfit_oracle.lm from the default start with the priors below.  A candidate is KEPT only
if the oracle converges within MAX_ITERS - MARGIN trials and reaches the same minimum from a second damping start (lambda0 = 1e-2):
largest parameter gap relative to the largest |parameter| below 1e-6, so that no case with two nearby minima is used.
TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

V, REG, SEED = 70, 'dense', 0
POSE_PRIOR, SHAPE_PRIOR = 1000.0, 100.0          # strong enough that the 85 unknowns are well determined by 54 joint rows
MAX_ITERS, CANDIDATES, KEEP_GAP = 30, 32, 1e-6
MARGIN = 4                                        # trials kept in hand: the kernel starts from its own fp32 alignment, a few ulp away
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'smplfit_cases.npz')


def candidates():
    """-> planted x [CANDIDATES,85] float64 of fp32 values; the pose amplitude cycles through 0.1 .. 0.4 rad."""
    import _smplfit_inputs as si
    out = []
    for i in range(CANDIDATES):
        out.append(si.random_params(1, 500 + i, pose_amp=(0.1, 0.2, 0.3, 0.4)[i % 4], beta_amp=1.0)[0])
    return np.stack(out)


def generate():
    import torch
    import _smplfit_inputs as si
    import _smplfit_oracle as so
    m = so.model_arrays(si.arrays(V, REG, SEED))
    w = torch.ones(18, dtype=torch.float64)
    keep = {k: [] for k in ('index', 'planted', 'targets', 'x0', 'x', 'cost', 'iters', 'gap2', 'g0')}
    for i, xp in enumerate(candidates()):
        tgt = so.joints(torch.as_tensor(xp), m).float()
        x0 = so.kabsch_init(m, tgt.double(), w)
        a = so.lm(x0, m, tgt.double(), w, POSE_PRIOR, SHAPE_PRIOR, MAX_ITERS)
        if a['status'] != 0 or a['iters'] > MAX_ITERS - MARGIN:
            print('candidate %d: no convergence within %d trials' % (i, MAX_ITERS - MARGIN))
            continue
        b = so.lm(x0, m, tgt.double(), w, POSE_PRIOR, SHAPE_PRIOR, 4 * MAX_ITERS, lambda0=1e-2)
        gap = float((a['x'] - b['x']).abs().max() / a['x'].abs().max())
        print('candidate %d: %d trials, cost %.3f -> %.6f, second start status %d gap %.2e' % (i, a['iters'], *a['cost'], b['status'], gap))
        if b['status'] != 0 or not gap < KEEP_GAP:
            continue
        r0, J0 = so.linearise(x0, m, tgt.double(), w, POSE_PRIOR, SHAPE_PRIOR)
        for k, v in (('index', i), ('planted', xp), ('targets', tgt.numpy()), ('x0', x0.numpy()), ('x', a['x'].numpy()),
                     ('cost', np.array(a['cost'])), ('iters', a['iters']), ('gap2', gap), ('g0', float((J0.T @ r0).abs().max()))):
            keep[k].append(v)
    print('%d of %d candidates kept' % (len(keep['index']), CANDIDATES))
    np.savez(PATH, **{k: np.asarray(v) for k, v in keep.items()})


def load():
    with np.load(PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    generate()
