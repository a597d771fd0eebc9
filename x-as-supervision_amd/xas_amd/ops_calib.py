"""Bundle adjustment of the camera extrinsics on the device (csrc/calibrate.hip, xas_calibrate_bundle): per rig a correction
(omega, tau) of every free camera and every free point of the rig's samples, by a double-precision Levenberg-Marquardt with the
points eliminated (Schur complement).  include/xas_hip.h states the problem and the schedule.  Imported only when eval.py is
given --calibrate or --calibration.  No reference counterpart."""
import ctypes

import torch

from xas_amd._lib import call, ptr, query
from xas_amd.ops_eval import _scatter, _solver_inputs, _sorted

# Weights of the priors on the corrections, in cost per rad^2 and per mm^2: sigma = 0.01 rad and 10 mm at a 1 px residual.
# UNTUNED GUESSES: there is neither a dataset nor a checkpoint here to tune them on.  With camera 0 fixed they settle the gauge.
CALIB_PRIOR_ROT = 1e4
CALIB_PRIOR_TRANS = 1e-2
CALIB_MAX_RIGS = 16      # xas_hip.h XAS_CALIB_MAX_RIGS
REFINE_WEIGHTED = 1      # xas_hip.h XAS_REFINE_WEIGHTED

STATUS_CONVERGED, STATUS_LIMIT, STATUS_PASSED = 0, 1, 2
STATUS_NAMES = ('converged', 'trial limit', 'passed through')


def rigs_of(pmat):
    """pmat [N,V,3,4] -> (rig [N] int64, keys [R,V,3,4]): samples whose V projection matrices are bit-identical share a rig.
    Nothing but the matrices is looked at.  Raises beyond CALIB_MAX_RIGS rigs."""
    if pmat.dim() != 4 or tuple(pmat.shape[2:]) != (3, 4):
        raise RuntimeError('rigs_of: projection matrices must be [N,V,3,4], got %s' % (tuple(pmat.shape),))
    N, V = pmat.shape[:2]
    bits = pmat.detach().float().contiguous().reshape(N, V * 12).view(torch.int32)
    keys, rig = torch.unique(bits, dim=0, return_inverse=True)
    if keys.shape[0] > CALIB_MAX_RIGS:
        raise RuntimeError('rigs_of: %d different camera rigs in the set (at most %d)' % (keys.shape[0], CALIB_MAX_RIGS))
    return rig.to(torch.int64), keys.contiguous().view(torch.float32).reshape(-1, V, 3, 4)


def default_free(V):
    """Every camera but camera 0."""
    return ((1 << V) - 1) & ~1


def _prepare(name, points, pmat, init, rig, views, num_rigs):
    points, pmat, init, views, N, V, K = _solver_inputs(name, points, pmat, init, views, 'N')
    if rig.shape != (N,):
        raise RuntimeError('%s: rig %s is not one index per sample of points %s' % (name, tuple(rig.shape), tuple(points.shape)))
    rig = rig.to(device=points.device, dtype=torch.int64)
    R = int(num_rigs) if num_rigs is not None else int(rig.max()) + 1
    order = torch.argsort(rig, stable=True)
    counts = torch.bincount(rig, minlength=R).tolist()          # the one host read: rig_start is a host array
    if len(counts) != R or R > CALIB_MAX_RIGS:
        raise RuntimeError('%s: %d rigs (needs rig indices in [0, R), R <= %d)' % (name, len(counts), CALIB_MAX_RIGS))
    start = [0]
    for c in counts:
        start.append(start[-1] + int(c))
    table = (ctypes.c_int * (R + 1))(*start)
    points, pmat, init, views = _sorted(order, points, pmat, init, views)
    ws = torch.empty(max(query('xas_calibrate_workspace_bytes', N, V, K, R), 16), device=points.device, dtype=torch.uint8)
    return points, pmat, init, views, order, table, ws, N, V, K, R


def _delta(delta, R, V, dev):
    if delta is None:
        return torch.zeros(R, V, 6, device=dev, dtype=torch.float64)
    if tuple(delta.shape) != (R, V, 6):
        raise RuntimeError('calibrate: delta %s is not [R,V,6] = (%d, %d, 6)' % (tuple(delta.shape), R, V))
    return delta.detach().to(device=dev, dtype=torch.float64).contiguous().clone()


def calibrate_linearise(points, pmat, init, rig, views=None, free=None, weighted=False, huber_px=0.0, prior_rot=CALIB_PRIOR_ROT,
                        prior_trans=CALIB_PRIOR_TRANS, lam=0.0, delta=None, num_rigs=None):
    """One linearisation at (delta, the points of init) with damping `lam` (xas_calibrate_linearise) -> dict: S [R,n,n], b [R,n]
    (n = 6 * free cameras, slots in ascending camera order, omega before tau) and C [R], float64."""
    points, pmat, init, views, _, table, ws, N, V, K, R = _prepare('calibrate_linearise', points, pmat, init, rig, views, num_rigs)
    free = default_free(V) if free is None else int(free)
    n = 6 * bin(free & ((1 << V) - 1)).count('1')
    dev = points.device
    delta = _delta(delta, R, V, dev)
    out = {'S': torch.empty(R, n, n, device=dev, dtype=torch.float64), 'b': torch.empty(R, n, device=dev, dtype=torch.float64),
           'C': torch.empty(R, device=dev, dtype=torch.float64)}
    call('xas_calibrate_linearise', ptr(points), ptr(pmat), ptr(init), ptr(views), table, N, V, K, R, free,
         REFINE_WEIGHTED if weighted else 0, float(huber_px), float(prior_rot), float(prior_trans), float(lam), ptr(delta),
         ptr(out['S']) if n else None, ptr(out['b']) if n else None, ptr(out['C']), ptr(ws))
    return out


def calibrate_bundle(points, pmat, init, rig, views=None, free=None, weighted=False, huber_px=0.0, prior_rot=CALIB_PRIOR_ROT,
                     prior_trans=CALIB_PRIOR_TRANS, max_iter=30, want=('cost', 'rms', 'status', 'cam_cov', 'trials'), delta=None,
                     num_rigs=None):
    """points [N,V,K,3] (u, v, weight), pmat [N,V,3,4], init [N,K,4] and views [N,K] uint8 (or None) as for
    ops_eval.triangulate_refine, over the whole evaluation set; rig [N] int64 in any order (rigs_of); free = mask of the cameras
    that may move (None = all but camera 0); delta [R,V,6] = the start corrections (None = 0).
    -> dict: delta [R,V,6] float64 (omega rad, tau mm; P T(delta) is the corrected matrix, modules.util.correction_matrix),
    xyzw [N,K,4] in the order given; cost [R,2], rms [R,2] (px, before and after), cam_cov [R,6V,6V] float64, status [R] uint8
    (STATUS_*), trials [R,2] int32 (made, accepted) as requested.  The semantics are those of include/xas_hip.h."""
    points, pmat, init, views, order, table, ws, N, V, K, R = _prepare('calibrate_bundle', points, pmat, init, rig, views, num_rigs)
    free = default_free(V) if free is None else int(free)
    dev = points.device
    f64 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    out = {'delta': _delta(delta, R, V, dev)}
    sorted_out = torch.empty(N, K, 4, device=dev)
    if 'cost' in want:
        out['cost'] = f64(R, 2)
    if 'rms' in want:
        out['rms'] = f64(R, 2)
    if 'cam_cov' in want:
        out['cam_cov'] = f64(R, 6 * V, 6 * V)
    if 'status' in want:
        out['status'] = torch.empty(R, device=dev, dtype=torch.uint8)
    if 'trials' in want:
        out['trials'] = torch.empty(R, 2, device=dev, dtype=torch.int32)
    call('xas_calibrate_bundle', ptr(points), ptr(pmat), ptr(init), ptr(views), table, N, V, K, R, free,
         REFINE_WEIGHTED if weighted else 0, float(huber_px), float(prior_rot), float(prior_trans), int(max_iter), ptr(out['delta']),
         ptr(sorted_out), ptr(out.get('cost')), ptr(out.get('rms')), ptr(out.get('cam_cov')), ptr(out.get('status')),
         ptr(out.get('trials')), ptr(ws))
    out['xyzw'] = _scatter(order, sorted_out)
    return out
