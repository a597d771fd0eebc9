"""Float64 restatement of xas_triangulate_refine (include/xas_hip.h): the specification the GPU tests compare with.

The cost, the views used, the pass-through rules, `resid` and `cov` are the header's, term for term.  The MINIMISER is not the
kernel's: Gauss-Newton damped by a multiple of the identity (the kernel damps by diag(H)), another schedule of the damping
(x4 / x0.25 against x10 / x0.1, from 0 against 1e-3), and it stops on the gradient, not on the step: when |g| falls under 1e-10
of its value at the start.  Where float64 cannot resolve that (a noise-free start has a gradient of rounding size already) it
stops when the step falls under 1e-10 mm, six orders under the tolerance the results are compared with.
`schedule` restates the header's own loop beside it, for the one question `minimise` cannot answer: where that loop stands
after a given number of trials when it has not converged yet (Huber's loss, the default 20 trials).

Every result carries `cond`, the condition number of the Gauss-Newton Hessian at the minimum: the position of a joint is a fair
comparison only where the minimum is well determined (COND_MAX).  That is a condition on the inputs, checked without a GPU.
"""
import numpy as np

import _tri_oracle as to

COND_MAX = 1e3
GRAD_REL = 1e-10
STEP_FLOOR_MM = 1e-10


def views_used(pts, byte):
    """pts [V,3] float32, byte = views[b][k] or 0 -> the list F."""
    valid = [v for v in range(pts.shape[0]) if np.isfinite(pts[v, 2]) and pts[v, 2] > 0]
    return [v for v in valid if byte >> v & 1] if byte else valid


def terms(pts, P, X, F, weighted, huber):
    """-> (C, sum |r|^2, H [3,3], g [3], in front of every view of F) at X [3], everything float64."""
    C, r2, H, g, front = 0.0, 0.0, np.zeros((3, 3)), np.zeros(3), True
    for v in F:
        Pv = P[v].astype(np.float64)
        h = Pv[:, :3] @ X + Pv[:, 3]
        front = front and not h[2] <= 0             # the header's rule: a NaN h2 is not behind
        with np.errstate(all='ignore'):
            proj = h[:2] / h[2]
            r = proj - pts[v, :2].astype(np.float64)
            s = np.float64(pts[v, 2]) if weighted else 1.0
            e = s * np.sqrt(r @ r)
            tail = huber > 0 and e > huber
            C += 2 * huber * e - huber * huber if tail else e * e
            psi = huber / e if tail else 1.0
            J = (Pv[:2, :3] - np.outer(proj, Pv[2, :3])) / h[2]
        r2 += r @ r
        H += psi * s * s * J.T @ J
        g += psi * s * s * J.T @ r
    return C, r2, H, g, front


def minimise(pts, P, X0, F, weighted, huber):
    X = np.array(X0, np.float64)
    C, _, H, g, front = terms(pts, P, X, F, weighted, huber)
    assert front
    g0, mu = np.linalg.norm(g), 0.0
    for _ in range(2000):
        if np.linalg.norm(g) <= GRAD_REL * g0:
            return X
        step = -np.linalg.solve(H + mu * np.trace(H) / 3 * np.eye(3), g)
        if np.linalg.norm(step) < STEP_FLOOR_MM:
            return X
        Ct, _, Ht, gt, ft = terms(pts, P, X + step, F, weighted, huber)
        # next to the minimum the cost changes by less than float64 resolves; there a smaller gradient is the progress
        if ft and (Ct < C or (abs(Ct - C) <= 1e-13 * C and np.linalg.norm(gt) < np.linalg.norm(g))):
            X, C, H, g = X + step, Ct, Ht, gt
            mu = mu / 4 if mu > 1e-12 else 0.0
        else:
            mu = max(4 * mu, 1e-6)
    raise AssertionError('the oracle did not converge')


def _cov6(H):
    with np.errstate(all='ignore'):
        c = np.linalg.inv(H) if np.linalg.matrix_rank(H) == 3 else np.full((3, 3), np.nan)
    return c[np.triu_indices(3)]


def refine_one(pts, P, init, byte, weighted, huber):
    """pts [V,3], P [V,3,4], init [4] (float32), byte -> dict for one joint."""
    F = views_used(pts, byte)
    X0 = init[:3].astype(np.float64)
    nan = dict(F=F, passed=True, xyz=X0, resid=np.full(2, np.nan), cov=np.full(6, np.nan), cov_shift=np.nan, resid_shift=np.nan,
               cond=np.nan, C_init=np.nan, C=np.nan)
    if len(F) < 2 or not np.isfinite(X0).all():
        return nan
    C0, r20, _, _, front = terms(pts, P, X0, F, weighted, huber)
    if not front:
        return nan
    X = minimise(pts, P, X0, F, weighted, huber)
    C, r2, H, _, _ = terms(pts, P, X, F, weighted, huber)
    cov = _cov6(H)
    shift, rshift = 0.0, 0.0                       # how far cov and resid move when the point moves by the position tolerance
    for d in np.concatenate([np.eye(3), -np.eye(3)]) * 1e-4:
        t = terms(pts, P, X + d, F, weighted, huber)
        shift = max(shift, np.abs(_cov6(t[2]) - cov).max())
        rshift = max(rshift, abs(np.sqrt(t[1] / len(F)) - np.sqrt(r2 / len(F))))
    # the tolerance is on the largest coordinate, so all three may move by it at once: sqrt(3) of the largest axis shift covers
    # every direction to first order (where resid is stationary, without weights or Huber, both are ~1e-10 px)
    return dict(F=F, passed=False, xyz=X, resid=np.sqrt(np.array([r20, r2]) / len(F)), cov=cov, cov_shift=shift,
                resid_shift=np.sqrt(3.0) * rshift, cond=np.linalg.cond(H), C_init=C0, C=C)


def _byte(views, b, k):
    return 0 if views is None else int(views[b, k])


def refine(points, P, init, views=None, weighted=False, huber=0.0):
    """points [B,V,K,3], P [B,V,3,4], init [B,K,4] float32, views [B,K] uint8 or None -> dict of arrays [B,K,...]."""
    points, P, init = np.asarray(points, np.float32), np.asarray(P, np.float32), np.asarray(init, np.float32)
    B, V, K, _ = points.shape
    res = [[refine_one(points[b, :, k], P[b], init[b, k], _byte(views, b, k), weighted, huber) for k in range(K)] for b in range(B)]
    g = lambda key, dt: np.array([[r[key] for r in row] for row in res], dtype=dt)
    out = {key: g(key, np.float64) for key in ('xyz', 'resid', 'cov', 'cov_shift', 'resid_shift', 'cond', 'C_init', 'C')}
    out['passed'] = g('passed', bool)
    out['used'] = np.array([[sum(1 << v for v in r['F']) for r in row] for row in res], np.uint8)
    return out


def cost_at(points, P, xyz, views=None, weighted=False, huber=0.0):
    """C at given points xyz [B,K,3] (float32: a kernel's output) in float64 -> (C [B,K], slack [B,K]).  slack = what rounding
    the point to float32 can add to C: with d = half an ulp of each coordinate, |grad C| . d + d^T |Hessian C| d / 2 to second
    order, where grad C = 2 g and Hessian C = 2 H + (the residuals times the projection's second derivative, smaller than 2 H by
    |r| / (f |J|) ~ 1e-3 here); the third order is smaller than the second by |d| / depth ~ 1e-8."""
    points, P = np.asarray(points, np.float32), np.asarray(P, np.float32)
    xyz = np.asarray(xyz, np.float32)
    B, V, K, _ = points.shape
    C, slack = np.full((B, K), np.nan), np.zeros((B, K))
    for b in range(B):
        for k in range(K):
            F = views_used(points[b, :, k], _byte(views, b, k))
            if len(F) >= 2 and np.isfinite(xyz[b, k]).all():
                C[b, k], _, H, g, _ = terms(points[b, :, k], P[b], xyz[b, k].astype(np.float64), F, weighted, huber)
                d = np.spacing(np.abs(xyz[b, k])).astype(np.float64) / 2
                slack[b, k] = 2 * np.abs(g) @ d + d @ np.abs(H) @ d
    return C, slack


def dlt_start(points, P, views=None):
    """The float64 DLT over the views used, rounded to float32, with the mean weight: a stand-in for what xas_triangulate_dlt /
    xas_triangulate_robust write, for building inputs without a GPU.  NaN where fewer than two views are used."""
    points, P = np.asarray(points, np.float32), np.asarray(P, np.float32)
    B, V, K, _ = points.shape
    out = np.full((B, K, 4), np.nan, np.float32)
    for b in range(B):
        for k in range(K):
            F = views_used(points[b, :, k], _byte(views, b, k))
            if len(F) >= 2:
                X = to._solve({v: to._rows(points[b, v, k], P[b, v]) for v in F}, F)
                out[b, k, :3] = X[:3] / X[3]
                out[b, k, 3] = np.mean([points[b, v, k, 2] for v in F])
    return out


def schedule_one(pts, P, init, byte, weighted, huber, max_iter=20):
    """The header's Levenberg-Marquardt schedule itself, restated in float64 for one joint -> (xyz [3], status, trials).  Beside
    `minimise`, which says WHERE the minimum is, this says where the specified loop stands after `max_iter` trials: under Huber's
    loss its convergence is linear, and with few trials that is short of the minimum."""
    F = views_used(pts, byte)
    X = init[:3].astype(np.float64)
    if len(F) < 2 or not np.isfinite(X).all():
        return X, 2, 0
    C, _, H, g, front = terms(pts, P, X, F, weighted, huber)
    if not front:
        return X, 2, 0
    lam, status, n = 1e-3, 1, 0
    for _ in range(max_iter):
        n += 1
        with np.errstate(all='ignore'):
            try:
                d = -np.linalg.solve(H + lam * np.diag(np.diag(H)), g)
            except np.linalg.LinAlgError:
                d = np.full(3, np.nan)
            Ct, _, Ht, gt, ft = terms(pts, P, X + d, F, weighted, huber)
        if ft and Ct < C:
            X, C, H, g = X + d, Ct, Ht, gt
            lam *= 0.1
            if np.linalg.norm(d) < 1e-5:
                status = 0
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return X, status, n


def schedule(points, P, init, views=None, weighted=False, huber=0.0, max_iter=20):
    """-> dict: xyz [B,K,3] float64, status [B,K], trials [B,K]."""
    points, P, init = np.asarray(points, np.float32), np.asarray(P, np.float32), np.asarray(init, np.float32)
    B, V, K, _ = points.shape
    res = [[schedule_one(points[b, :, k], P[b], init[b, k], _byte(views, b, k), weighted, huber, max_iter) for k in range(K)]
           for b in range(B)]
    return dict(xyz=np.array([[r[0] for r in row] for row in res]), status=np.array([[r[1] for r in row] for row in res], np.uint8),
                trials=np.array([[r[2] for r in row] for row in res]))
