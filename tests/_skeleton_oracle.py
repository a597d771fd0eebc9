"""Float64 restatement of xas_triangulate_skeleton (include/xas_hip.h): the specification the GPU tests compare with.

The cost, the views used, the free / fixed and active rules, `resid`, `sym` and `cost` are the header's, term for term (the
reprojection part is checked against _refine_oracle.terms in tests/test_tri_skeleton_abi.py).  The MINIMISER is not the kernel's,
as in _refine_oracle: Gauss-Newton damped by a multiple of the identity (the kernel damps by diag(H)), another schedule of the
damping (x4 / x0.25 against x10 / x0.1, from 0 against 1e-3), a dense solve (the kernel: Cholesky over an envelope), and it stops
on the gradient, not on the step: when |g| falls under 1e-10 of its value at the start, or, where float64 cannot resolve that,
when the step falls under 1e-10 mm.
`schedule` restates the header's own loop beside it.  It answers what `minimise` cannot: where that loop stands after a given
number of trials, and how fast it converges (`rate`), which is what the kernel's stop rule leaves undone.

Every sample carries `cond`, the condition number of the full free Gauss-Newton matrix at the minimum (COND_MAX as in
_refine_oracle), and `floor`, the distance from the minimum under which float64 no longer resolves a decrease of the cost.
"""
import numpy as np

import _refine_oracle as ro

COND_MAX = ro.COND_MAX
GRAD_REL = 1e-10
STEP_FLOOR_MM = 1e-10
FLAT_MM = 1e-9
EPS = np.finfo(np.float64).eps


class Sample:
    """One sample's problem: what is used, free and active, fixed by the inputs before any iteration."""

    def __init__(self, pts, P, init, views, limbs, weighted, huber, sym_w):
        V, K, _ = pts.shape
        self.V, self.K, self.weighted, self.huber, self.sym_w = V, K, weighted, float(huber), float(sym_w)
        self.uv = pts[..., :2].astype(np.float64).transpose(1, 0, 2)                        # [K,V,2]
        self.s = pts[..., 2].astype(np.float64).T if weighted else np.ones((K, V))          # [K,V]
        self.P = P.astype(np.float64)
        self.F = np.zeros((K, V), bool)
        for k in range(K):
            self.F[k, ro.views_used(pts[:, k], 0 if views is None else int(views[k]))] = True
        self.X0 = init[:, :3].astype(np.float64)
        self.limbs = np.asarray(limbs, np.int64).reshape(-1, 4)
        cand = (self.F.sum(1) >= 2) & np.isfinite(self.X0).all(1)
        self.free = cand.copy()
        self.free = cand & self.reproj(np.where(cand[:, None], self.X0, 0.0), cand)[4]
        self.active = self.free[self.limbs].all(1) if len(self.limbs) else np.zeros(0, bool)
        self.idx = np.flatnonzero(self.free)
        self.slot = -np.ones(K, np.int64)
        self.slot[self.idx] = np.arange(len(self.idx))
        self.n = 3 * len(self.idx)

    def reproj(self, X, joints=None):
        """-> (C [K], sum |r|^2 [K], H [K,3,3], g [K,3], in front of every view used [K], J^T J unweighted [K,3,3]) at X [K,3];
        zeros for joints outside `joints` (default: the free ones)."""
        M = self.F & (self.free if joints is None else joints)[:, None]
        with np.errstate(all='ignore'):
            h = np.einsum('vij,kj->kvi', self.P[:, :, :3], X) + self.P[None, :, :, 3]
            proj = h[..., :2] / h[..., 2:]
            r = proj - self.uv
            rr = (r * r).sum(-1)
            e = self.s * np.sqrt(rr)
            tail = (self.huber > 0) & (e > self.huber)
            rho = np.where(tail, 2 * self.huber * e - self.huber ** 2, e * e)
            wt = np.where(tail, self.huber / e, 1.0) * self.s * self.s
            J = (self.P[None, :, :2, :3] - proj[..., None] * self.P[None, :, 2:3, :3]) / h[..., 2][..., None, None]     # [K,V,2,3]
            JtJ = np.einsum('kvai,kvaj->kvij', J, J)
            Jtr = np.einsum('kvai,kva->kvi', J, r)
        z = lambda a: np.where(M.reshape(M.shape + (1,) * (a.ndim - 2)), a, 0.0).sum(1)
        front = ~(M & (h[..., 2] <= 0)).any(1)                      # the header's rule: a NaN h2 is not behind
        return z(rho), z(rr), z(wt[..., None, None] * JtJ), z(wt[..., None] * Jtr), front, z(JtJ)

    def limb_terms(self, X):
        """-> (e [L] mm, J [L,n]); rows of pairs that are not active are zero, e of those NaN."""
        L = len(self.limbs)
        e, J = np.full(L, np.nan), np.zeros((L, self.n))
        for l in np.flatnonzero(self.active):
            fa, na, fb, nb = self.limbs[l]
            a, b = X[fa] - X[na], X[fb] - X[nb]
            la, lb = np.sqrt(a @ a), np.sqrt(b @ b)
            e[l] = la - lb
            if la >= FLAT_MM and lb >= FLAT_MM:
                for j, c in ((fa, a / la), (na, -a / la), (fb, -b / lb), (nb, b / lb)):
                    J[l, 3 * self.slot[j]:3 * self.slot[j] + 3] += c
        return e, J

    def terms(self, X):
        """-> (C, H [n,n], g [n], front, r2 [K], e [L]) of the whole sample at X [K,3]."""
        Ck, r2, Hk, gk, front, _ = self.reproj(X)
        e, J = self.limb_terms(X)
        ea = np.where(self.active, e, 0.0) if len(e) else e
        H, g = self.sym_w * J.T @ J, self.sym_w * J.T @ ea
        for c, k in enumerate(self.idx):
            H[3 * c:3 * c + 3, 3 * c:3 * c + 3] += Hk[k]
            g[3 * c:3 * c + 3] += gk[k]
        return Ck[self.free].sum() + self.sym_w * (ea * ea).sum(), H, g, bool(front[self.free].all()), r2, e

    def moved(self, X, d):
        Y = X.copy()
        Y[self.idx] += d.reshape(-1, 3)
        return Y

    def start(self):
        return np.where(self.free[:, None], self.X0, 0.0)          # fixed joints take part in nothing: any finite number does


def minimise(sp):
    X = sp.start()
    if sp.n == 0:
        return X
    C, H, g, front, _, _ = sp.terms(X)
    assert front
    g0, mu = np.linalg.norm(g), 0.0
    for _ in range(4000):
        if np.linalg.norm(g) <= GRAD_REL * g0:
            return X
        step = -np.linalg.solve(H + mu * np.trace(H) / sp.n * np.eye(sp.n), g)
        if np.abs(step).max() < STEP_FLOOR_MM:
            return X
        Ct, Ht, gt, ft, _, _ = sp.terms(sp.moved(X, step))
        # next to the minimum the cost changes by less than float64 resolves; there a smaller gradient is the progress
        if ft and (Ct < C or (abs(Ct - C) <= 1e-13 * C and np.linalg.norm(gt) < np.linalg.norm(g))):
            X, C, H, g = sp.moved(X, step), Ct, Ht, gt
            mu = mu / 4 if mu > 1e-12 else 0.0
        else:
            mu = max(4 * mu, 1e-6)
    raise AssertionError('the oracle did not converge')


def schedule_one(sp, max_iter=20):
    """The header's loop in float64 -> (X [K,3], status of the sample, trials, max |coordinate| of every accepted step)."""
    X, steps = sp.start(), []
    if sp.n == 0:
        return X, 1, 0, steps
    C, H, g, _, _, _ = sp.terms(X)
    lam, status, n = 1e-3, 1, 0
    for _ in range(max_iter):
        n += 1
        accept = False
        with np.errstate(all='ignore'):
            try:
                Lc = np.linalg.cholesky(H + lam * np.diag(np.diag(H)))
                d = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
                Ct, Ht, gt, ft, _, _ = sp.terms(sp.moved(X, d))
                accept = ft and Ct < C
            except np.linalg.LinAlgError:
                pass
        if accept:
            X, C, H, g = sp.moved(X, d), Ct, Ht, gt
            lam *= 0.1
            steps.append(np.abs(d).max())
            if np.abs(d).max() < 1e-5:
                status = 0
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return X, status, n, steps


def rate_of(steps):
    """The linear convergence rate the accepted steps show: the largest ratio of consecutive step lengths after the first step,
    among steps long enough for float64 to mean something (> 1e-7 mm)."""
    r = [b / a for a, b in zip(steps[1:], steps[2:]) if a > 1e-7]
    return max(r) if r else 0.0


def _samples(points, P, init, views, limbs, weighted, huber, sym_w):
    points, P, init = np.asarray(points, np.float32), np.asarray(P, np.float32), np.asarray(init, np.float32)
    return [Sample(points[b], P[b], init[b], None if views is None else views[b], limbs, weighted, huber, sym_w)
            for b in range(points.shape[0])]


def refine(points, P, init, views=None, limbs=(), weighted=False, huber=0.0, sym_w=0.0, tol_mm=1e-4):
    """-> dict of arrays: xyz [B,K,3] (init where fixed), free [B,K], active [B,L], resid [B,K,2], sym [B,L,2], cost [B,2],
    cond [B], floor [B] mm, and how far resid / sym / cost at the result move when every coordinate moves by `tol_mm`:
    resid_shift [B,K] (|J d| / sqrt(n) with J the unweighted Jacobian: the RMS is a norm, so this bounds it at any point),
    sym_shift [B,L] (|J_l|_1 tol + the curvature 4 tol^2 / the shorter limb), cost_shift [B] (2 |g|_1 tol + tol^2 sum |H|)."""
    sps = _samples(points, P, init, views, limbs, weighted, huber, sym_w)
    B, K, L = len(sps), sps[0].K, len(sps[0].limbs)
    o = dict(xyz=np.asarray(init, np.float32)[..., :3].astype(np.float64), free=np.zeros((B, K), bool), active=np.zeros((B, L), bool),
             resid=np.full((B, K, 2), np.nan), sym=np.full((B, L, 2), np.nan), cost=np.zeros((B, 2)), cond=np.full(B, np.nan),
             floor=np.zeros(B), resid_shift=np.zeros((B, K)), sym_shift=np.zeros((B, L)), cost_shift=np.zeros(B))
    for b, sp in enumerate(sps):
        o['free'][b], o['active'][b] = sp.free, sp.active
        if sp.n == 0:
            continue
        nv = sp.F.sum(1)[sp.free]
        C0, _, _, _, r20, e0 = sp.terms(sp.start())
        X = minimise(sp)
        C, H, g, _, r2, e = sp.terms(X)
        o['xyz'][b][sp.free] = X[sp.free]
        o['resid'][b][sp.free] = np.sqrt(np.stack([r20[sp.free], r2[sp.free]], -1) / nv[:, None])
        o['sym'][b] = np.stack([e0, e], -1)
        o['cost'][b] = C0, C
        ev = np.linalg.eigvalsh(H)
        o['cond'][b] = ev[-1] / ev[0] if ev[0] > 0 else np.inf
        # a step from distance d to the minimum lowers the cost by d^T H d >= lambda_min d^2; both costs carry a rounding error of
        # up to ~16 eps C (six terms per joint in sequence, six levels of the wave's butterfly, a few roundings per term)
        o['floor'][b] = np.sqrt(32 * EPS * C / ev[0]) if ev[0] > 0 else np.inf
        JtJ = sp.reproj(X)[5]
        o['resid_shift'][b][sp.free] = tol_mm * np.sqrt(np.abs(JtJ[sp.free]).sum((1, 2)) / nv)
        _, J = sp.limb_terms(X)
        for l in np.flatnonzero(sp.active):
            fa, na, fb, nb = sp.limbs[l]
            short = min(np.linalg.norm(X[fa] - X[na]), np.linalg.norm(X[fb] - X[nb]))
            o['sym_shift'][b, l] = np.abs(J[l]).sum() * tol_mm + 4 * tol_mm ** 2 / max(short, FLAT_MM)
        o['cost_shift'][b] = 2 * np.abs(g).sum() * tol_mm + tol_mm ** 2 * np.abs(H).sum()
    return o


def schedule(points, P, init, views=None, limbs=(), weighted=False, huber=0.0, sym_w=0.0, max_iter=20):
    """-> dict: xyz [B,K,3] float64, status [B] (of the sample's free joints), trials [B], rate [B]."""
    sps = _samples(points, P, init, views, limbs, weighted, huber, sym_w)
    res = [schedule_one(sp, max_iter) for sp in sps]
    xyz = np.asarray(init, np.float32)[..., :3].astype(np.float64)
    for b, (sp, r) in enumerate(zip(sps, res)):
        xyz[b][sp.free] = r[0][sp.free]
    return dict(xyz=xyz, status=np.array([r[1] for r in res], np.uint8), trials=np.array([r[2] for r in res]),
                rate=np.array([rate_of(r[3]) for r in res]))


def cost_at(points, P, init, xyz, views=None, limbs=(), weighted=False, huber=0.0, sym_w=0.0):
    """C of every sample at the float32 points xyz [B,K,3] (a kernel's output) in float64, over the joints and pairs that `init`
    makes free and active -> (C [B], slack [B]).  slack = what rounding the point to float32 can add: with d = half an ulp of
    each free coordinate, 2 |g| . d + d^T |H| d (the reasoning of _refine_oracle.cost_at)."""
    sps = _samples(points, P, init, views, limbs, weighted, huber, sym_w)
    xyz = np.asarray(xyz, np.float32)
    C, slack = np.zeros(len(sps)), np.zeros(len(sps))
    for b, sp in enumerate(sps):
        if sp.n:
            X = np.where(sp.free[:, None], xyz[b].astype(np.float64), 0.0)
            C[b], H, g, _, _, _ = sp.terms(X)
            d = (np.spacing(np.abs(xyz[b][sp.free])).astype(np.float64) / 2).ravel()
            slack[b] = 2 * np.abs(g) @ d + d @ np.abs(H) @ d
    return C, slack
