"""float64 restatement of xas_calibrate_bundle (include/xas_hip.h) for one rig, in torch on the CPU.  It does not import the
library.  The cost is the header's definition; the Jacobian of form (a) comes from torch.autograd on it.  The Levenberg-Marquardt
schedule is written once (`Rig.lm`) and driven by two ways of solving a trial:
  step_dense   (a) the normal equations over ALL unknowns (cameras, then points), one dense Cholesky
  step_schur   (b) the points eliminated: the Jacobian written out by hand as the kernel forms it, S d_c = b, back-substitution
`schur_of_dense` reduces (a)'s matrix to the camera system by dense algebra: its distance to (b)'s S and b is what the GPU's
xas_calibrate_linearise is held to, and the distance between the two schedules' results what xas_calibrate_bundle is held to."""
import numpy as np
import torch

LM0, ACCEPT, REJECT, LAMBDA_MAX = 1e-3, 0.1, 10.0, 1e12
TOL_POINT, TOL_ROT, TOL_TRANS = 1e-5, 1e-9, 1e-5
# A relative cost change below this is a TIE: 1e6 x the double rounding of a sum of ~1e3 terms.  No arithmetic that sums in
# another order can be held to the oracle's decision there.
TIE_MARGIN = 1e-9
F64 = torch.float64


def cross_matrix(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def _coefficients(w):
    th2 = (w * w).sum(-1)
    small = th2 < 1e-16
    t2 = torch.where(small, torch.ones_like(th2), th2)
    th = torch.sqrt(t2)
    a = torch.where(small, torch.ones_like(th), torch.sin(th) / th)
    b = torch.where(small, torch.full_like(th, 0.5), (1.0 - torch.cos(th)) / t2)
    c = torch.where(small, torch.full_like(th, 1.0 / 6.0), (th - torch.sin(th)) / (t2 * th))
    return a[..., None, None], b[..., None, None], c[..., None, None]


def expmap(w):
    """exp([w]x) for w [...,3]; the series I + K + K^2 / 2 for |w|^2 < 1e-16, so autograd has a derivative at 0."""
    a, b, _ = _coefficients(w)
    K = cross_matrix(w)
    return torch.eye(3, dtype=w.dtype) + a * K + b * (K @ K)


def left_jacobian(w):
    _, b, c = _coefficients(w)
    K = cross_matrix(w)
    return torch.eye(3, dtype=w.dtype) + b * K + c * (K @ K)


def correction_matrix(delta):
    """T(delta) [...,4,4] = [exp omega, tau; 0 1]."""
    delta = torch.as_tensor(delta, dtype=F64)
    T = torch.zeros(delta.shape[:-1] + (4, 4), dtype=F64)
    T[..., :3, :3] = expmap(delta[..., :3])
    T[..., :3, 3] = delta[..., 3:]
    T[..., 3, 3] = 1.0
    return T


class Rig:
    """One rig's problem.  points [n,V,K,3], P [n,V,3,4], init [n,K,4] float32 arrays, views [n,K] uint8 or None."""

    def __init__(self, points, P, init, views=None, free_mask=None, weighted=False, huber=0.0, prior_rot=1e4, prior_trans=1e-2,
                 delta0=None):
        points, P, init = (np.asarray(t, np.float32) for t in (points, P, init))
        n, V, K, _ = points.shape
        self.n, self.V, self.K = n, V, K
        self.init = init
        free_mask = (((1 << V) - 1) & ~1) if free_mask is None else int(free_mask) & ((1 << V) - 1)
        self.free_cams = [v for v in range(V) if (free_mask >> v) & 1]
        self.slot = {v: s for s, v in enumerate(self.free_cams)}
        self.nc = 6 * len(self.free_cams)
        self.huber, self.prior = float(huber), (float(prior_rot), float(prior_trans))
        d0 = np.zeros((V, 6)) if delta0 is None else np.array(delta0, np.float64).reshape(V, 6)
        for v in range(V):
            if v not in self.slot:
                d0[v] = 0.0
        self.delta0 = torch.as_tensor(d0, dtype=F64)
        w = points[..., 2]
        valid = (w > 0) & np.isfinite(w)                                         # [n,V,K]
        sel = np.zeros((n, K), np.uint8) if views is None else np.asarray(views, np.uint8)
        bits = np.stack([(sel >> v) & 1 for v in range(V)], 1).astype(bool)
        used = np.where((sel != 0)[:, None, :], valid & bits, valid)
        X0 = init[..., :3].astype(np.float64)
        cand = (used.sum(1) >= 2) & np.isfinite(X0).all(-1)
        Pd = torch.as_tensor(P.astype(np.float64))
        with np.errstate(all='ignore'):
            T = correction_matrix(self.delta0)                                   # [V,4,4]
            Xh = torch.cat([torch.as_tensor(np.nan_to_num(X0)), torch.ones(n, K, 1, dtype=F64)], -1)
            h2 = torch.einsum('nvj,vjk,nlk->nvl', Pd[:, :, 2, :], T, Xh).numpy()   # [n,V,K]
        behind = (used & (h2 <= 0)).any(1)
        self.free = cand & ~behind                                               # [n,K]
        idx = -np.ones((n, K), np.int64)
        idx[self.free] = np.arange(int(self.free.sum()))
        self.M = int(self.free.sum())
        si, vi, ki = np.nonzero(used & self.free[:, None, :])
        order = np.lexsort((vi, ki, si))                                         # by point, then by view
        si, vi, ki = si[order], vi[order], ki[order]
        self.ocam, self.opt = torch.as_tensor(vi), torch.as_tensor(idx[si, ki])
        self.oP = Pd[si, vi]
        self.ouv = torch.as_tensor(points[si, vi, ki, :2].astype(np.float64))
        self.os = torch.as_tensor(points[si, vi, ki, 2].astype(np.float64)) if weighted else torch.ones(len(si), dtype=F64)
        self.oslot = torch.as_tensor([self.slot.get(int(v), -1) for v in vi], dtype=torch.int64)
        self.X0 = torch.as_tensor(X0[self.free])

    # ---- the definition --------------------------------------------------------------------------------------------
    def _resid(self, d, X):
        """d [O,6] and X [O,3] per observation -> r [O,2], h2 [O]."""
        Xp = torch.einsum('oij,oj->oi', expmap(d[:, :3]), X) + d[:, 3:]
        h = torch.einsum('oij,oj->oi', self.oP[:, :, :3], Xp) + self.oP[:, :, 3]
        return h[:, :2] / h[:, 2:3] - self.ouv, h[:, 2]

    def _robust(self, r):
        rr = (r * r).sum(-1)
        e = self.os * torch.sqrt(rr)
        tail = (e > self.huber) if self.huber > 0 else torch.zeros_like(e, dtype=torch.bool)
        rho = torch.where(tail, 2.0 * self.huber * e - self.huber ** 2, e * e)
        wgt = torch.where(tail, self.huber / torch.where(tail, e, torch.ones_like(e)), torch.ones_like(e)) * self.os ** 2
        return rho, wgt, rr

    def prior_cost(self, delta):
        f = delta[self.free_cams] if self.free_cams else delta[:0]
        return self.prior[0] * float((f[:, :3] ** 2).sum()) + self.prior[1] * float((f[:, 3:] ** 2).sum())

    def cost(self, delta, X):
        """-> C, behind (bool), sum |r|^2."""
        r, h2 = self._resid(delta[self.ocam], X[self.opt])
        rho, _, rr = self._robust(r)
        return float(rho.sum()) + self.prior_cost(delta), bool((h2 <= 0).any()), float(rr.sum())

    # ---- (a) autograd, dense -------------------------------------------------------------------------------------------
    def jacobian_autograd(self, delta, X):
        d = delta[self.ocam].clone().requires_grad_(True)
        x = X[self.opt].clone().requires_grad_(True)
        r, _ = self._resid(d, x)
        Jc, Jp = [], []
        for c in range(2):
            gd, gx = torch.autograd.grad(r[:, c].sum(), (d, x), retain_graph=True)
            Jc.append(gd); Jp.append(gx)
        return r.detach(), torch.stack(Jc, 1), torch.stack(Jp, 1)               # [O,2], [O,2,6], [O,2,3]

    def jacobian_by_hand(self, delta, X):
        """The kernel's expressions: d(u,v)/dX' from P, dX'/d omega = -[R X]x Jl, dX'/d tau = I, dX'/dX = R."""
        d, x = delta[self.ocam], X[self.opt]
        R, Jl = expmap(d[:, :3]), left_jacobian(d[:, :3])
        a = torch.einsum('oij,oj->oi', R, x)
        Xp = a + d[:, 3:]
        h = torch.einsum('oij,oj->oi', self.oP[:, :, :3], Xp) + self.oP[:, :, 3]
        uv = h[:, :2] / h[:, 2:3]
        J = (self.oP[:, :2, :3] - uv[:, :, None] * self.oP[:, 2:3, :3]) / h[:, 2, None, None]      # [O,2,3] by X'
        m = torch.cross(a[:, None, :].expand(-1, 2, -1), J, dim=-1)
        Jc = torch.cat([torch.einsum('oij,oci->ocj', Jl, m), J], -1)
        return uv - self.ouv, Jc, torch.einsum('oij,oci->ocj', R, J)

    def blocks(self, delta, X, jac):
        """Gauss-Newton blocks: Hcc [nc,nc], gc [nc], Hcp [nc,M,3], App [M,3,3], gp [M,3] (prior included, no damping)."""
        r, Jc, Jp = jac(delta, X)
        _, w, _ = self._robust(r)
        nc, M = self.nc, self.M
        Hcc, gc = torch.zeros(nc, nc, dtype=F64), torch.zeros(nc, dtype=F64)
        Hcp = torch.zeros(max(nc // 6, 1), M, 6, 3, dtype=F64)
        App = torch.zeros(M, 3, 3, dtype=F64).index_add_(0, self.opt, torch.einsum('o,oci,ocj->oij', w, Jp, Jp))
        gp = torch.zeros(M, 3, dtype=F64).index_add_(0, self.opt, torch.einsum('o,oci,oc->oi', w, Jp, r))
        cam = self.oslot >= 0
        if nc:
            s = self.oslot[cam]
            hcc = torch.zeros(nc // 6, 6, 6, dtype=F64).index_add_(0, s, torch.einsum('o,oci,ocj->oij', w[cam], Jc[cam], Jc[cam]))
            g = torch.zeros(nc // 6, 6, dtype=F64).index_add_(0, s, torch.einsum('o,oci,oc->oi', w[cam], Jc[cam], r[cam]))
            Hcc = torch.block_diag(*hcc)
            gc = g.reshape(-1)
            Hcp.index_put_((s, self.opt[cam]), torch.einsum('o,oci,ocj->oij', w[cam], Jc[cam], Jp[cam]), accumulate=True)
            pr = torch.tensor(([self.prior[0]] * 3 + [self.prior[1]] * 3) * (nc // 6), dtype=F64)
            Hcc = Hcc + torch.diag(pr)
            gc = gc + pr * delta[self.free_cams].reshape(-1)
        Hcp = Hcp.permute(0, 2, 1, 3).reshape(-1, M, 3)[:nc]
        return Hcc, gc, Hcp, App, gp

    def dense_system(self, delta, X, lam):
        Hcc, gc, Hcp, App, gp = self.blocks(delta, X, self.jacobian_autograd)
        nc, M = self.nc, self.M
        H = torch.zeros(nc + 3 * M, nc + 3 * M, dtype=F64)
        H[:nc, :nc] = Hcc
        H[:nc, nc:] = Hcp.reshape(nc, 3 * M)
        H[nc:, :nc] = Hcp.reshape(nc, 3 * M).T
        H[nc:, nc:] = torch.block_diag(*App) if M else H[nc:, nc:]
        H = H + lam * torch.diag(torch.diagonal(H))
        return H, torch.cat([gc, gp.reshape(-1)])

    def step_dense(self, delta, X, lam):
        H, g = self.dense_system(delta, X, lam)
        L, info = torch.linalg.cholesky_ex(H)
        if int(info) != 0 or not bool(torch.isfinite(H).all()):
            return None
        d = -torch.cholesky_solve(g[:, None], L)[:, 0]
        return self._spread(d[:self.nc]), d[self.nc:].reshape(-1, 3)

    def schur_of_dense(self, delta, X, lam):
        """(a)'s matrix reduced to the cameras by dense algebra -> S, b."""
        H, g = self.dense_system(delta, X, lam)
        nc = self.nc
        Z = torch.linalg.solve(H[nc:, nc:], torch.cat([H[nc:, :nc], g[nc:, None]], 1))
        return H[:nc, :nc] - H[:nc, nc:] @ Z[:, :nc], -g[:nc] + H[:nc, nc:] @ Z[:, nc]

    # ---- (b) Schur, as the kernel forms it ---------------------------------------------------------------------------
    def schur_system(self, delta, X, lam):
        Hcc, gc, Hcp, App, gp = self.blocks(delta, X, self.jacobian_by_hand)
        A = App + lam * torch.diag_embed(torch.diagonal(App, dim1=1, dim2=2))
        L, info = torch.linalg.cholesky_ex(A)
        W = torch.linalg.solve_triangular(L[None], Hcp[..., None], upper=False)[..., 0]            # [nc,M,3] = B L^-T rows
        y = torch.linalg.solve_triangular(L, gp[..., None], upper=False)[..., 0]
        S = Hcc + lam * torch.diag(torch.diagonal(Hcc)) - torch.einsum('imc,jmc->ij', W, W)
        b = -gc + torch.einsum('imc,mc->i', W, y)
        return S, b, (L, W, y, bool((info != 0).any()))

    def step_schur(self, delta, X, lam):
        S, b, (L, W, y, failed) = self.schur_system(delta, X, lam)
        if failed:
            return None
        dc = b
        if self.nc:                                                             # no free camera: the points alone
            Ls, info = torch.linalg.cholesky_ex(S)
            if int(info) != 0 or not bool(torch.isfinite(S).all()):
                return None
            dc = torch.cholesky_solve(b[:, None], Ls)[:, 0]
        z = y + torch.einsum('imc,i->mc', W, dc)
        dp = -torch.linalg.solve_triangular(L.transpose(1, 2), z[..., None], upper=True)[..., 0]
        return self._spread(dc), dp

    def _spread(self, dc):
        d = torch.zeros(self.V, 6, dtype=F64)
        if self.nc:
            d[self.free_cams] = dc.reshape(-1, 6)
        return d

    # ---- the schedule ---------------------------------------------------------------------------------------------------
    def lm(self, step, max_iter, forced=None):
        """The schedule.  `forced` {trial: accept?} overrules the comparison C(trial) < C at those trials (a TIE, below): the
        result says `invalid` if a forced accept had no trial state to move to.  `ties` lists the trials whose relative cost
        change was under TIE_MARGIN, where another order of summation may decide the other way."""
        forced = forced or {}
        delta, X, lam = self.delta0.clone(), self.X0.clone(), LM0
        nobs = len(self.ocam)
        C, _, r2 = self.cost(delta, X)
        res = {'cost': [C, C], 'rms': [np.sqrt(r2 / nobs) if nobs else np.nan] * 2, 'status': 1, 'trials': 0, 'accepted': 0,
               'decisions': [], 'natural': [], 'margins': [], 'ties': [], 'invalid': False}
        if self.M == 0:
            res['status'] = 2
        else:
            for it in range(max_iter):
                res['trials'] += 1
                sol, acc = step(delta, X, lam), False
                if sol is not None:
                    dc, dp = sol
                    Ct, bad, r2t = self.cost(delta + dc, X + dp)
                    acc = (not bad) and Ct < C
                    res['margins'].append(abs(Ct - C) / abs(C) if np.isfinite(Ct) and C != 0 else np.inf)
                    if not bad and res['margins'][-1] < TIE_MARGIN:
                        res['ties'].append(it)
                res['natural'].append(bool(acc))
                if it in forced and forced[it] != acc:
                    if forced[it] and (sol is None or bad or not np.isfinite(Ct)):
                        res['invalid'] = True
                        break
                    acc = forced[it]
                res['decisions'].append(bool(acc))
                if acc:
                    delta, X, C, r2, lam = delta + dc, X + dp, Ct, r2t, lam * ACCEPT
                    res['accepted'] += 1
                    if float(dp.abs().max()) < TOL_POINT and float(dc[:, :3].abs().max()) < TOL_ROT and \
                            float(dc[:, 3:].abs().max()) < TOL_TRANS:
                        res['status'] = 0
                        break
                else:
                    lam *= REJECT
                    if lam > LAMBDA_MAX:
                        break
            res['cost'][1], res['rms'][1] = C, np.sqrt(r2 / nobs)
        out = self.init.copy()
        xyz = out[..., :3]
        xyz[self.free] = X.numpy().astype(np.float32)
        out[..., :3] = xyz
        res.update(delta=delta.numpy(), X=X.numpy(), out=out)
        return res


def solve(case, step='schur', rigs=None):
    """Every rig of a case (_calib_inputs) -> list of Rig.lm results, by rig."""
    out = []
    for r in range(case['R']) if rigs is None else rigs:
        rig = make_rig(case, r)
        out.append(rig.lm(rig.step_schur if step == 'schur' else rig.step_dense, case['max_iter']))
    return out


def make_rig(case, r, delta0=None):
    m = case['rig'] == r
    d0 = case['delta0'][r] if delta0 is None else delta0
    return Rig(case['points'][m], case['P'][m], case['init'][m], None if case['views'] is None else case['views'][m],
               case['free_mask'], case['weighted'], case['huber'], case['prior_rot'], case['prior_trans'], d0)


def similarity_align(A, B):
    """Least-squares similarity (scale, rotation, translation) of points A [M,3] onto B -> A aligned."""
    ca, cb = A.mean(0), B.mean(0)
    a, b = A - ca, B - cb
    U, s, Vt = np.linalg.svd(b.T @ a)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    scale = np.trace(np.diag(s) @ D) / (a * a).sum()
    return scale * a @ R.T + cb


def follow(rig, decisions, max_iter):
    """The oracle's two schedules made to take `decisions` (what another implementation decided, trial by trial).  -> (dense,
    schur) results.  Raises if a decision differs from the oracle's own at a trial that is no TIE, in either schedule: only at a
    tie may another order of summation decide the other way."""
    forced = dict(enumerate(decisions))
    res = [rig.lm(step, max_iter, forced) for step in (rig.step_dense, rig.step_schur)]
    for r in res:
        if r['invalid']:
            raise AssertionError('a forced accept had no trial state: %s' % (decisions,))
        for t, (mine, theirs) in enumerate(zip(r['natural'], decisions)):
            if mine != theirs and t not in r['ties']:
                raise AssertionError('trial %d decided %s where the oracle decides %s with margin %.2e' % (
                    t, theirs, mine, r['margins'][t] if t < len(r['margins']) else float('nan')))
    return res
