"""Oracle of xas_smpl_fit_tracks_smooth (include/xas_hip.h): tests/_smplfit_tracks_oracle.py's Track supplies the data terms; this
file adds the acceleration prior's residuals on the frame numbers, the rule for repeated frame numbers and the unwrapping of the
root vectors, builds the full (75 T + 10) Jacobian by autograd, solves the damped normal equations DENSELY and a second time by a
hand-written block recurrence with border (the distance of the two is the oracle's own SPREAD), and runs the header's
Levenberg-Marquardt step for step.  CPU, float64.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np
import torch

import _smplfit_tracks_oracle as to
from _smplfit_oracle import STEP_TOL

NY, NB = to.NY, to.NB


def stencil(f, k):
    """track_stencil.h's TsStencil centred at position k of the frame numbers f -> (cm, c0, cp, ws)."""
    h0, h1 = float(f[k] - f[k - 1]), float(f[k + 1] - f[k])
    cm, cp = 1.0 / h0, 1.0 / h1
    return cm, -(cm + cp), cp, 2.0 / (h0 + h1)


def unwrap(y):
    """The root vectors of y [T,75] in track order, each after the first replaced by the equivalent vector nearest the one before."""
    y = y.clone()
    for i in range(1, len(y)):
        th = float(y[i, :3].norm())
        if th > 0.0:
            u = y[i, :3] / th
            k = float(np.rint((float(u @ y[i - 1, :3]) - th) / (2 * math.pi)))
            y[i, :3] = y[i, :3] + (2 * math.pi * k) * u
    return y


class SmoothTrack(to.Track):
    """to.Track plus the frame numbers (ascending; the samples of a track in its order) and the two weights."""

    def __init__(self, x0, tgt, w, frames, m, wp, ws, rot_w, trans_w):
        super().__init__(x0, tgt, w, m, wp, ws)
        self.rot_w, self.trans_w = float(rot_w), float(trans_w)
        frames = [int(f) for f in frames]
        if rot_w + trans_w > 0:                                      # a usable frame with the number of the usable frame before it
            last = None
            for t in range(len(frames)):
                if not self.usable[t]:
                    continue
                if last is not None and frames[t] == last:
                    self.usable[t] = False
                else:
                    last = frames[t]
            self.rows = [t for t, u in enumerate(self.usable) if u]
            self.T = len(self.rows)
            beta = torch.zeros(NB, dtype=torch.float64)
            for t in (self.rows or range(len(frames))):
                beta = beta + self.x0[t, NY:]
            self.beta0 = beta / max(len(self.rows or range(len(frames))), 1)
            self.y0 = self.x0[self.rows, :NY].clone() if self.T else torch.zeros(0, NY, dtype=torch.float64)
        self.raw_y0 = self.y0.clone()
        if rot_w > 0 and self.T:
            self.y0 = unwrap(self.y0)
        self.f = [frames[t] for t in self.rows]
        self.wvec = torch.full((NY,), self.rot_w, dtype=torch.float64)
        self.wvec[3:6] = self.trans_w
        self.temporal = self.T >= 3 and rot_w + trans_w > 0

    def prior_residual(self, y):
        """[(T - 2) 75]: sqrt(ws_k w_c) (cm y_k-1 + c0 y_k + cp y_k+1), stencil k = 1 .. T - 2, c ascending."""
        rows = []
        for k in range(1, self.T - 1):
            cm, c0, cp, ws = stencil(self.f, k)
            rows.append(torch.sqrt(ws * self.wvec) * (cm * y[k - 1] + c0 * y[k] + cp * y[k + 1]))
        return torch.cat(rows)

    def prior_cost(self, y):
        return float((self.prior_residual(y) ** 2).sum()) if self.temporal else 0.0

    def accel(self, y):
        """[T - 2, 75]: the stencil's second differences of y."""
        return torch.stack([sum(c * y[k + o] for c, o in zip(stencil(self.f, k)[:3], (-1, 0, 1))) for k in range(1, self.T - 1)])

    def total(self, y, beta):
        return self.cost(y, beta) + self.prior_cost(y)

    def normal(self, y, beta):
        """H, g of the whole cost: the data's J^T J, J^T r and the prior's, the latter's Jacobian by autograd."""
        H, g = super().normal(y, beta)
        if self.temporal:
            n = NY * self.T
            Jp = torch.autograd.functional.jacobian(lambda v: self.prior_residual(v.view(self.T, NY)), y.reshape(-1))
            rp = self.prior_residual(y)
            H, g = H.clone(), g.clone()
            H[:n, :n] += Jp.T @ Jp
            g[:n] += Jp.T @ rp
        return H, g


def solve_block(H, g, lam, T):
    """(H + lam diag H) d = -g by the block recurrence with border: block rows L_ii, L_i,i-1, L_i,i-2 and L_beta,i in frame order,
    the corner last, then both substitutions -> d, or None at a pivot that is not positive."""
    A = H + lam * torch.diag(torch.diagonal(H))
    n = NY * T
    blk = lambda i, j: A[NY * i:NY * (i + 1), NY * j:NY * (j + 1)]
    tsolve = lambda L, M: torch.linalg.solve_triangular(L, M, upper=False)           # L^-1 M
    Ld, L1, L2, Lb, z = [], [], [], [], []
    S, b = A[n:, n:].clone(), -g[n:].clone()
    for i in range(T):
        l2 = tsolve(Ld[i - 2], blk(i, i - 2).T).T if i >= 2 else None
        l1 = None
        if i >= 1:
            M = blk(i, i - 1) - (l2 @ L1[i - 1].T if i >= 2 else 0)
            l1 = tsolve(Ld[i - 1], M.T).T
        Si = blk(i, i) - (l1 @ l1.T if i >= 1 else 0) - (l2 @ l2.T if i >= 2 else 0)
        ld, info = torch.linalg.cholesky_ex(Si)
        if int(info) != 0:
            return None
        R = A[n:, NY * i:NY * (i + 1)] - (Lb[i - 1] @ l1.T if i >= 1 else 0) - (Lb[i - 2] @ l2.T if i >= 2 else 0)
        lb = tsolve(ld, R.T).T
        rz = -g[NY * i:NY * (i + 1)] - (l1 @ z[i - 1] if i >= 1 else 0) - (l2 @ z[i - 2] if i >= 2 else 0)
        zi = tsolve(ld, rz.unsqueeze(1))[:, 0]
        S, b = S - lb @ lb.T, b - lb @ zi
        Ld.append(ld), L1.append(l1), L2.append(l2), Lb.append(lb), z.append(zi)
    Ls, info = torch.linalg.cholesky_ex(S)
    if int(info) != 0:
        return None
    db = torch.cholesky_solve(b.unsqueeze(1), Ls)[:, 0]
    d = torch.zeros(n + NB, dtype=torch.float64)
    d[n:] = db
    for i in range(T - 1, -1, -1):
        r = z[i] - Lb[i].T @ db
        if i + 1 < T:
            r = r - L1[i + 1].T @ d[NY * (i + 1):NY * (i + 2)]
        if i + 2 < T:
            r = r - L2[i + 2].T @ d[NY * (i + 2):NY * (i + 3)]
        d[NY * i:NY * (i + 1)] = torch.linalg.solve_triangular(Ld[i].T, r.unsqueeze(1), upper=True)[:, 0]
    return d


def lm(trk, max_iters, lambda0=1e-3):
    """The header's loop on one track, every step solved densely -> to.lm's dict; cost is the whole C_s, frame_cost the data cost."""
    y, beta = trk.y0.clone(), trk.beta0.clone()
    if trk.T == 0:
        return dict(y=y, beta=beta, cost=(0.0, 0.0), frame_cost=np.zeros((0, 2)), trials=0, status=2, spread=0.0, margin=np.inf, accepts=[])
    c0 = trk.frame_costs(y, beta)
    C = trk.total(y, beta)
    C0, st, it, lam, spread, margin, accepts = C, 1, 0, lambda0, 0.0, np.inf, []
    n = NY * trk.T
    if max_iters > 0:
        H, g = trk.normal(y, beta)
    while it < max_iters:
        it += 1
        accept, d = False, to.solve_dense(H, g, lam)
        if d is not None:
            other = solve_block(H, g, lam, trk.T)
            if other is not None:
                spread = max(spread, to.rel(other, d))
            yt, bt = y + d[:n].view(trk.T, NY), beta + d[n:]
            Ct = trk.total(yt, bt)
            accept = bool(np.isfinite(Ct) and Ct < C)
            if np.isfinite(Ct):
                margin = min(margin, abs(Ct - C) / C)
        accepts.append(accept)
        if accept:
            y, beta, C, lam = yt, bt, Ct, lam * 0.1
            if float(d.abs().max()) < STEP_TOL:
                st = 0
                break
            H, g = trk.normal(y, beta)
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return dict(y=y, beta=beta, cost=(C0, C), frame_cost=np.stack([c0, trk.frame_costs(y, beta)], 1), trials=it, status=st,
                spread=spread, margin=margin, accepts=accepts)


def rotation(om):
    """The plain exponential map of the header, float64 [3] -> [3,3]."""
    th = float(om.norm())
    K = torch.tensor([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]], dtype=torch.float64)
    if th * th < 1e-16:
        return torch.eye(3, dtype=torch.float64) + K + K @ K / 2
    K = K / th
    return torch.eye(3, dtype=torch.float64) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
