"""Oracle of xas_smpl_fit_tracks (include/xas_hip.h): per track the full (75 T + 10) Jacobian from the per-frame autograd
Jacobians of tests/_smplfit_oracle.py, the damped normal equations solved DENSELY, and the header's Levenberg-Marquardt
schedule step for step.  A second solve eliminates the frames by hand (Schur complement); the difference between the two is
the oracle's own spread, the yardstick of the device's distance.  CPU, float64.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

from _smplfit_oracle import STEP_TOL, cost_of, linearise, residual

NY, NB = 75, 10
EPS = float(np.finfo(np.float64).eps)


def frame_usable(x0, m, tgt, w, wp, ws):
    """xas_smpl_fit's rule at the frame's own init: >= 6 joints used and a finite cost there."""
    return int((w > 0).sum()) >= 6 and bool(np.isfinite(cost_of(residual(x0, m, tgt, w, wp, ws))))


class Track:
    """One track: x0 [T,85], tgt [T,18,3], w [T,18] (float64 tensors of the fp32 inputs) IN ASCENDING FRAME ORDER."""

    def __init__(self, x0, tgt, w, m, wp, ws):
        self.m, self.wp, self.ws = m, wp, ws
        self.x0, self.tgt, self.w = x0.double(), tgt.double(), w.double()
        self.usable = [frame_usable(self.x0[t], m, self.tgt[t], self.w[t], wp, ws) for t in range(len(x0))]
        self.rows = [t for t, u in enumerate(self.usable) if u]
        self.T = len(self.rows)
        beta = torch.zeros(NB, dtype=torch.float64)
        for t in (self.rows or range(len(x0))):                     # ascending frame order, in double
            beta = beta + self.x0[t, NY:]
        self.beta0 = beta / max(len(self.rows or range(len(x0))), 1)
        self.y0 = self.x0[self.rows, :NY].clone() if self.T else torch.zeros(0, NY, dtype=torch.float64)

    def point(self, y, beta, i):
        return torch.cat([y[i], beta])

    def frame_costs(self, y, beta):
        return [cost_of(residual(self.point(y, beta, i), self.m, self.tgt[t], self.w[t], self.wp, self.ws)) for i, t in enumerate(self.rows)]

    def cost(self, y, beta):
        C = 0.0
        for c in self.frame_costs(y, beta):
            C += c
        return C

    def jacobian(self, y, beta):
        """-> r [133 T], J [133 T, 75 T + 10]: frame i's rows hold its 75 columns and the shared last 10."""
        T = self.T
        r, J = torch.zeros(133 * T, dtype=torch.float64), torch.zeros(133 * T, NY * T + NB, dtype=torch.float64)
        for i, t in enumerate(self.rows):
            ri, Ji = linearise(self.point(y, beta, i), self.m, self.tgt[t], self.w[t], self.wp, self.ws)
            r[133 * i:133 * (i + 1)] = ri
            J[133 * i:133 * (i + 1), NY * i:NY * (i + 1)] = Ji[:, :NY]
            J[133 * i:133 * (i + 1), NY * T:] = Ji[:, NY:]
        return r, J

    def normal(self, y, beta):
        r, J = self.jacobian(y, beta)
        return J.T @ J, J.T @ r


def solve_dense(H, g, lam):
    """(H + lam diag H) d = -g by one dense Cholesky -> d, or None at a pivot that is not positive."""
    A = H + lam * torch.diag(torch.diagonal(H))
    L, info = torch.linalg.cholesky_ex(A)
    if int(info) != 0:
        return None
    return -torch.cholesky_solve(g.unsqueeze(1), L)[:, 0]


def solve_schur(H, g, lam, T):
    """The same system by eliminating each frame's 75 unknowns -> dict(d, reduced [10,10] (summed, damped), rhs [10]), or
    None at a pivot that is not positive."""
    A = H + lam * torch.diag(torch.diagonal(H))
    n = NY * T
    S, b = A[n:, n:].clone(), -g[n:].clone()
    keep = []
    for i in range(T):
        sl = slice(NY * i, NY * (i + 1))
        L11, info = torch.linalg.cholesky_ex(A[sl, sl])
        if int(info) != 0:
            return None
        L21 = torch.linalg.solve_triangular(L11, A[sl, n:], upper=False).T           # [10,75]
        z = torch.linalg.solve_triangular(L11, -g[sl].unsqueeze(1), upper=False)[:, 0]
        S = S - L21 @ L21.T
        b = b - L21 @ z
        keep.append((L11, L21, z))
    Ls, info = torch.linalg.cholesky_ex(S)
    if int(info) != 0:
        return None
    db = torch.cholesky_solve(b.unsqueeze(1), Ls)[:, 0]
    d = torch.zeros(n + NB, dtype=torch.float64)
    d[n:] = db
    for i, (L11, L21, z) in enumerate(keep):
        d[NY * i:NY * (i + 1)] = torch.linalg.solve_triangular(L11.T, (z - L21.T @ db).unsqueeze(1), upper=True)[:, 0]
    return dict(d=d, reduced=S, rhs=b)


def reduced_by_lu(H, g, lam, T):
    """The reduced system a third way (LU of the whole leading block): its distance to solve_schur's is the spread of `reduced`."""
    A = H + lam * torch.diag(torch.diagonal(H))
    n = NY * T
    X = torch.linalg.solve(A[:n, :n], torch.cat([A[:n, n:], -g[:n].unsqueeze(1)], 1))
    return A[n:, n:] - A[n:, :n] @ X[:, :NB], -g[n:] - A[n:, :n] @ X[:, NB]


def residual_of(H, g, lam, d):
    """max |(H + lam diag H) d + g| / max |g|: how well d solves the dense system."""
    A = H + lam * torch.diag(torch.diagonal(H))
    return float((A @ d + g).abs().max() / g.abs().max())


def rel(a, b):
    """max |a - b| relative to the largest |b|."""
    return float((a - b).abs().max() / b.abs().max())


def lm(trk, max_iters, lambda0=1e-3):
    """The header's loop on one track, every step solved densely.  -> dict(y [T,75], beta, cost
    (start, result), frame_cost [T,2], trials, status, spread = the largest relative gap of the dense and the eliminated step
    over the trials, margin = the smallest |C_trial - C| / C over the trials, accepts)."""
    y, beta = trk.y0.clone(), trk.beta0.clone()
    if trk.T == 0:
        return dict(y=y, beta=beta, cost=(0.0, 0.0), frame_cost=np.zeros((0, 2)), trials=0, status=2, spread=0.0, margin=np.inf, accepts=[])
    c0 = trk.frame_costs(y, beta)
    C = trk.cost(y, beta)
    C0, st, it, lam, spread, margin, accepts = C, 1, 0, lambda0, 0.0, np.inf, []
    n = NY * trk.T
    if max_iters > 0:
        H, g = trk.normal(y, beta)
    while it < max_iters:
        it += 1
        accept, d = False, solve_dense(H, g, lam)
        if d is not None:
            other = solve_schur(H, g, lam, trk.T)
            if other is not None:
                spread = max(spread, rel(other['d'], d))
            yt, bt = y + d[:n].view(trk.T, NY), beta + d[n:]
            Ct = trk.cost(yt, bt)
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
