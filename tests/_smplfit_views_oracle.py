"""Oracle of xas_smpl_fit_views (include/xas_hip.h) in float64 torch, one sample at a time, on the CPU.  The model is
_smplfit_oracle's (by import); which views count is _refine_oracle.views_used plus the header's two further rules; the pixel
term of the by-hand assembly is _refine_oracle.terms and the anchor's matrix is _track_anchor_oracle.sym.  The Gauss-Newton
system is formed twice:
  normal_rows    (a) the stacked rows sqrt(w_irls) r of every term (the IRLS weight detached) as a function of x, their Jacobian
                 from autograd: H = J^T J, g = J^T r
  normal_blocks  (b) per joint the cost c_k, the 3x3 block A_k and the gradient b_k by hand, and dY/dx from autograd:
                 H = sum_k Jy_k^T A_k Jy_k, g = sum_k Jy_k^T b_k
Their distance is the oracle's own SPREAD.  `lm` follows the header's schedule.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import _refine_oracle as ro
import _smplfit_oracle as so
import _track_anchor_oracle as tao

F64 = torch.float64
EPS = float(np.finfo(np.float64).eps)
STEP_TOL = so.STEP_TOL
ANCHOR_BIT = 0x80


def rel(a, b):
    """Largest |a - b| relative to the largest |b| (0 where both are all zero)."""
    a, b = torch.as_tensor(np.asarray(a), dtype=F64), torch.as_tensor(np.asarray(b), dtype=F64)
    top = float(b.abs().max()) if b.numel() else 0.0
    return float((a - b).abs().max()) / top if top > 0 else float((a - b).abs().max()) if a.numel() else 0.0


def anchor_usable(anchor, info):
    """[K,3], [K,6] float32 -> [K] bool: TsAnchored::load's rule."""
    A, W = np.asarray(anchor, np.float32).astype(np.float64), np.asarray(info, np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        return np.isfinite(A).all(-1) & np.isfinite(W).all(-1) & (W[:, [0, 3, 5]] >= 0).all(-1) & (W[:, [0, 3, 5]].sum(-1) > 0)


class Sample:
    """One sample of a case.  x0 [85] (fp32 values), points [C,18,3], P [C,3,4] float32, views [18] uint8 or None, anchor [18,3]
    and info [18,6] float32 or both None."""

    def __init__(self, m, x0, points, P, views=None, anchor=None, info=None, weighted=False, huber=0.0, anchor_huber=0.0, wp=10.0,
                 ws=2.5, center_idx=0):
        self.m, self.center = m, (None if center_idx < 0 else center_idx)
        self.x0 = torch.as_tensor(np.asarray(x0, np.float32).astype(np.float64))
        self.pts, self.P = np.asarray(points, np.float32), np.asarray(P, np.float32)
        self.C = self.pts.shape[0]
        self.weighted, self.huber_px, self.ah, self.wp, self.ws = bool(weighted), float(huber), float(anchor_huber), float(wp), float(ws)
        with torch.no_grad():
            Y0 = self.joints(self.x0).numpy()
        self.F = []                                                       # per joint: the views it uses
        for k in range(18):
            F = ro.views_used(self.pts[:, k], 0 if views is None else int(views[k]))
            keep = []
            for v in F:
                Pv = self.P[v].astype(np.float64)
                with np.errstate(all='ignore'):
                    h2 = Pv[2, :3] @ Y0[k] + Pv[2, 3]
                if np.isfinite(self.pts[v, k, :2]).all() and not h2 <= 0:   # NaN is not behind, as everywhere
                    keep.append(v)
            self.F.append(keep)
        self.anchored = anchor_usable(anchor, info) if anchor is not None else np.zeros(18, bool)
        self.A = None if anchor is None else np.asarray(anchor, np.float32).astype(np.float64)
        self.W = None if info is None else tao.sym(np.asarray(info, np.float32).astype(np.float64))
        self.used = np.array([sum(1 << v for v in self.F[k]) | (ANCHOR_BIT if self.anchored[k] else 0) for k in range(18)], np.uint8)
        self.n_used = int((self.used != 0).sum())

    def joints(self, x):
        return so.joints(x, self.m, center_idx=self.center)

    # ---- the terms as torch functions of Y (for autograd) ----------------------------------------------------------------------
    def _index(self):
        if not hasattr(self, 'ok'):
            kv = [(k, v) for k in range(18) for v in self.F[k]]
            self.ok = torch.as_tensor([k for k, _ in kv], dtype=torch.long)
            self.oP = torch.as_tensor(np.stack([self.P[v] for _, v in kv]).astype(np.float64)) if kv else torch.zeros(0, 3, 4, dtype=F64)
            self.ouv = torch.as_tensor(np.stack([self.pts[v, k, :2] for k, v in kv]).astype(np.float64)) if kv else torch.zeros(0, 2, dtype=F64)
            self.os = torch.as_tensor([float(self.pts[v, k, 2]) if self.weighted else 1.0 for k, v in kv], dtype=F64)
            self.ak = torch.as_tensor(np.nonzero(self.anchored)[0], dtype=torch.long)
            self.aA = torch.as_tensor(self.A[self.anchored]) if self.A is not None else torch.zeros(0, 3, dtype=F64)
            self.aW = torch.as_tensor(self.W[self.anchored]) if self.W is not None else torch.zeros(0, 3, 3, dtype=F64)

    def pixel_residuals(self, Y):
        """-> r [n,2] px and h2 [n] over the observations used, joints ascending, then views ascending."""
        self._index()
        h = torch.einsum('nij,nj->ni', self.oP[:, :, :3], Y[self.ok]) + self.oP[:, :, 3]
        return h[:, :2] / h[:, 2:3] - self.ouv, h[:, 2]

    def anchor_residuals(self, Y):
        self._index()
        return Y[self.ak] - self.aA

    @staticmethod
    def huber(e, delta):
        """e [n] >= 0 -> (rho, psi)."""
        tail = (e > delta) if delta > 0 else torch.zeros_like(e, dtype=torch.bool)
        safe = torch.where(tail, e, torch.ones_like(e))
        return torch.where(tail, 2.0 * delta * e - delta * delta, e * e), torch.where(tail, delta / safe, torch.ones_like(e))

    def weights(self, x):
        """The IRLS weights at x, detached: w [n] of the pixel terms (psi s^2) and psi [m] of the anchors."""
        with torch.no_grad():
            Y = self.joints(x)
            r, _ = self.pixel_residuals(Y)
            w = self.huber(self.os * r.norm(dim=1), self.huber_px)[1] * self.os * self.os
            e = self.anchor_residuals(Y)
            psi = self.huber(torch.sqrt(torch.clamp(torch.einsum('ni,nij,nj->n', e, self.aW, e), min=0.0)), self.ah)[1]
        return w, psi

    def cost(self, x):
        """-> (C, in front of every view used).  Joints ascending: its views ascending, then its anchor; then the priors."""
        with torch.no_grad():
            Y = self.joints(x)
            r, h2 = self.pixel_residuals(Y)
            rho = self.huber(self.os * r.norm(dim=1), self.huber_px)[0].tolist()
            e = self.anchor_residuals(Y)
            rho_a = self.huber(torch.sqrt(torch.clamp(torch.einsum('ni,nij,nj->n', e, self.aW, e), min=0.0)), self.ah)[0].tolist()
            front = not bool((h2 <= 0).any())
            C, n, m = 0.0, 0, 0
            for k in range(18):
                for _ in self.F[k]:
                    C += rho[n]
                    n += 1
                if self.anchored[k]:
                    C += rho_a[m]
                    m += 1
            for i in range(6, 75):
                C += self.wp * float(x[i]) ** 2
            for i in range(75, 85):
                C += self.ws * float(x[i]) ** 2
        return C, front

    # ---- (a) stacked rows ------------------------------------------------------------------------------------------------------
    def rows(self, x, w):
        """The rows sqrt(w_irls) r of the pixel terms and the priors at x, the weights `w` detached."""
        r, _ = self.pixel_residuals(self.joints(x))
        return torch.cat([(w.sqrt().unsqueeze(1) * r).reshape(-1), (self.wp ** 0.5) * x[6:75], (self.ws ** 0.5) * x[75:85]])

    def normal_rows(self, x):
        """H = J^T J and g = J^T r of the rows, J from autograd; the anchors join as Je^T (psi W) Je and Je^T (psi W) e with
        Je = d e / d x from autograd (W is not factored: it may have rank one)."""
        x = x.detach().double()
        w, psi = self.weights(x)
        f = lambda y: self.rows(y, w)
        J = torch.autograd.functional.jacobian(f, x, vectorize=True).detach()
        r = f(x).detach()
        H, g = J.T @ J, J.T @ r
        if len(self.ak):
            fe = lambda y: self.anchor_residuals(self.joints(y)).reshape(-1)
            Je = torch.autograd.functional.jacobian(fe, x, vectorize=True).detach().reshape(-1, 3, 85)
            e = fe(x).detach().reshape(-1, 3)
            H = H + torch.einsum('nai,n,nab,nbj->ij', Je, psi, self.aW, Je)
            g = g + torch.einsum('nai,n,nab,nb->i', Je, psi, self.aW, e)
        return H, g

    # ---- (b) joint blocks --------------------------------------------------------------------------------------------------------
    def blocks(self, x):
        """-> A [18,3,3], b [18,3], c [18] by hand (numpy), zero for a joint not used."""
        with torch.no_grad():
            Y = self.joints(x.detach().double()).numpy()
        A, b, c = np.zeros((18, 3, 3)), np.zeros((18, 3)), np.zeros(18)
        for k in range(18):
            if self.F[k]:
                c[k], _, A[k], b[k], _ = ro.terms(self.pts[:, k], self.P, Y[k], self.F[k], self.weighted, self.huber_px)
            if self.anchored[k]:
                e = Y[k] - self.A[k]
                We = self.W[k] @ e
                mm = float(np.sqrt(max(e @ We, 0.0)))
                tail = self.ah > 0 and mm > self.ah
                psi = self.ah / mm if tail else 1.0
                c[k] += 2 * self.ah * mm - self.ah ** 2 if tail else mm * mm
                A[k] += psi * self.W[k]
                b[k] += psi * We
        return A, b, c

    def normal_blocks(self, x):
        x = x.detach().double()
        A, b, _ = self.blocks(x)
        Jy = torch.autograd.functional.jacobian(lambda y: self.joints(y).reshape(-1), x, vectorize=True).detach().reshape(18, 3, 85)
        H = torch.einsum('kai,kab,kbj->ij', Jy, torch.as_tensor(A), Jy)
        g = torch.einsum('kai,ka->i', Jy, torch.as_tensor(b))
        prior = torch.cat([torch.zeros(6, dtype=F64), torch.full((69,), self.wp, dtype=F64), torch.full((10,), self.ws, dtype=F64)])
        return H + torch.diag(prior), g + prior * x

    def blocks_autograd(self, x):
        """The joint blocks a second way: the pixel rows sqrt(w_irls) r as a function of Y, their Jacobian from autograd, J^T J
        and J^T r cut into joints; the anchors' psi W and psi W e join.  -> [18,9] like joint_blocks."""
        x = x.detach().double()
        w, psi = self.weights(x)
        with torch.no_grad():
            Y = self.joints(x)
        f = lambda y: (w.sqrt().unsqueeze(1) * self.pixel_residuals(y.view(18, 3))[0]).reshape(-1)
        H, g = torch.zeros(54, 54, dtype=F64), torch.zeros(54, dtype=F64)
        if len(self.ok):
            J = torch.autograd.functional.jacobian(f, Y.reshape(-1), vectorize=True).detach()
            H, g = J.T @ J, J.T @ f(Y.reshape(-1))
        A = torch.stack([H[3 * k:3 * k + 3, 3 * k:3 * k + 3] for k in range(18)])
        b = g.view(18, 3).clone()
        e = self.anchor_residuals(Y)
        for n, k in enumerate(self.ak.tolist()):
            A[k] += psi[n] * self.aW[n]
            b[k] += psi[n] * (self.aW[n] @ e[n])
        return torch.cat([A[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], b], dim=1).numpy()

    def joint_blocks(self, x):
        A, b, _ = self.blocks(x)
        return np.concatenate([A[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], b], axis=1)

    # ---- the header's loop --------------------------------------------------------------------------------------------------------
    def passed(self):
        C, _ = self.cost(self.x0)
        return self.n_used < 6 or not np.isfinite(C)

    def lm(self, max_iters, lambda0=1e-3):
        """-> dict(x, cost (start, result), iters, status, costs: per trial the cost (or None at a failed factorisation),
        accepts, spread: the largest relative gap of the steps of the two assemblies, margin: the smallest |Ct - C| / C)."""
        x = self.x0.clone()
        C, _ = self.cost(x)
        C0 = C
        if self.n_used < 6 or not np.isfinite(C):
            return dict(x=x, cost=(C0, C0), iters=0, status=2, accepts=[], spread=0.0, margin=np.inf, costs=[])
        st, it, lam, spread, margin, accepts, costs = 1, 0, lambda0, 0.0, np.inf, [], []
        if max_iters > 0:
            H, g = self.normal_rows(x)
            Hb, gb = self.normal_blocks(x)
        while it < max_iters:
            it += 1
            accept, d = False, solve(H, g, lam)
            Ct = None
            if d is not None:
                db = solve(Hb, gb, lam)
                if db is not None:
                    spread = max(spread, rel(db, d))
                xt = x + d
                Ct, front = self.cost(xt)
                accept = bool(front and np.isfinite(Ct) and Ct < C)
                if np.isfinite(Ct):
                    margin = min(margin, abs(Ct - C) / C)
            costs.append(Ct)
            accepts.append(accept)
            if accept:
                x, C, lam = xt, Ct, lam * 0.1
                if float(d.abs().max()) < STEP_TOL:
                    st = 0
                    break
                H, g = self.normal_rows(x)
                Hb, gb = self.normal_blocks(x)
            else:
                lam *= 10.0
                if lam > 1e12:
                    break
        return dict(x=x, cost=(C0, C), iters=it, status=st, accepts=accepts, spread=spread, margin=margin, costs=costs)


def solve(H, g, lam):
    """(H + lam diag H) d = -g by Cholesky -> d, or None at a pivot that is not positive."""
    L, info = torch.linalg.cholesky_ex(H + lam * torch.diag(torch.diagonal(H)))
    if int(info) != 0 or not torch.isfinite(L).all():
        return None
    return -torch.cholesky_solve(g.unsqueeze(1), L)[:, 0]
