"""float64 restatement of xas_track_anchor_smooth (include/xas_hip.h) for one (track, joint): _track_oracle.Track with the
anchor term and the header's frame rules.  It does not import the library.  Track's schedule (`lm`) and its two ways of solving
a trial are kept; each gains the anchor term in its own way:
  step_dense   (a) Track's stacked residuals and autograd Jacobian for the pixels and the prior; the anchor term's block and
               gradient as half the autograd Hessian and gradient of sum psi e^T W e with psi held at the current point
  step_band    (b) psi W and psi W e by hand, added to Track's band and gradient before the damping
"""
import numpy as np
import torch

import _track_oracle as tk

F64 = torch.float64


def sym(info):
    """[..,6] (xx xy xz yy yz zz) -> [..,3,3]."""
    i = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    return np.asarray(info)[..., i]


class AnchorTrack(tk.Track):
    """One (track, joint).  Track's arguments, and anchor [T,3], info [T,6] float32 or both None; anchor_huber."""

    def __init__(self, points, P, init, frame, views=None, weighted=False, huber=0.0, acc_w=0.05, anchor=None, info=None,
                 anchor_huber=0.0):
        super().__init__(points, P, init, frame, views, weighted, huber, acc_w)      # the frames without a usable anchor
        points, P, init = (np.asarray(t, np.float32) for t in (points, P, init))
        T, V = self.T, self.V
        self.ah = float(anchor_huber)
        if anchor is None:
            anchor, info = np.full((T, 3), np.nan, np.float32), np.full((T, 6), np.nan, np.float32)
        A, W = np.asarray(anchor, np.float32).astype(np.float64), np.asarray(info, np.float32).astype(np.float64)
        with np.errstate(all='ignore'):
            usable = np.isfinite(A).all(-1) & np.isfinite(W).all(-1) & (W[:, [0, 3, 5]] >= 0).all(-1) & (W[:, [0, 3, 5]].sum(-1) > 0)
        # the views xas_triangulate_refine would use, and the start
        w = points[..., 2]
        valid = (w > 0) & np.isfinite(w)
        sel = np.zeros(T, np.uint8) if views is None else np.asarray(views, np.uint8)
        bits = np.stack([(sel >> v) & 1 for v in range(V)], 1).astype(bool)
        F = np.where((sel != 0)[:, None], valid & bits, valid)
        X0 = init[:, :3].astype(np.float64)
        start = np.where(np.isfinite(X0).all(-1, keepdims=True), X0, A)
        Pd = P.astype(np.float64)
        with np.errstate(all='ignore'):
            h2 = np.einsum('tvj,tj->tv', Pd[:, :, 2, :3], np.nan_to_num(start)) + Pd[:, :, 2, 3]
        F = F & ~(F & (h2 <= 0)).any(1, keepdims=True)                 # a start behind a view used: the anchor term alone
        self.used = np.where(usable[:, None], F, self.used)
        self.data = self.data | usable
        self.passed = int(self.data.sum()) < 2
        self.nused = self.used.sum(1)
        ti, vi = np.nonzero(self.used)
        self.ot = torch.as_tensor(ti)
        self.oP = torch.as_tensor(Pd[ti, vi])
        self.ouv = torch.as_tensor(points[ti, vi, :2].astype(np.float64))
        self.os = torch.as_tensor(points[ti, vi, 2].astype(np.float64)) if weighted else torch.ones(len(ti), dtype=F64)
        self.X0 = torch.as_tensor(self.fill(np.where(usable[:, None], start, X0)))
        self.usable = usable
        self.at = torch.as_tensor(np.nonzero(usable)[0])
        self.A = torch.as_tensor(A[usable])
        self.W = torch.as_tensor(sym(W[usable]))

    # ---- the anchor term ---------------------------------------------------------------------------------------------------
    def _anchor(self, X):
        """-> rho [n], psi [n], e [n,3] over the frames with a usable anchor."""
        e = X[self.at] - self.A
        m = torch.sqrt(torch.clamp(torch.einsum('ni,nij,nj->n', e, self.W, e), min=0.0))
        tail = (m > self.ah) if self.ah > 0 else torch.zeros_like(m, dtype=torch.bool)
        rho = torch.where(tail, 2.0 * self.ah * m - self.ah ** 2, m * m)
        psi = torch.where(tail, self.ah / torch.where(tail, m, torch.ones_like(m)), torch.ones_like(m))
        return rho, psi, e

    def anchor_cost(self, X):
        return self._anchor(X)[0].sum()

    def cost(self, X):
        C, behind, r2 = super().cost(X)
        return C + float(self.anchor_cost(X)), behind, r2

    # ---- (a) autograd ------------------------------------------------------------------------------------------------------
    def dense_system(self, X, lam):
        H, g = super().dense_system(X, 0.0)
        if len(self.at):
            with torch.no_grad():
                psi = self._anchor(X)[1]

            def irls(x):
                e = x[self.at] - self.A
                return (psi * torch.einsum('ni,nij,nj->n', e, self.W, e)).sum()
            n = 3 * self.T
            H = H + 0.5 * torch.autograd.functional.hessian(irls, X).reshape(n, n)
            g = g + 0.5 * torch.autograd.functional.jacobian(irls, X).reshape(n)
        return H + lam * torch.diag(torch.diagonal(H)), g

    # ---- (b) by hand -------------------------------------------------------------------------------------------------------
    def band_system(self, X, lam):
        band, g = super().band_system(X, 0.0)
        _, psi, e = self._anchor(X)
        Wn, We = (psi[:, None, None] * self.W).numpy(), (psi[:, None] * torch.einsum('nij,nj->ni', self.W, e)).numpy()
        for n, t in enumerate(self.at.tolist()):
            for c in range(3):
                for o in range(c + 1):
                    band[3 * t + c, o] += Wn[n, c, c - o]
                g[3 * t + c] += We[n, c]
        band[:, 0] *= 1.0 + lam
        return band, g

    # ---- the schedule: Track's; resid is NaN where a data frame uses no view -----------------------------------------------------
    def lm(self, step, max_iter, forced=None):
        res = super().lm(step, max_iter, forced)
        res['resid'][self.nused == 0] = np.nan
        return res


def make_track(case, s, k, **over):
    """AnchorTrack of joint k of track s of a case of _track_anchor_inputs -> it and the case's rows of the track."""
    m = np.nonzero(case['track'] == s)[0]
    m = m[np.argsort(case['frame'][m], kind='stable')]
    kw = dict(anchor=None if case.get('anchor') is None else case['anchor'][m][:, k],
              info=None if case.get('info') is None else case['info'][m][:, k], anchor_huber=case.get('anchor_huber', 0.0))
    kw.update(over)
    return AnchorTrack(case['points'][m][:, :, k], case['P'][m], case['init'][m][:, k], case['frame'][m],
                       None if case['views'] is None else case['views'][m][:, k], case['weighted'], case['huber'], case['acc_w'],
                       **kw), m
