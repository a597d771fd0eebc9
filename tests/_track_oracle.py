"""float64 restatement of xas_track_smooth (include/xas_hip.h) for one (track, joint), in torch / numpy on the CPU.  It does not
import the library.  The cost is the header's definition.  The Levenberg-Marquardt schedule is written once (`Track.lm`) and
driven by two ways of solving a trial:
  step_dense   (a) every residual stacked (sqrt(w) r of the data, sqrt(acc_w ws) q of the prior), the Jacobian from
               torch.autograd on that vector, H = J^T J, g = J^T r, one dense Cholesky
  step_band    (b) the Jacobian by hand as the kernel forms it, the prior's pentadiagonal matrix summed from its stencils, the
               band of half-bandwidth 8 assembled and solved by LAPACK's banded Cholesky
The distance between (a)'s band and (b)'s is what xas_track_linearise is held to, the distance between the two schedules'
results what xas_track_smooth is held to."""
import numpy as np
import torch
from scipy.linalg import cholesky_banded, cho_solve_banded

LM0, ACCEPT, REJECT, LAMBDA_MAX, STEP_TOL = 1e-3, 0.1, 10.0, 1e12, 1e-5
# A relative cost change below this is a TIE: no arithmetic that sums in another order can be held to the oracle's decision.
TIE_MARGIN = 1e-9
F64 = torch.float64
BW = 8


class Track:
    """One (track, joint).  points [T,V,3], P [T,V,3,4], init [T,4] float32; views [T] uint8 or None; frame [T] integers."""

    def __init__(self, points, P, init, frame, views=None, weighted=False, huber=0.0, acc_w=0.05):
        points, P, init = (np.asarray(t, np.float32) for t in (points, P, init))
        T, V, _ = points.shape
        self.T, self.V, self.init = T, V, init
        self.huber, self.acc_w = float(huber), float(acc_w)
        self.tau = np.asarray(frame, np.float64)
        w = points[..., 2]
        valid = (w > 0) & np.isfinite(w)                                          # [T,V]
        sel = np.zeros(T, np.uint8) if views is None else np.asarray(views, np.uint8)
        bits = np.stack([(sel >> v) & 1 for v in range(V)], 1).astype(bool)
        used = np.where((sel != 0)[:, None], valid & bits, valid)
        X0 = init[:, :3].astype(np.float64)
        cand = (used.sum(1) >= 2) & np.isfinite(X0).all(-1)
        Pd = P.astype(np.float64)
        with np.errstate(all='ignore'):
            h2 = np.einsum('tvj,tj->tv', Pd[:, :, 2, :3], np.nan_to_num(X0)) + Pd[:, :, 2, 3]
        self.data = cand & ~(used & (h2 <= 0)).any(1)                             # [T]
        self.used = used & self.data[:, None]
        self.passed = int(self.data.sum()) < 2
        ti, vi = np.nonzero(self.used)
        self.ot = torch.as_tensor(ti)
        self.oP = torch.as_tensor(Pd[ti, vi])
        self.ouv = torch.as_tensor(points[ti, vi, :2].astype(np.float64))
        self.os = torch.as_tensor(points[ti, vi, 2].astype(np.float64)) if weighted else torch.ones(len(ti), dtype=F64)
        self.nused = self.used.sum(1)
        # the stencils of the prior: centre s = 1 .. T-2
        tau = self.tau
        self.sten = []
        for s in range(1, T - 1):
            h0, h1 = tau[s] - tau[s - 1], tau[s + 1] - tau[s]
            self.sten.append((s, 1.0 / h0, -(1.0 / h0 + 1.0 / h1), 1.0 / h1, 2.0 / (h0 + h1)))
        self.X0 = torch.as_tensor(self.fill(X0))

    def fill(self, X):
        """Gap frames: the line in tau through the nearest data frames, beyond the ends the nearest data frame's point."""
        X = X.copy()
        if self.passed:
            return X
        idx = np.nonzero(self.data)[0]
        for t in np.nonzero(~self.data)[0]:
            left, right = idx[idx < t], idx[idx > t]
            if len(left) and len(right):
                l, r = left[-1], right[0]
                X[t] = X[l] + (X[r] - X[l]) * ((self.tau[t] - self.tau[l]) / (self.tau[r] - self.tau[l]))
            else:
                X[t] = X[left[-1] if len(left) else right[0]]
        return X

    # ---- the definition ----------------------------------------------------------------------------------------------
    def _resid(self, X):
        x = X[self.ot]
        h = torch.einsum('oij,oj->oi', self.oP[:, :, :3], x) + self.oP[:, :, 3]
        return h[:, :2] / h[:, 2:3] - self.ouv, h[:, 2]

    def _robust(self, r):
        rr = (r * r).sum(-1)
        e = self.os * torch.sqrt(rr)
        tail = (e > self.huber) if self.huber > 0 else torch.zeros_like(e, dtype=torch.bool)
        rho = torch.where(tail, 2.0 * self.huber * e - self.huber ** 2, e * e)
        wgt = torch.where(tail, self.huber / torch.where(tail, e, torch.ones_like(e)), torch.ones_like(e)) * self.os ** 2
        return rho, wgt, rr

    def _accel(self, X):
        """q [T-2,3] and ws [T-2]."""
        if self.T < 3:
            return torch.zeros(0, 3, dtype=F64), torch.zeros(0, dtype=F64)
        tau = torch.as_tensor(self.tau)
        h0, h1 = tau[1:-1] - tau[:-2], tau[2:] - tau[1:-1]
        q = (X[2:] - X[1:-1]) / h1[:, None] - (X[1:-1] - X[:-2]) / h0[:, None]
        return q, 2.0 / (h0 + h1)

    def cost(self, X):
        """-> C, behind (bool), sum |r|^2 per frame [T]."""
        r, h2 = self._resid(X)
        rho, _, rr = self._robust(r)
        q, ws = self._accel(X)
        r2 = torch.zeros(self.T, dtype=F64).index_add_(0, self.ot, rr)
        return float(rho.sum()) + self.acc_w * float((ws * (q * q).sum(-1)).sum()), bool((h2 <= 0).any()), r2.numpy()

    # ---- (a) autograd, dense --------------------------------------------------------------------------------------------
    def dense_system(self, X, lam):
        with torch.no_grad():
            _, w, _ = self._robust(self._resid(X)[0])

        def stacked(x):
            r, _ = self._resid(x)
            q, ws = self._accel(x)
            return torch.cat([(torch.sqrt(w)[:, None] * r).reshape(-1), (torch.sqrt(self.acc_w * ws)[:, None] * q).reshape(-1)])
        res = stacked(X)
        J = torch.autograd.functional.jacobian(stacked, X).reshape(len(res), 3 * self.T)
        H = J.T @ J
        return H + lam * torch.diag(torch.diagonal(H)), J.T @ res

    def step_dense(self, X, lam):
        H, g = self.dense_system(X, lam)
        L, info = torch.linalg.cholesky_ex(H)
        if int(info) != 0 or not bool(torch.isfinite(H).all()):
            return None
        return -torch.cholesky_solve(g[:, None], L)[:, 0].reshape(-1, 3)

    # ---- (b) by hand, banded --------------------------------------------------------------------------------------------
    def prior_matrix(self):
        """A [T,3]: A_tt, A_t,t-1, A_t,t-2."""
        A = np.zeros((self.T, 3))
        for s, cm, c0, cp, ws in self.sten:
            c = {s - 1: cm, s: c0, s + 1: cp}
            for t in c:
                A[t, 0] += ws * c[t] * c[t]
                if t - 1 in c:
                    A[t, 1] += ws * c[t] * c[t - 1]
                if t - 2 in c:
                    A[t, 2] += ws * c[t] * c[t - 2]
        return A

    def band_system(self, X, lam):
        """-> band [3T,9] (row i, column i - o; the kernel's layout) and g [3T]."""
        T = self.T
        x = X[self.ot]
        h = torch.einsum('oij,oj->oi', self.oP[:, :, :3], x) + self.oP[:, :, 3]
        uv = h[:, :2] / h[:, 2:3]
        J = (self.oP[:, :2, :3] - uv[:, :, None] * self.oP[:, 2:3, :3]) / h[:, 2, None, None]       # [O,2,3]
        r = uv - self.ouv
        _, w, _ = self._robust(r)
        D = torch.zeros(T, 3, 3, dtype=F64).index_add_(0, self.ot, torch.einsum('o,oci,ocj->oij', w, J, J)).numpy()
        gd = torch.zeros(T, 3, dtype=F64).index_add_(0, self.ot, torch.einsum('o,oci,oc->oi', w, J, r)).numpy()
        A = self.prior_matrix()
        Xn = X.numpy()
        g = gd.copy()
        for s, cm, c0, cp, ws in self.sten:
            q = cp * (Xn[s + 1] - Xn[s]) - cm * (Xn[s] - Xn[s - 1])
            for t, c in ((s - 1, cm), (s, c0), (s + 1, cp)):
                g[t] += self.acc_w * ws * c * q
        band = np.zeros((3 * T, BW + 1))
        for t in range(T):
            full = D[t] + self.acc_w * A[t, 0] * np.eye(3)
            for c in range(3):
                i = 3 * t + c
                band[i, 0] = full[c, c] * (1.0 + lam)
                for o in range(1, c + 1):
                    band[i, o] = full[c, c - o]
                if t >= 1:
                    band[i, 3] = self.acc_w * A[t, 1]
                if t >= 2:
                    band[i, 6] = self.acc_w * A[t, 2]
        return band, g.reshape(-1)

    def step_band(self, X, lam):
        band, g = self.band_system(X, lam)
        if not np.isfinite(band).all():
            return None
        ab = np.zeros((BW + 1, 3 * self.T))                             # LAPACK lower form: ab[o, j] = a[j + o, j]
        for o in range(min(BW + 1, 3 * self.T)):
            ab[o, :3 * self.T - o] = band[o:, o]
        try:
            c = cholesky_banded(ab, lower=True)
        except np.linalg.LinAlgError:
            return None
        return torch.as_tensor(-cho_solve_banded((c, True), g)).reshape(-1, 3)

    @staticmethod
    def band_of(H):
        n = H.shape[0]
        band = np.zeros((n, BW + 1))
        for o in range(min(BW + 1, n)):
            band[o:, o] = np.diagonal(np.asarray(H), -o)
        return band

    # ---- the schedule ---------------------------------------------------------------------------------------------------
    def lm(self, step, max_iter, forced=None):
        """`forced` {trial: accept?} overrules the comparison at those trials; `ties` lists the trials whose relative cost
        change was under TIE_MARGIN."""
        forced = forced or {}
        out = self.init.copy()
        res = {'status': 2, 'trials': 0, 'cost': [0.0, 0.0], 'decisions': [], 'natural': [], 'margins': [], 'ties': [],
               'invalid': False, 'frame_status': np.full(self.T, 2, np.uint8), 'resid': np.full((self.T, 2), np.nan)}
        if self.passed:
            res.update(X=self.init[:, :3].astype(np.float64), out=out)
            return res
        X, lam = self.X0.clone(), LM0
        C, _, r2 = self.cost(X)
        n = np.maximum(self.nused, 1)
        res['resid'][self.data, 0] = np.sqrt(r2 / n)[self.data]
        res['cost'][0] = C
        res['status'] = 1
        for it in range(max_iter):
            res['trials'] += 1
            d, acc = step(X, lam), False
            bad, Ct = True, np.nan
            if d is not None:
                Ct, bad, r2t = self.cost(X + d)
                acc = (not bad) and Ct < C
                res['margins'].append(abs(Ct - C) / abs(C) if np.isfinite(Ct) and C != 0 else np.inf)
                if not bad and res['margins'][-1] < TIE_MARGIN:
                    res['ties'].append(it)
            else:
                res['margins'].append(np.inf)
            res['natural'].append(bool(acc))
            if it in forced and forced[it] != acc:
                if forced[it] and (d is None or bad or not np.isfinite(Ct)):
                    res['invalid'] = True
                    break
                acc = forced[it]
            res['decisions'].append(bool(acc))
            if acc:
                X, C, r2, lam = X + d, Ct, r2t, lam * ACCEPT
                if float(d.norm(dim=-1).max()) < STEP_TOL:
                    res['status'] = 0
                    break
            else:
                lam *= REJECT
                if lam > LAMBDA_MAX:
                    break
        res['cost'][1] = C
        res['resid'][self.data, 1] = np.sqrt(r2 / n)[self.data]
        res['frame_status'] = np.where(self.data, 0, 1).astype(np.uint8)
        out[:, :3] = X.numpy().astype(np.float32)
        res.update(X=X.numpy(), out=out)
        return res


def make_track(case, s, k):
    m = np.nonzero(case['track'] == s)[0]
    m = m[np.argsort(case['frame'][m], kind='stable')]
    return Track(case['points'][m][:, :, k], case['P'][m], case['init'][m][:, k], case['frame'][m],
                 None if case['views'] is None else case['views'][m][:, k], case['weighted'], case['huber'], case['acc_w']), m


def follow(trk, decisions, max_iter):
    """The oracle's two schedules made to take `decisions` (what another implementation decided, trial by trial) -> (dense,
    band) results.  Raises if a decision differs from the oracle's own at a trial that is no TIE."""
    forced = dict(enumerate(decisions))
    res = [trk.lm(step, max_iter, forced) for step in (trk.step_dense, trk.step_band)]
    for r in res:
        if r['invalid']:
            raise AssertionError('a forced accept had no trial state: %s' % (decisions,))
        for t, (mine, theirs) in enumerate(zip(r['natural'], decisions)):
            if mine != theirs and t not in r['ties']:
                raise AssertionError('trial %d decided %s where the oracle decides %s with margin %.2e' % (
                    t, theirs, mine, r['margins'][t]))
    return res


def distance(a, b):
    """Largest distance between two results, relative to the largest |coordinate| of the points (mm)."""
    scale = max(1.0, float(np.nanmax(np.abs(b['X'])))) if np.isfinite(b['X']).any() else 1.0
    d = np.abs(a['X'] - b['X'])
    return (float(np.nanmax(d)) if np.isfinite(d).any() else 0.0) / scale, scale
