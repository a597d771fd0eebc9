"""float64 restatement of xas_track_skeleton_smooth (include/xas_hip.h) for one track, in torch / numpy on the CPU.  It does
not import the library.  The data terms, the frame rules and the prior are those of _track_anchor_oracle.AnchorTrack, one per
joint, taken by import; this file adds the bones and the coupled solve.  The schedule is written once (`lm`) and driven by two
ways of solving a trial over the unknowns 3K t + 3k + c:
  step_dense   (a) one matrix over all unknowns: per joint AnchorTrack's stacked residuals and anchor term with their
               autograd Jacobians, the bones' Jacobian from torch.autograd on the stacked residuals sqrt(bone_w) e, summed into
               the band that holds all of it; then dense, numpy.linalg.cholesky and two numpy.linalg.solve.  Above DENSE_MAX
               unknowns the band goes to LAPACK's banded Cholesky as it is: dense solves of 7020 unknowns would take the
               planted case to minutes
  step_block   (b) by hand as the kernel forms it: per joint AnchorTrack's band, u u^T per bone, then the block-pentadiagonal
               Cholesky with its forward and back substitution over the frames
A fixed joint keeps identity rows and a zero right-hand side in both."""
import numpy as np
import torch
from scipy.linalg import cholesky_banded, cho_solve_banded

import _track_anchor_oracle as ao
import _track_oracle as tk

F64 = torch.float64
SHORT = 1e-9
DENSE_MAX = 2500


class SkeletonTrack:
    """Track s of a case of _track_skeleton_inputs."""

    def __init__(self, case, s, **over):
        self.joints = [ao.make_track(case, s, k, **over)[0] for k in range(case['K'])]
        self.rows = ao.make_track(case, s, 0)[1]
        self.T, self.K = self.joints[0].T, case['K']
        self.n = 3 * self.K
        self.free = np.array([not j.passed for j in self.joints])
        self.bones = np.asarray(case['bones'], np.int64).reshape(-1, 2)
        self.length = np.asarray(case['length'], np.float32)[s].astype(np.float64).reshape(-1)
        self.bone_w, self.acc_w = float(case['bone_w']), float(case['acc_w'])
        with np.errstate(all='ignore'):
            ok = np.isfinite(self.length) & (self.length > 0)
        self.act = np.array([bool(ok[b] and self.free[i] and self.free[j]) for b, (i, j) in enumerate(self.bones)], bool).reshape(-1)
        self.ba, self.bb = torch.as_tensor(self.bones[self.act, 0]), torch.as_tensor(self.bones[self.act, 1])
        self.bl = torch.as_tensor(self.length[self.act])
        self.init = np.stack([j.init for j in self.joints], 1)                                       # [T,K,4]
        self.X0 = torch.stack([j.X0 for j in self.joints], 1)                                        # [T,K,3]
        self.data = np.stack([j.data for j in self.joints], 1)
        self.nused = np.stack([j.nused for j in self.joints], 1)
        self.terms = sum(len(j.ot) + len(j.sten) + len(j.at) for j, f in zip(self.joints, self.free) if f) + self.T * int(self.act.sum())

    # ---- the definition --------------------------------------------------------------------------------------------------
    def bone_e(self, X):
        """e [T, active bones] and |d|."""
        if not len(self.ba):
            return torch.zeros(self.T, 0, dtype=F64), torch.zeros(self.T, 0, dtype=F64)
        ln = torch.linalg.vector_norm(X[:, self.ba] - X[:, self.bb], dim=-1)
        return ln - self.bl, ln

    def bone_all(self, X):
        """e [T,Bn] with NaN where the bone is not active."""
        e = np.full((self.T, len(self.bones)), np.nan)
        e[:, self.act] = self.bone_e(torch.as_tensor(X))[0].numpy()
        return e

    def cost(self, X):
        """-> C, behind, sum |r|^2 per frame and joint [T,K]."""
        C, behind, r2 = 0.0, False, np.zeros((self.T, self.K))
        for k in np.nonzero(self.free)[0]:
            c, b, r = self.joints[k].cost(X[:, k])
            C, behind, r2[:, k] = C + c, behind or b, r
        e, _ = self.bone_e(X)
        return C + self.bone_w * float((e * e).sum()), behind, r2

    def index(self, k):
        return (np.arange(self.T)[:, None] * self.n + 3 * k + np.arange(3)).reshape(-1)

    # ---- (a) autograd, one matrix --------------------------------------------------------------------------------------------
    def joint_system(self, k, X):
        """AnchorTrack.dense_system of joint k without damping, with the Jacobians taken in one vectorised sweep each."""
        j = self.joints[k]
        jac = lambda f, x: torch.autograd.functional.jacobian(f, x, vectorize=True)
        with torch.no_grad():
            _, w, _ = j._robust(j._resid(X)[0])
            psi = j._anchor(X)[1]

        def stacked(x):
            r, _ = j._resid(x)
            q, ws = j._accel(x)
            return torch.cat([(torch.sqrt(w)[:, None] * r).reshape(-1), (torch.sqrt(j.acc_w * ws)[:, None] * q).reshape(-1)])

        def irls(x):
            e = x[j.at] - j.A
            return (psi * torch.einsum('ni,nij,nj->n', e, j.W, e)).sum()
        n = 3 * self.T
        res = stacked(X)
        J = jac(stacked, X).reshape(len(res), n)
        H, g = J.T @ J, J.T @ res
        if len(j.at):
            H = H + 0.5 * torch.autograd.functional.hessian(irls, X, vectorize=True).reshape(n, n)
            g = g + 0.5 * jac(irls, X).reshape(n)
        return H.numpy(), g.numpy()

    def dense_system(self, X, lam):
        """-> the lower band ab [3n, T n] of H + lam diag H (ab[o, j] = H[j + o, j]: every entry of H, nothing of it lies
        outside) and g [T n]."""
        N, bw = self.T * self.n, 3 * self.n - 1
        ab, g = np.zeros((bw + 1, N)), np.zeros(N)

        def add(rows, cols, vals):
            low = rows >= cols
            o = rows[low] - cols[low]
            assert not np.abs(vals[low][o > bw]).any()
            np.add.at(ab, (o[o <= bw], cols[low][o <= bw]), vals[low][o <= bw])
        for k in range(self.K):
            idx = self.index(k)
            if not self.free[k]:
                ab[0, idx] = 1.0
                continue
            Hk, gk = self.joint_system(k, X[:, k])
            I, J = np.meshgrid(idx, idx, indexing='ij')
            add(I.reshape(-1), J.reshape(-1), Hk.reshape(-1))
            g[idx] += gk
        if len(self.ba) and self.bone_w > 0:
            Xf = torch.where(torch.as_tensor(self.free)[None, :, None], X, torch.zeros_like(X))      # a fixed joint may be NaN
            stacked = lambda x: (np.sqrt(self.bone_w) * self.bone_e(x)[0]).reshape(-1)
            e, ln = self.bone_e(Xf)
            J = torch.autograd.functional.jacobian(stacked, Xf, vectorize=True).reshape(self.T, -1, self.T, self.n)
            J = torch.where((ln < SHORT)[:, :, None, None], torch.zeros_like(J), J).numpy()
            Jt = J[np.arange(self.T), :, np.arange(self.T)]                                          # [T,nb,n]: a bone couples one frame
            assert np.count_nonzero(J) == np.count_nonzero(Jt)
            Hb = np.einsum('tbi,tbj->tij', Jt, Jt)
            base = (np.arange(self.T) * self.n)[:, None, None]
            I, Jc = np.arange(self.n)[None, :, None] + base, np.arange(self.n)[None, None, :] + base
            add(np.broadcast_to(I, Hb.shape).reshape(-1), np.broadcast_to(Jc, Hb.shape).reshape(-1), Hb.reshape(-1))
            g += np.einsum('tbi,tb->ti', Jt, np.sqrt(self.bone_w) * e.numpy()).reshape(-1)
        ab[0] *= 1.0 + lam
        return ab, g

    @staticmethod
    def full(ab):
        """The band as the symmetric dense matrix."""
        N = ab.shape[1]
        H = np.zeros((N, N))
        for o in range(min(ab.shape[0], N)):
            H += np.diag(ab[o, :N - o], -o)
        return H + np.tril(H, -1).T

    def step_dense(self, X, lam):
        ab, g = self.dense_system(X, lam)
        if not np.isfinite(ab).all():
            return None
        try:
            if len(g) <= DENSE_MAX:
                L = np.linalg.cholesky(self.full(ab))
                d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            else:
                d = -cho_solve_banded((cholesky_banded(ab[:min(ab.shape[0], len(g))], lower=True), True), g)
        except np.linalg.LinAlgError:
            return None
        return torch.as_tensor(d).reshape(self.T, self.K, 3)

    # ---- (b) by hand, in blocks ------------------------------------------------------------------------------------------------
    def block_system(self, X, lam):
        """-> hdiag [T,n,n] (H + lam diag H, a fixed joint's rows as identity rows), hoff [T,2], g [T,n]."""
        T, n = self.T, self.n
        Hd, g = np.zeros((T, n, n)), np.zeros((T, n))
        A = self.joints[0].prior_matrix()
        hoff = np.zeros((T, 2))
        hoff[1:, 0], hoff[2:, 1] = self.acc_w * A[1:, 1], self.acc_w * A[2:, 2]
        for k in range(self.K):
            sl = slice(3 * k, 3 * k + 3)
            if not self.free[k]:
                Hd[:, sl, sl] = np.eye(3)
                continue
            band, gk = self.joints[k].band_system(X[:, k], 0.0)
            band = band.reshape(T, 3, -1)
            for c in range(3):
                for o in range(c + 1):
                    Hd[:, 3 * k + c, 3 * k + c - o] = band[:, c, o]
                    Hd[:, 3 * k + c - o, 3 * k + c] = band[:, c, o]
            g[:, sl] = gk.reshape(T, 3)
        Xn = X.numpy()
        for b in np.nonzero(self.act)[0]:
            i, j = self.bones[b]
            d = Xn[:, i] - Xn[:, j]
            ln = np.linalg.norm(d, axis=-1)
            row = ln >= SHORT
            u = np.where(row[:, None], d / np.where(row, ln, 1.0)[:, None], 0.0)
            e = ln - self.length[b]
            uu = self.bone_w * u[:, :, None] * u[:, None, :]
            si, sj = slice(3 * i, 3 * i + 3), slice(3 * j, 3 * j + 3)
            Hd[:, si, si] += uu; Hd[:, sj, sj] += uu; Hd[:, si, sj] -= uu; Hd[:, sj, si] -= uu
            g[:, si] += self.bone_w * u * e[:, None]; g[:, sj] -= self.bone_w * u * e[:, None]
        Hd = Hd + lam * Hd * np.eye(n)
        return Hd, hoff, g

    def step_block(self, X, lam):
        Hd, hoff, g = self.block_system(X, lam)
        if not np.isfinite(Hd).all():
            return None
        T, n = self.T, self.n
        P = np.diag(np.repeat(self.free, 3).astype(np.float64))
        L0, L1, L2, y = np.zeros((T, n, n)), np.zeros((T, n, n)), np.zeros((T, n, n)), np.zeros((T, n))
        try:
            for t in range(T):
                if t >= 2:
                    L2[t] = np.linalg.solve(L0[t - 2], hoff[t, 1] * P).T
                if t >= 1:
                    L1[t] = np.linalg.solve(L0[t - 1], (hoff[t, 0] * P - L2[t] @ L1[t - 1].T).T).T
                L0[t] = np.linalg.cholesky(Hd[t] - L1[t] @ L1[t].T - L2[t] @ L2[t].T)
                rhs = -g[t] - (L1[t] @ y[t - 1] if t >= 1 else 0.0) - (L2[t] @ y[t - 2] if t >= 2 else 0.0)
                y[t] = np.linalg.solve(L0[t], rhs)
        except np.linalg.LinAlgError:
            return None
        d = np.zeros((T, n))
        for t in range(T - 1, -1, -1):
            rhs = y[t] - (L1[t + 1].T @ d[t + 1] if t + 1 < T else 0.0) - (L2[t + 2].T @ d[t + 2] if t + 2 < T else 0.0)
            d[t] = np.linalg.solve(L0[t].T, rhs)
        return torch.as_tensor(d).reshape(T, self.K, 3)

    def residual_of(self, d, lam):
        """Largest |(H + lam diag H) d + g| of the by-hand system at the start, relative to the largest |g|."""
        Hd, hoff, g = self.block_system(self.X0, lam)
        d = np.asarray(d, np.float64).reshape(self.T, self.n)
        P = np.repeat(self.free, 3).astype(np.float64)
        r = np.einsum('tij,tj->ti', Hd, d) + g
        r[1:] += hoff[1:, :1] * P * d[:-1]; r[:-1] += hoff[1:, :1] * P * d[1:]
        r[2:] += hoff[2:, 1:] * P * d[:-2]; r[:-2] += hoff[2:, 1:] * P * d[2:]
        return float(np.abs(r).max() / max(np.abs(g).max(), 1e-300))

    # ---- the schedule: _track_oracle.Track.lm's, over the whole track ---------------------------------------------------------
    def lm(self, step, max_iter, forced=None):
        forced = forced or {}
        T, K = self.T, self.K
        out = self.init.copy()
        res = {'status': 2, 'trials': 0, 'cost': [0.0, 0.0], 'decisions': [], 'natural': [], 'margins': [], 'ties': [], 'invalid': False,
               'frame_status': np.full((T, K), 2, np.uint8), 'resid': np.full((T, K, 2), np.nan),
               'bone': np.full((T, len(self.bones), 2), np.nan)}
        if not self.free.any():
            res.update(X=self.init[..., :3].astype(np.float64), out=out)
            return res
        X, lam = self.X0.clone(), tk.LM0
        C, _, r2 = self.cost(X)
        nv = np.maximum(self.nused, 1)
        shown = self.free[None, :] & self.data & (self.nused > 0)
        res['resid'][shown, 0] = np.sqrt(r2 / nv)[shown]
        res['bone'][..., 0] = self.bone_all(X)
        res['cost'][0], res['status'] = C, 1
        for it in range(max_iter):
            res['trials'] += 1
            d, acc = step(X, lam), False
            bad, Ct = True, np.nan
            if d is not None:
                d = torch.where(torch.as_tensor(self.free)[None, :, None], d, torch.zeros_like(d))
                Ct, bad, r2t = self.cost(X + d)
                acc = (not bad) and Ct < C
                res['margins'].append(abs(Ct - C) / abs(C) if np.isfinite(Ct) and C != 0 else np.inf)
                if not bad and res['margins'][-1] < tk.TIE_MARGIN:
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
                X, C, r2, lam = X + d, Ct, r2t, lam * tk.ACCEPT
                if float(d.norm(dim=-1).max()) < tk.STEP_TOL:
                    res['status'] = 0
                    break
            else:
                lam *= tk.REJECT
                if lam > tk.LAMBDA_MAX:
                    break
        res['cost'][1] = C
        res['resid'][shown, 1] = np.sqrt(r2 / nv)[shown]
        res['bone'][..., 1] = self.bone_all(X)
        res['frame_status'] = np.where(self.free[None, :], np.where(self.data, 0, 1), 2).astype(np.uint8)
        Xn = X.numpy()
        out[:, self.free, :3] = Xn[:, self.free].astype(np.float32)
        res.update(X=np.where(self.free[None, :, None], Xn, np.nan), out=out)
        return res


def follow(trk, decisions, max_iter):
    """_track_oracle.follow for a SkeletonTrack: both schedules made to take `decisions` -> (dense, block) results."""
    forced = dict(enumerate(decisions))
    res = [trk.lm(step, max_iter, forced) for step in (trk.step_dense, trk.step_block)]
    for r in res:
        if r['invalid']:
            raise AssertionError('a forced accept had no trial state: %s' % (decisions,))
        for t, (mine, theirs) in enumerate(zip(r['natural'], decisions)):
            if mine != theirs and t not in r['ties']:
                raise AssertionError('trial %d decided %s where the oracle decides %s with margin %.2e' % (t, theirs, mine, r['margins'][t]))
    return res
