"""float64 restatement of xas_multiview_consistency_fwd / _bwd (include/xas_hip.h), numpy only: the forward with the header's
validity and pass-through rules, the analytic gradient through the DLT's null vector, every joint's eigenvalue ratio
lambda_1 / lambda_0 and whether its hypothesis choice is decidable.  `torch_loss` states the same loss in plain torch ops with
torch.linalg.eigh, in any dtype: in float64 its autograd checks the analytic gradient, in float32 it is the yardstick of
tests/test_gpu_multiview.py."""
import numpy as np

DECIDABLE_REL = 1e-4         # best and second-best squared distance of a view's hypotheses differ by more than this, relative
RATIO_MIN = 50.0             # lambda_1 / lambda_0 of every compared joint


def image_points(kps_xy, ti, S):
    """(u, v) [B,V,K,2] and the inverse crop affines [B,V,2,2], float64."""
    A = ti[..., :2].astype(np.float64)
    inv = np.linalg.inv(A)
    p = (kps_xy.astype(np.float64) + 1.0) / 2.0 * (S - 1.0) - ti[..., None, :, 2].astype(np.float64)
    return np.einsum('bvij,bvkj->bvki', inv, p), inv


MIN_GAP = 1e-10              # xas_hip.h XAS_MV_MIN_GAP


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def fma32(a, b, c):
    """float32 fused multiply-add: the product of two float32 numbers is exact in float64, so one float64 addition and one
    rounding to float32 is the fused result (but for a double rounding on an exact tie of the float64 sum)."""
    return f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def image_points_f32(kps_xy, ti, S):
    """image_points with the header's float32 patch stage, rounding for rounding: -> ((u, v) [B,V,K,2] float32 as float64, the
    float32 inverse affines [B,V,2,2] as float64)."""
    a00, a01, a10, a11 = (ti[..., 0, 0], ti[..., 0, 1], ti[..., 1, 0], ti[..., 1, 1])
    with np.errstate(all='ignore'):
        det = f32(a00 * a11) - f32(a01 * a10)                         # float32 arrays: every operation rounds once
        i00, i01, i10, i11 = (a11 / det)[..., None], (-a01 / det)[..., None], (-a10 / det)[..., None], (a00 / det)[..., None]
        p0 = (kps_xy[..., 0] + np.float32(1)) * np.float32(0.5) * np.float32(S - 1.0)
        p1 = (kps_xy[..., 1] + np.float32(1)) * np.float32(0.5) * np.float32(S - 1.0)
        du, dv = p0 - ti[..., None, 0, 2], p1 - ti[..., None, 1, 2]
        u, v = fma32(i00 + 0 * du, du, i01 * dv), fma32(i11 + 0 * dv, dv, i10 * du)
    inv = np.stack([np.stack([i00[..., 0], i01[..., 0]], -1), np.stack([i10[..., 0], i11[..., 0]], -1)], -2)
    return np.stack([u, v], -1).astype(np.float64), inv.astype(np.float64)


def rho(e, huber):
    """(rho(e), psi(e)): the square, or Huber's with its IRLS weight."""
    if huber > 0.0 and e > huber:
        return 2.0 * huber * e - huber * huber, huber / e
    return e * e, 1.0


def joint(uv, Pm, c, world, huber, eig=None, rows32=False):
    """One joint: uv [V,2], Pm [V,3,4], c [V] weights, world [V,Hy,3].  -> dict; `passed` joints carry zeros and NaN.
    `eig` = (eigenvalues [4] ascending, eigenvectors [4,4] in columns) of the Gram matrix from elsewhere, in place of numpy's.
    `rows32`: the DLT's rows are formed in float32 as dlt_view_gram forms them (uv and c must then hold float32 numbers)."""
    V, Hy = world.shape[:2]
    F = [v for v in range(V) if np.isfinite(c[v]) and c[v] > 0]
    out = dict(passed=True, reproj=0.0, depth=0.0, xyz=np.full(3, np.nan), hsel=np.zeros(V, np.int32), ratio=np.nan,
               decidable=True, F=F, gap=False)
    if len(F) < 2:
        return out
    rows = []
    for v in F:
        for t in range(2):
            if rows32:
                with np.errstate(all='ignore'):
                    rows.append(f32(c[v]) * fma32(np.full(4, uv[v, t], np.float32), f32(Pm[v, 2]), -f32(Pm[v, t])))
            else:
                rows.append(c[v] * (uv[v, t] * Pm[v, 2] - Pm[v, t]))
    A = np.array(rows, np.float64)
    G = A.T @ A
    if not np.isfinite(G).all():
        return out
    lam, vec = np.linalg.eigh(G) if eig is None else eig
    x = vec[:, 0]
    with np.errstate(all='ignore'):
        X = x[:3] / x[3]
        out['ratio'] = lam[1] / lam[0] if lam[0] > 0 else np.inf
    if not np.isfinite(X).all():
        return out
    h = np.array([Pm[v] @ np.append(X, 1.0) for v in range(V)])
    if any(h[v, 2] <= 0 for v in F):
        return out
    d2 = ((world - X) ** 2).sum(-1)                                    # [V,Hy]
    with np.errstate(invalid='ignore'):
        hsel = np.array([int(np.nanargmin(d2[v])) if np.isfinite(d2[v]).any() else 0 for v in range(V)], np.int32)
    if Hy > 1:
        s = np.sort(d2, axis=1)
        out['decidable'] = bool(((s[:, 1] - s[:, 0]) > DECIDABLE_REL * s[:, 1]).all())
    r = h[:, :2] / h[:, 2:3] - uv
    e = np.sqrt((r ** 2).sum(-1))
    n = len(F)
    out.update(passed=False, xyz=X, hsel=hsel, lam=lam, vec=vec, h=h, r=r, e=e, n=n, gap=lam[1] - lam[0] > MIN_GAP * lam[3],
               reproj=sum(rho(e[v], huber)[0] for v in F) / n, depth=sum(d2[v, hsel[v]] for v in F) / n)
    return out


def joint_grad(o, uv, Pm, c, world, huber, g_reproj, g_depth, detach):
    """The header's backward pass of one solved joint -> (d / d uv [V,2], d / d world [V,Hy,3])."""
    V = world.shape[0]
    g_uv, g_w = np.zeros((V, 2)), np.zeros(world.shape)
    a, d = g_reproj / o['n'], g_depth / o['n']
    X, gX = o['xyz'], np.zeros(3)
    for v in o['F']:
        psi = rho(o['e'][v], huber)[1]
        g_uv[v] = -2.0 * a * psi * o['r'][v]
        diff = world[v, o['hsel'][v]] - X
        g_w[v, o['hsel'][v]] = 2.0 * d * diff
        h = o['h'][v]
        J = (Pm[v, :2, :3] - (h[:2] / h[2])[:, None] * Pm[v, 2, :3]) / h[2]
        gX += 2.0 * a * psi * (J.T @ o['r'][v]) - 2.0 * d * diff
    if not detach and o['gap']:
        lam, vec = o['lam'], o['vec']
        x = vec[:, 0]
        gx = np.append(gX / x[3], -(gX @ x[:3]) / x[3] ** 2)
        gG = np.zeros((4, 4))
        for j in range(1, 4):
            m = np.outer(vec[:, j], x)
            gG += (vec[:, j] @ gx) / (lam[0] - lam[j]) * (m + m.T) / 2.0
        for v in o['F']:
            for t in range(2):
                g_uv[v, t] += 2.0 * c[v] ** 2 * (uv[v, t] * Pm[v, 2] - Pm[v, t]) @ gG @ Pm[v, 2]
    return g_uv, g_w


def run(case, g_reproj=None, g_depth=None, detach=False, eig=None, as_kernel=False):
    """case: dict of kps_xy [B,V,K,2], ti [B,V,2,3], world [B,V,Hy,K,3], P [B,V,3,4], weight [B,V,K] or None, S, huber.
    -> dict of float64 arrays: reproj, depth [B,K], xyz [B,K,3], hsel [B,V,K], status, ratio, decidable, gap (the backward pass differentiates through X: MIN_GAP) [B,K], and with upstream
    gradients grad_kps_xy [B,V,K,2], grad_world [B,V,Hy,K,3].  `eig` = (lam [B,K,4], vec [B,K,4,4]): see joint().
    `as_kernel`: the two float32 stages of the header - the patch stage and the DLT's rows - are rounded as the kernels round
    them, and everything else stays float64: what the kernels compute, but for their double-precision rounding and the one
    rounding of every output."""
    kps, ti, world, P = case['kps_xy'], case['ti'], case['world'].astype(np.float64), case['P'].astype(np.float64)
    B, V, K, _ = kps.shape
    S, huber = float(case['S']), float(case['huber'])
    w = np.ones((B, V, K)) if case['weight'] is None else case['weight'].astype(np.float64)
    uv, inv = image_points_f32(kps, ti, S) if as_kernel else image_points(kps, ti, S)
    res = dict(reproj=np.zeros((B, K)), depth=np.zeros((B, K)), xyz=np.full((B, K, 3), np.nan), hsel=np.zeros((B, V, K), np.int32),
               status=np.zeros((B, K), np.uint8), ratio=np.full((B, K), np.nan), decidable=np.ones((B, K), bool),
               gap=np.zeros((B, K), bool))
    if g_reproj is not None:
        res['grad_kps_xy'], res['grad_world'] = np.zeros((B, V, K, 2)), np.zeros(world.shape)
    for b in range(B):
        for k in range(K):
            args = (uv[b, :, k], P[b], w[b, :, k], world[b, :, :, k])
            o = joint(*args, huber, None if eig is None else (eig[0][b, k], eig[1][b, k]), rows32=as_kernel)
            res['reproj'][b, k], res['depth'][b, k], res['xyz'][b, k] = o['reproj'], o['depth'], o['xyz']
            res['hsel'][b, :, k], res['status'][b, k] = o['hsel'], 2 if o['passed'] else 0
            res['ratio'][b, k], res['decidable'][b, k], res['gap'][b, k] = o['ratio'], o['decidable'], o['gap']
            if g_reproj is not None and not o['passed']:
                g_uv, g_w = joint_grad(o, *args, huber, float(g_reproj[b, k]), float(g_depth[b, k]), detach)
                res['grad_kps_xy'][b, :, k] = np.einsum('vji,vj->vi', inv[b], g_uv) * (S - 1.0) / 2.0     # transposed inverse affine
                res['grad_world'][b, :, :, k] = g_w
    return res


def objective(case, g_reproj, g_depth, hsel=None):
    """sum(g_reproj * reproj + g_depth * depth) in float64, for central differences (X follows the inputs)."""
    r = run(case)
    return float((g_reproj * r['reproj'] + g_depth * r['depth']).sum())


def torch_loss(case, dtype, status, g_reproj, g_depth, detach=False):
    """The same loss in plain torch ops with torch.linalg.eigh, on the CPU in `dtype`; joints with status != 0 (the oracle's) are
    left out of the objective.  -> dict of float64 numpy arrays like run(): reproj, depth, xyz, grad_kps_xy, grad_world (of the
    solved joints; the others' entries are meaningless), and the eigensystems it worked with, lam [B,K,4] and vec [B,K,4,4]."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    kps, world = t(case['kps_xy']).requires_grad_(), t(case['world']).requires_grad_()
    ti, P = t(case['ti']), t(case['P'])
    B, V, K, _ = kps.shape
    S = float(case['S'])
    wn = np.ones((B, V, K), np.float32) if case['weight'] is None else case['weight']
    ok = torch.from_numpy(np.isfinite(wn) & (wn > 0))
    c = torch.where(ok, t(np.nan_to_num(wn, nan=0.0, posinf=0.0, neginf=0.0)), torch.zeros((), dtype=dtype))
    n = ok.sum(1).clamp(min=1).to(dtype)                                                       # [B,K]
    p = (kps + 1.0) / 2.0 * (S - 1.0) - ti[:, :, None, :, 2]
    uv = torch.einsum('bvij,bvkj->bvki', torch.linalg.inv(ti[..., :2]), p)
    P0, P1, P2 = (P[:, :, None, r, :] for r in range(3))                                       # [B,V,1,4]
    rows = torch.cat([c[..., None] * (uv[..., 0:1] * P2 - P0), c[..., None] * (uv[..., 1:2] * P2 - P1)], dim=1)   # [B,2V,K,4]
    A = rows.permute(0, 2, 1, 3)
    G = A.transpose(-1, -2) @ A
    G = torch.where(torch.isfinite(G).all(-1).all(-1)[..., None, None], G, torch.eye(4, dtype=dtype))     # eigh refuses NaN
    lam, vec = torch.linalg.eigh(G)
    x = vec[..., 0]
    X = x[..., :3] / x[..., 3:4]                                                               # [B,K,3]
    if detach:
        X = X.detach()
    Xh = torch.cat([X, torch.ones_like(X[..., :1])], -1)
    h = torch.einsum('bvij,bkj->bvki', P, Xh)
    r = h[..., :2] / h[..., 2:3] - uv
    r2 = (r ** 2).sum(-1)
    hub = float(case['huber'])
    if hub > 0:
        e = torch.sqrt(r2.clamp(min=1e-30))
        r2 = torch.where(e > hub, 2.0 * hub * e - hub * hub, r2)
    reproj = torch.where(ok, r2, torch.zeros((), dtype=dtype)).sum(1) / n
    d2 = ((world - X[:, None, None]) ** 2).sum(-1)                                             # [B,V,Hy,K]
    hsel = torch.nan_to_num(d2.detach(), nan=float('inf')).argmin(2, keepdim=True)
    depth = torch.where(ok, d2.gather(2, hsel)[:, :, 0], torch.zeros((), dtype=dtype)).sum(1) / n
    solved = torch.from_numpy(status == 0)
    obj = (t(g_reproj) * reproj + t(g_depth) * depth)[solved].sum()
    gk, gw = torch.autograd.grad(obj, [kps, world], allow_unused=True) if solved.any() else (None, None)
    z = lambda g, like: np.zeros(like.shape) if g is None else g.double().numpy()
    return dict(reproj=reproj.detach().double().numpy(), depth=depth.detach().double().numpy(), xyz=X.detach().double().numpy(),
                hsel=hsel[:, :, 0].numpy(), grad_kps_xy=z(gk, kps), grad_world=z(gw, world), lam=lam.detach().double().numpy(),
                vec=vec.detach().double().numpy())
