"""Oracle of xas_smpl_fit (include/xas_hip.h): the same residual in float64 torch on oracle.smpl, its Jacobian by
torch.autograd, and a Levenberg-Marquardt that follows the header's schedule step for step.  CPU, one sample at a time.
TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

from oracle.smpl import smpl_lbs, smpl_to_h36m

STEP_TOL = 1e-7                 # XAS_SMPLFIT_STEP_TOL
N, ROWS = 85, 133


def model_arrays(a):
    """dict of _smplfit_inputs.arrays -> float64 tensors of the fp32 values."""
    t = lambda k: torch.as_tensor(np.asarray(a[k], dtype=np.float32)).double()
    return dict(vt=t('v_template').reshape(1, -1, 3), sd=t('shapedirs'), pd=t('posedirs'), jr=t('J_regressor'), w=t('weights'),
                hr=t('h36m_regressor'), parents=tuple(a.get('kintree_parents', ())) or None)


def expmap(om):
    """[3] -> [3,3]: I + sin(th) K + (1 - cos(th)) K^2 (xas_amd.pseudo._rodrigues); its series below th^2 = 1e-16."""
    z = torch.zeros((), dtype=om.dtype)
    cross = lambda k: torch.stack([z, -k[2], k[1], k[2], z, -k[0], -k[1], k[0], z]).view(3, 3)
    th2 = (om * om).sum()
    if float(th2) < 1e-16:
        K = cross(om)
        return torch.eye(3, dtype=om.dtype) + K + 0.5 * (K @ K)
    th = th2.sqrt()
    K = cross(om / th)
    return torch.eye(3, dtype=om.dtype) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)


def joints(x, m, center_idx=0):
    """x [85] = (omega, t, theta, beta) -> Y [18,3] world mm."""
    pose = torch.cat([x.new_zeros(3), x[6:75]]).unsqueeze(0)
    kw = {} if m['parents'] is None else {'parents': m['parents']}
    verts, _ = smpl_lbs(pose, x[75:85].unsqueeze(0), m['vt'], m['sd'], m['pd'], m['jr'], m['w'], center_idx=center_idx, **kw)
    j = smpl_to_h36m(verts, m['hr'])[0] * 1000.0
    return j @ expmap(x[:3]).T + x[3:6]


def residual(x, m, tgt, w, wp, ws):
    """[133]: 54 joint rows, 69 pose-prior rows, 10 shape-prior rows.  A joint with w <= 0 (or NaN) gives zeros and its
    target is not read."""
    on = w > 0
    sw = torch.where(on, w, torch.zeros_like(w)).sqrt()
    tg = torch.where(on.unsqueeze(1), tgt, torch.zeros_like(tgt))
    rj = (sw.unsqueeze(1) * (joints(x, m) - tg)) * on.unsqueeze(1).to(x.dtype)
    return torch.cat([rj.reshape(-1), (wp ** 0.5) * x[6:75], (ws ** 0.5) * x[75:85]])


def linearise(x, m, tgt, w, wp, ws):
    """-> r [133], J [133,85] (autograd, exact)."""
    x = x.detach().double()
    f = lambda y: residual(y, m, tgt, w, wp, ws)
    J = torch.autograd.functional.jacobian(f, x, vectorize=True)
    return f(x).detach(), J.detach()


def cost_of(r):
    return float((r * r).sum())


def lm(x0, m, tgt, w, wp, ws, max_iters, lambda0=1e-3):
    """The header's loop.  -> dict(x, cost (start, result), iters, status)."""
    x = x0.detach().double().clone()
    usable = int((w > 0).sum())
    r = residual(x, m, tgt, w, wp, ws)
    C = cost_of(r)
    C0 = C
    if usable < 6 or not np.isfinite(C):
        return dict(x=x, cost=(C0, C0), iters=0, status=2)
    st, it, lam = 1, 0, lambda0
    if max_iters > 0:
        r, J = linearise(x, m, tgt, w, wp, ws)
        H, g = J.T @ J, J.T @ r
    while it < max_iters:
        it += 1
        accept = False
        A = H + lam * torch.diag(torch.diagonal(H))
        L, info = torch.linalg.cholesky_ex(A)
        if int(info) == 0:
            d = -torch.cholesky_solve(g.unsqueeze(1), L)[:, 0]
            xt = x + d
            Ct = cost_of(residual(xt, m, tgt, w, wp, ws))
            accept = np.isfinite(Ct) and Ct < C
        if accept:
            x, C, lam = xt, Ct, lam * 0.1
            if float(d.abs().max()) < STEP_TOL:
                st = 0
                break
            r, J = linearise(x, m, tgt, w, wp, ws)
            H, g = J.T @ J, J.T @ r
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return dict(x=x, cost=(C0, C), iters=it, status=st)


def kabsch_init(m, tgt, w):
    """The default start of ops_smplfit.default_init in float64: zero body pose and betas, t = the target pelvis, omega from the
    weighted rigid alignment of the zero-pose joints.  Rounded to fp32, as the kernel receives it."""
    src = joints(torch.zeros(N, dtype=torch.float64), m)
    wn = torch.where(w > 0, w, torch.zeros_like(w))
    wn = wn / wn.sum()
    tg = torch.where((w > 0).unsqueeze(1), tgt, torch.zeros_like(tgt))
    ca, cb = (wn.unsqueeze(1) * src).sum(0), (wn.unsqueeze(1) * tg).sum(0)
    M = torch.einsum('k,ki,kj->ij', wn, tg - cb, src - ca)
    U, _, Vh = torch.linalg.svd(M)
    D = torch.diag(torch.tensor([1.0, 1.0, float(torch.sign(torch.linalg.det(U @ Vh)))], dtype=torch.float64))
    R = U @ D @ Vh
    th = torch.acos(((torch.trace(R) - 1) / 2).clamp(-1, 1))
    v = torch.stack([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    om = v * (th / v.norm().clamp(min=1e-12))
    x = torch.zeros(N, dtype=torch.float64)
    x[:3], x[3:6] = om, tg[0]
    return x.float().double()
