"""Float64 restatement of xas_triangulate_volume (include/xas_hip.h): the specification the GPU tests compare with.

Written from the header's formulas, not from the kernel: numpy over all voxels of a level at once, every sum by numpy, the
softmax in its plain two-pass form (subtract the maximum, exponentiate, normalise) and the covariance as the weighted mean of
(X - mean)(X - mean)^T.  Inputs are the float32 arrays the device reads; everything after the load is float64.

Besides xyz, cov and status every joint carries `lead`: at the last level, |largest score on a face of the grid - largest
score inside it| over max(1, |largest score|).  Status 0 against 2 hangs on the sign of that difference, so a case is a fair
test of the device's status only where `lead` is well above the rounding of a score (STATUS_MIN_LEAD).
"""
import numpy as np

STATUS_MIN_LEAD = 1e-9


def world_to_cube(cams, v, b, X, D, image_size, rect_width):
    """World points X [...,3] (float64) -> (w, h, d, Zc) of view v, sample b: cube coordinates in cells, not clamped."""
    f = lambda name: np.asarray(cams[name][v, b], np.float64)
    R, T, Km, A, pz = f('rot_world'), f('trans_world'), f('k_mat'), f('trans_image'), f('pelvis')[2]
    S, rect = float(np.float32(image_size)), float(np.float32(rect_width))
    Pc = X @ R.T + T
    Xc, Yc, Zc = Pc[..., 0], Pc[..., 1], Pc[..., 2]
    with np.errstate(all='ignore'):
        u = Km[0, 0] * Xc / Zc + Km[0, 2]
        vv = Km[1, 1] * Yc / Zc + Km[1, 2]
        up = A[0, 0] * u + A[0, 1] * vv + A[0, 2]
        vp = A[1, 0] * u + A[1, 1] * vv + A[1, 2]
        w = up * D / (S - 1.0)
        h = vp * D / (S - 1.0)
        d = ((Zc - pz) * S / rect / (S - 1.0) + 1.0) * D / 2.0
    return w, h, d, Zc


def sample(cube, w, h, d, Zc, out_penalty):
    """cube [H,W,D] float32 (one joint's channel of one view), cube coordinates [N] -> (samples [N], all logits finite)."""
    D = cube.shape[0]
    behind = ~(Zc > 0.0)
    pts, o = [], np.where(behind, 3.0 * D, 0.0)
    for c in (w, h, d):
        c = np.where(behind, 0.0, c)
        cl = np.clip(c, 0.0, D - 1.0)
        o = o + np.where(behind, 0.0, np.abs(c - cl))
        pts.append(cl)
    base = [np.minimum(np.floor(c), D - 2).astype(np.int64) for c in pts]
    frac = [c - i for c, i in zip(pts, base)]
    (w0, h0, d0), (fw, fh, fd) = base, frac
    val, finite = np.zeros(len(w0)), True
    for dh in (0, 1):
        for dw in (0, 1):
            for dd in (0, 1):
                l = cube[h0 + dh, w0 + dw, d0 + dd].astype(np.float64)
                finite = finite and bool(np.all(np.isfinite(l)))
                with np.errstate(all='ignore'):
                    val = val + (fh if dh else 1.0 - fh) * (fw if dw else 1.0 - fw) * (fd if dd else 1.0 - fd) * l
    return val - out_penalty * o, finite


def voxel_offsets(G, side):
    """[G^3,3] offsets of the voxel centres from the grid's centre, x fastest (index = (iz G + iy) G + ix)."""
    a = ((np.arange(G) + 0.5) / G - 0.5) * side
    iz, iy, ix = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing='ij')
    return np.stack([a[ix.ravel()], a[iy.ravel()], a[iz.ravel()]], -1), np.stack([ix.ravel(), iy.ravel(), iz.ravel()], -1)


def fuse_one(logits, chan, cams, b, k, init, views, weight, G, levels, side_mm, beta, out_penalty, image_size, rect_width):
    """One joint.  logits: list of V arrays [B,H,W,K*D] float32.  -> dict(xyz, cov, status, lead, scores of the last level)."""
    V = len(logits)
    D = logits[0].shape[1]
    K = logits[0].shape[3] // D
    beta, out_penalty, side = float(np.float32(beta)), float(np.float32(out_penalty)), float(np.float32(side_mm))
    take = []
    for v in range(V):
        ch = k if chan is None else int(chan[v, b, k])
        wt = 1.0 if weight is None else float(np.float32(weight[v, b, k]))
        sel = True if views is None else bool(int(views[b, k]) >> v & 1)
        if sel and np.isfinite(wt) and wt > 0 and 0 <= ch < K:
            take.append((v, ch, wt))
    x0 = np.asarray(init[b, k, :3], np.float32)
    through = lambda st: dict(xyz=x0.astype(np.float64), cov=np.full(6, np.nan), status=st, lead=np.inf)
    if len(take) < 2 or not np.all(np.isfinite(x0)):
        return through(1)
    centre = x0.astype(np.float64)
    for lvl in range(levels):
        off, idx = voxel_offsets(G, side * 0.5 ** lvl)
        X = centre + off
        score = np.zeros(len(X))
        for v, ch, wt in take:
            s, finite = sample(logits[v][b, :, :, ch * D:(ch + 1) * D], *world_to_cube(cams, v, b, X, D, image_size, rect_width),
                               out_penalty)
            if not finite:
                return through(3)
            score = score + wt * s
        score = beta * score
        p = np.exp(score - score.max())
        p = p / p.sum()
        mean = (p[:, None] * X).sum(0)
        last_centre, centre = centre, mean
    r = X - mean
    cov = np.array([(p * r[:, i] * r[:, j]).sum() for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
    face = np.any((idx == 0) | (idx == G - 1), axis=1)
    best = int(np.argmax(score))
    lead = abs(score[face].max() - score[~face].max()) / max(1.0, abs(score.max())) if (~face).any() else np.inf
    return dict(xyz=mean, cov=cov, status=2 if face[best] else 0, lead=lead, score=score, offsets=off, centre=last_centre)


def fuse(logits, chan, cams, init, views=None, weight=None, G=16, levels=2, side_mm=800.0, beta=1.0, out_penalty=1.0,
         image_size=256.0, rect_width=2000.0):
    """-> dict: xyz [B,K,3] float64, cov [B,K,6], status [B,K] uint8, lead [B,K]."""
    B, K = init.shape[:2]
    res = [[fuse_one(logits, chan, cams, b, k, init, views, weight, G, levels, side_mm, beta, out_penalty, image_size, rect_width)
            for k in range(K)] for b in range(B)]
    g = lambda key, dt: np.array([[r[key] for r in row] for row in res], dtype=dt)
    return dict(xyz=g('xyz', np.float64), cov=g('cov', np.float64), status=g('status', np.uint8), lead=g('lead', np.float64))
