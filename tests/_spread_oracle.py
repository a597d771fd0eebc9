"""Heat-map spread (xas_head_spread, ops_head.spread_flip, modules.util.spread_weight) restated in float64 numpy from the
definition - the plain soft-max and the plain moments, not the kernel's merge - plus the inputs that the CPU and the GPU test
files share, and a float32 numpy model of the kernel's record-and-merge scheme from which the GPU test's tolerance is taken.

    python tests/_spread_oracle.py        prints the float32 model's distance from the float64 definition for every shape
"""
import numpy as np

# (D, K, B) of tests/test_gpu_head_spread.py and the launch path each reaches (policy_of below restates the dispatch rule).
SHAPES = [(4, 1, 2), (4, 3, 2), (4, 4, 2), (8, 2, 3), (12, 2, 2), (64, 2, 1), (44, 94, 1), (128, 1, 1)]
# Tolerance of the GPU test: 8 x the largest |float32 model - float64 definition| over SHAPES with logits() below, means and
# second moments apart (this file run as a script prints both maxima; DESIGN.md records the run).
MODEL_ERR_MEAN, MODEL_ERR_MOM2 = 8.807e-06, 2.925e-04     # cells ((44, 94, 1)), cells^2 ((128, 1, 1)): largest model error seen
TOL_MEAN, TOL_MOM2 = 8 * MODEL_ERR_MEAN, 8 * MODEL_ERR_MOM2


def logits(D, K, B, seed=0):
    """[B, K*D, D, D] float32, randn * 3, rounded to multiples of 2^-10 so that logits + 1e4 is exact in float32."""
    rng = np.random.Generator(np.random.PCG64(1000 * D + 10 * K + B + seed))
    l = rng.standard_normal((B, K * D, D, D)) * 3.0
    return (np.round(l * 1024.0) / 1024.0).astype(np.float32)


def spike(D, K=1):
    """Logit 80 at cell (h, w) = (D-1, D-1) of depth bin 1 of every joint, else 0."""
    l = np.zeros((1, K, D, D, D), np.float32)
    l[:, :, 1, D - 1, D - 1] = 80.0
    return l.reshape(1, K * D, D, D)


def spread64(l, K):
    """logits [B, K*D, H, W] -> [B, K, 5] float64: (E w, E h, Var w, Var h, Cov(w, h)) of the x-y marginal of the soft-max over
    each joint's D*H*W logits, in cells.  A joint with a NaN logit is NaN."""
    l = np.asarray(l, np.float64)
    B, C, H, W = l.shape
    D = C // K
    l = l.reshape(B, K, D, H, W)
    with np.errstate(invalid='ignore'):
        e = np.exp(l - np.nanmax(np.where(np.isnan(l), -np.inf, l), axis=(2, 3, 4), keepdims=True))
        q = e.sum(axis=2) / e.sum(axis=(2, 3, 4))[..., None, None]            # [B,K,H,W]
    w, h = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    s = lambda a: (q * a).sum(axis=(2, 3))
    uw, uh = s(w), s(h)
    dw, dh = w - uw[..., None, None], h - uh[..., None, None]
    return np.stack([uw, uh, s(dw * dw), s(dh * dh), s(dw * dh)], axis=-1)


def marginal64(l, K):
    """[B, K, H, W] float64 x-y marginals (for the flip restatement)."""
    l = np.asarray(l, np.float64)
    B, C, H, W = l.shape
    l = l.reshape(B, K, C // K, H, W)
    e = np.exp(l - l.max(axis=(2, 3, 4), keepdims=True))
    return e.sum(axis=2) / e.sum(axis=(2, 3, 4))[..., None, None]


def moments64(q):
    """[..., H, W] distributions -> [..., 5]."""
    H, W = q.shape[-2:]
    w, h = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    s = lambda a: (q * a).sum(axis=(-2, -1))
    uw, uh = s(w), s(h)
    dw, dh = w - uw[..., None, None], h - uh[..., None, None]
    return np.stack([uw, uh, s(dw * dw), s(dh * dh), s(dw * dh)], axis=-1)


def spread_flip64(l2b, K, perm):
    """Spread of the flip test's averaged heat-map, formed explicitly: logits [2B, K*D, H, W] of B images and their mirrors ->
    the moments of (q[b, k] + mirror_w(q[B + b, perm[k]])) / 2."""
    q = marginal64(l2b, K)
    B = q.shape[0] // 2
    return moments64(0.5 * (q[:B] + q[B:][:, np.asarray(perm)][..., ::-1]))


def spread_weight64(spread, trans_image, cell_px=4.0):
    """[B,K,5], [B,2,3] -> [B,K]: 1 / sqrt((Var w + Var h + 2/12) (cell_px s)^2), s = 1 / sqrt(|det trans_image[:, :2, :2]|)."""
    a = np.asarray(trans_image, np.float64)
    det = np.abs(a[:, 0, 0] * a[:, 1, 1] - a[:, 0, 1] * a[:, 1, 0])
    s = 1.0 / np.sqrt(det)
    sp = np.asarray(spread, np.float64)
    return 1.0 / np.sqrt((sp[..., 2] + sp[..., 3] + 2.0 / 12.0) * (cell_px * s[:, None]) ** 2)


# ---- the kernel's scheme in float32 numpy ---------------------------------------------------------------------------------
def policy_of(D, K, general=False):
    """csrc/head.hip pow2_policy + make_geom: -> dict(pow2, G, C4, KT, ntile, C4t, R, P, nchunk)."""
    def slots(C4):
        g = 1
        while g < 64 and C4 % (g * 2) == 0:
            g *= 2
        return 64 // g
    G = D // 4
    C4 = K * G
    pow2 = 4 <= D <= 64 and D & (D - 1) == 0 and not general
    if pow2:
        pow2 = slots(C4) <= D * D and C4 * slots(C4) <= 1024
    ntile = 1 if pow2 else -(-K // (1024 // G))
    KT = -(-K // ntile)
    C4t = KT * G
    R = slots(C4) if pow2 else 1
    while C4t * R * 2 <= 640 and R * 2 <= D * D:
        R *= 2
    P = min(max(R, 128), D * D) // R * R
    return dict(pow2=pow2, G=G, C4=C4, KT=KT, ntile=ntile, C4t=C4t, R=R, P=P, nchunk=-(-D * D // P))


F = np.float32


def _merge(a, b):
    """Pairwise merge of records (tuples of float32 arrays m, S, uw, uh, Mw, Mh, C), as spread_merge of head.hip."""
    with np.errstate(all='ignore'):
        m = np.maximum(a[0], b[0])
        sa = np.where(a[0] == -np.inf, F(0), np.exp(a[0] - m)).astype(F)
        sb = np.where(b[0] == -np.inf, F(0), np.exp(b[0] - m)).astype(F)
        Sa, Sb = a[1] * sa, b[1] * sb
        S = Sa + Sb
        f = np.where(S == 0, F(0), Sb / np.where(S == 0, F(1), S)).astype(F)
        x, dw, dh = Sa * f, b[2] - a[2], b[3] - a[3]
        return (m, S, a[2] + dw * f, a[3] + dh * f, a[4] * sa + b[4] * sb + dw * dw * x, a[5] * sa + b[5] * sb + dh * dh * x,
                a[6] * sa + b[6] * sb + dw * dh * x)


def model32(l, K, general=False):
    """logits [B, K*D, D, D] float32 -> [B, K, 5] float32 by the kernel's scheme in float32: per thread (pixel slot, channel
    quad) an online soft-max over its pixels, four to a trip, every pixel merged in as a one-point record; then the lanes of a
    joint (xor tree with the lower lane on the left, or in lane order), the slots of a block in slot order, the chunks of an
    image in ascending order; normalised at the end.  numpy's exp and division stand for the device's."""
    l = np.asarray(l, F)
    B, C, H, W = l.shape
    D = C // K
    g = policy_of(D, K, general)
    G, C4, R, P, nchunk = g['G'], g['C4'], g['R'], g['P'], g['nchunk']
    HW = D * D
    x = np.ascontiguousarray(l.transpose(0, 2, 3, 1)).reshape(B, HW, C4, 4)
    steps = P // R
    pix = (np.arange(nchunk)[:, None, None] * P + np.arange(R)[None, :, None] + np.arange(steps)[None, None, :] * R)
    local = np.arange(R)[None, :, None] + np.arange(steps)[None, None, :] * R + 0 * pix
    pend = np.minimum(P, HW - np.arange(nchunk) * P)[:, None, None]
    valid = local < pend                                                       # [nchunk,R,steps]
    nvis = valid.sum(axis=2)                                                   # visits of a thread
    quad = np.arange(steps)[None, None, :] < (nvis // 4 * 4)[..., None]        # steps taken four to a trip
    v = x[:, np.minimum(pix, HW - 1)]                                          # [B,nchunk,R,steps,C4,4]
    vmax = v.max(axis=-1)                                                      # (finite inputs only: fmaxf would drop a NaN)
    fw = (pix % W).astype(F)[None, :, :, :, None]
    fh = (pix // W).astype(F)[None, :, :, :, None]
    shape = (B, nchunk, R, C4)
    m = np.full(shape, -np.inf, F)
    S, uw, uh, Mw, Mh, Cc = (np.zeros(shape, F) for _ in range(6))
    with np.errstate(all='ignore'):
        for i in range(steps):
            act = valid[None, :, :, i, None]
            ahead = vmax[:, :, :, i]
            if i % 4 == 0 and i + 3 < steps:
                four = vmax[:, :, :, i:i + 4].max(axis=3)
                ahead = np.where(quad[None, :, :, i, None], four, ahead)
            mn = np.where(act, np.maximum(m, ahead), m)
            sc = np.where(mn == m, F(1), np.exp(m - mn)).astype(F)             # (a thread that has not started stays empty)
            m = mn
            S, Mw, Mh, Cc = S * sc, Mw * sc, Mh * sc, Cc * sc
            e = np.exp(v[:, :, :, i] - mn[..., None]).astype(F)
            es = (e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3])
            Sn = S + es
            f = np.where(Sn == 0, F(0), es / np.where(Sn == 0, F(1), Sn)).astype(F)
            xx, dw, dh = S * f, fw[:, :, :, i] - uw, fh[:, :, :, i] - uh
            new = (Sn, uw + dw * f, uh + dh * f, Mw + dw * dw * xx, Mh + dh * dh * xx, Cc + dw * dh * xx)
            S, uw, uh, Mw, Mh, Cc = (np.where(act, n, o) for n, o in zip(new, (S, uw, uh, Mw, Mh, Cc)))
    rec = tuple(a.reshape(B, nchunk, R, K, G) for a in (m, S, uw, uh, Mw, Mh, Cc))
    if g['pow2']:
        idx, o = np.arange(G), 1
        while o < G:
            rec = _merge(tuple(a[..., idx & ~o] for a in rec), tuple(a[..., idx | o] for a in rec))
            o *= 2
        rec = tuple(a[..., 0] for a in rec)
    else:
        r = tuple(a[..., 0] for a in rec)
        for j in range(1, G):
            r = _merge(r, tuple(a[..., j] for a in rec))
        rec = r
    r = tuple(a[:, :, 0] for a in rec)                                          # slots, in order
    for s in range(1, R):
        r = _merge(r, tuple(a[:, :, s] for a in rec))
    acc = (np.full((B, K), -np.inf, F),) + tuple(np.zeros((B, K), F) for _ in range(6))
    for c in range(nchunk):                                                     # chunks, ascending
        acc = _merge(acc, tuple(a[:, c] for a in r))
    with np.errstate(all='ignore'):
        vw, vh = acc[4] / acc[1], acc[5] / acc[1]
        return np.stack([acc[2], acc[3], np.where(vw < 0, F(0), vw), np.where(vh < 0, F(0), vh), acc[6] / acc[1]], axis=-1)


def model_errors(shapes=SHAPES):
    """-> [(shape, path, max |mean error|, max |second-moment error|)] of model32 against spread64 on logits()."""
    out = []
    for D, K, B in shapes:
        l = logits(D, K, B)
        e = np.abs(model32(l, K).astype(np.float64) - spread64(l, K))
        out.append(((D, K, B), 'pow2' if policy_of(D, K)['pow2'] else 'general', e[..., :2].max(), e[..., 2:].max()))
    return out


if __name__ == '__main__':
    rows = model_errors()
    for shape, path, em, e2 in rows:
        print('(D, K, B) = %-14s %-8s mean %.3e cells   second moments %.3e cells^2' % (shape, path, em, e2))
    print('largest: mean %.3e  second moments %.3e' % (max(r[2] for r in rows), max(r[3] for r in rows)))
