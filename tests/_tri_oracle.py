"""Float64 restatement of xas_triangulate_robust (include/xas_hip.h): the specification the GPU tests compare with.

The DLT rows are formed in float32 exactly as the kernels form them (one rounding per operation, weight included); everything
after that is float64: the null vector by numpy's SVD, the reprojection residuals, the three-key choice of the best subset.

Every result carries its MARGINS, and `check_decidable` asserts them: a case is only a fair test of the device code if the
answer does not hang on the last bits of a residual.
  thr_margin   the smallest distance of any residual (any candidate subset, any valid view) from the threshold, px;
  count_gap    inliers of the best candidate minus inliers of the best candidate with ANOTHER inlier set (None if every
               candidate has the same inlier set).  Candidates with the same inlier set lead to the same views used, so ties
               among them cannot change the result.
"""
import numpy as np

MIN_THR_MARGIN_PX = 1.0


def _rows(pt, P):
    """The two float32 DLT rows of one view, c (u P2 - P0) and c (v P2 - P1), as the kernels form them: u P2 - P0 is one fused
    multiply-add (the float64 product of two float32 values is exact, so rounding the float64 difference to float32 is that
    fma but for rare double roundings), then one float32 multiplication by the weight."""
    u, v, c = (np.float32(t) for t in pt)
    P = P.astype(np.float32)
    fma = lambda a, b, d: (np.float64(a) * b.astype(np.float64) - d.astype(np.float64)).astype(np.float32)
    return np.stack([c * fma(u, P[2], P[0]), c * fma(v, P[2], P[1])]).astype(np.float32)


def _solve(rows, views):
    A = np.concatenate([rows[v] for v in views]).astype(np.float64)
    return np.linalg.svd(A)[2][-1]


def _residual(pt, P, X):
    h = P.astype(np.float64) @ X
    with np.errstate(all='ignore'):
        if h[2] / X[3] <= 0:
            return np.inf
        return float(np.hypot(h[0] / h[2] - np.float64(pt[0]), h[1] / h[2] - np.float64(pt[1])))


def robust_one(pts, P, thr):
    """pts [V,3] float32 (u, v, weight), P [V,3,4] float32 -> dict for one joint."""
    V = pts.shape[0]
    valid = [v for v in range(V) if np.isfinite(pts[v, 2]) and pts[v, 2] > 0]
    rows = {v: _rows(pts[v], P[v]) for v in valid}
    out = dict(valid=sum(1 << v for v in valid), thr_margin=np.inf, count_gap=None)
    if len(valid) < 2:
        w = np.float32(sum(np.float32(pts[v, 2]) for v in valid)) / np.float32(len(valid)) if valid else np.float32(np.nan)
        out.update(mask=0, used=out['valid'], xyz=np.full(3, np.nan), w=w, resid=np.nan)
        return out
    cands = []
    for m in range(1 << V):
        views = [v for v in range(V) if m >> v & 1]
        if len(views) < 2 or any(v not in valid for v in views):
            continue
        X = _solve(rows, views)
        r = {v: _residual(pts[v], P[v], X) for v in valid}
        for x in r.values():
            if np.isfinite(x):
                out['thr_margin'] = min(out['thr_margin'], abs(x - thr))
        inl = [v for v in valid if r[v] < thr]
        cands.append((-len(inl), sum(r[v] ** 2 for v in inl), m, sum(1 << v for v in inl)))
    cands.sort()
    best = cands[0]
    others = [c for c in cands if c[3] != best[3]]
    if others:
        out['count_gap'] = -best[0] - (-others[0][0])
    mask = best[3] if -best[0] >= 2 else 0
    used = mask if mask else out['valid']
    views = [v for v in range(V) if used >> v & 1]
    X = _solve(rows, views)
    r = np.array([_residual(pts[v], P[v], X) for v in views])
    w = np.float32(0)
    for v in views:
        w = np.float32(w + np.float32(pts[v, 2]))
    out.update(mask=mask, used=used, xyz=X[:3] / X[3], w=w / np.float32(len(views)), resid=float(np.sqrt(np.mean(r ** 2))))
    return out


def dlt(points, P):
    """The plain DLT over all views (xas_triangulate_dlt) in float64: [B,K,3]."""
    points, P = np.asarray(points, np.float32), np.asarray(P, np.float32)
    B, V, K, _ = points.shape
    out = np.zeros((B, K, 3))
    for b in range(B):
        for k in range(K):
            X = _solve({v: _rows(points[b, v, k], P[b, v]) for v in range(V)}, range(V))
            out[b, k] = X[:3] / X[3]
    return out


def decidable_one(pts, P, thr):
    """One joint's inputs meet the condition of check_decidable."""
    r = robust_one(pts, P, thr)
    return r['thr_margin'] >= MIN_THR_MARGIN_PX and (r['mask'] == 0 or r['count_gap'] is None or r['count_gap'] >= 1)


def robust(points, P, thr):
    """points [B,V,K,3], P [B,V,3,4] (float32 arrays) -> dict of arrays [B,K,...] + per-joint margins."""
    points, P = np.asarray(points, np.float32), np.asarray(P, np.float32)
    B, V, K, _ = points.shape
    res = [[robust_one(points[b, :, k], P[b], thr) for k in range(K)] for b in range(B)]
    g = lambda key, dt: np.array([[r[key] for r in row] for row in res], dtype=dt)
    gaps = [r['count_gap'] for row in res for r in row if r['count_gap'] is not None and r['mask'] != 0]
    return dict(mask=g('mask', np.uint8), used=g('used', np.uint8), xyz=g('xyz', np.float64), w=g('w', np.float32),
                resid=g('resid', np.float64), thr_margin=g('thr_margin', np.float64),
                min_count_gap=min(gaps) if gaps else None)


def check_decidable(o, what=''):
    """The condition on the inputs of every planted case: no residual within MIN_THR_MARGIN_PX of the threshold, and a best
    candidate with strictly more inliers than any candidate with another inlier set.  (Where no candidate has two inliers
    the views used are all valid views whichever candidate is best, so there the threshold margin alone decides.)"""
    m = float(np.min(o['thr_margin']))
    assert m >= MIN_THR_MARGIN_PX, '%s: a residual lies %.3f px from the threshold (needs >= %.1f)' % (what, m, MIN_THR_MARGIN_PX)
    assert o['min_count_gap'] is None or o['min_count_gap'] >= 1, '%s: best and runner-up candidate tie on the inlier count' % what
    return m
