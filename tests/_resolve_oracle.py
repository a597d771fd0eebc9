"""Float64 restatement of xas_multiview_resolve (include/xas_hip.h): the specification the GPU tests compare with, built on the
DLT of tests/_tri_oracle.py (float32 rows as the kernels form them, float64 null vector by numpy's SVD, float64 residuals).

Every result carries its MARGINS, and `check_decidable` asserts them: a case is only a fair test of the device code if no
decision hangs on the last bits of a cost.
  cost_gap, cost_rel   per pair: runner-up cost minus best cost (px^2), and that difference over the runner-up cost.  Candidates
                       that give both joints exactly the same points (a coincident pair) are ONE candidate for this purpose:
                       their systems, solutions and costs are equal bit for bit on either side, so among them the smaller mask
                       wins by the tie rule, not by arithmetic.  inf where there is no second candidate.
  hyp_margin           per (view, joint): distance of the second-nearest hypothesis minus that of the nearest, mm.
  name_margin          per pair, with labels: |L1 sum as named - L1 sum exchanged|, in normalised patch units.
"""
import numpy as np

import _tri_oracle as to

MIN_COST_GAP_PX2 = 1.0
MIN_COST_REL = 0.1
MIN_HYP_MARGIN_MM = 1.0
# Each L1 sum has at most 2 * 6 * 2 float32 terms of size <= ~4, exact to ~2.4e-7 each, and is added up in double on both sides:
# the two implementations differ by less than 1e-5, a hundred times below this.
MIN_NAME_MARGIN = 1e-3


def _valid(p):
    return bool(np.isfinite(p[2]) and p[2] > 0)


def _solve_cost(pts, P, views):
    """DLT of one joint over `views` and the sum of its squared reprojection residuals there -> (X homogeneous, cost)."""
    X = to._solve({v: to._rows(pts[v], P[v]) for v in views}, views)
    with np.errstate(all='ignore'):
        cost = sum(to._residual(pts[v], P[v], X) ** 2 for v in views)
    return X, (cost if cost < np.inf else np.inf)             # NaN counts as +inf, as in the kernel


def _mean_w(pts, views):
    w = np.float32(0)
    for v in views:
        w = np.float32(w + np.float32(pts[v, 2]))
    with np.errstate(all='ignore'):
        return np.float32(w) / np.float32(len(views))


def stage1(pa, pc, P):
    """One pair.  pa, pc [V,3] float32 (u, v, weight) of joints a and c, P [V,3,4] -> dict(mask, valid, xyz [2,3], w [2],
    cost_gap, cost_rel).  pc None: an unpaired joint."""
    V = pa.shape[0]
    views = [v for v in range(V) if _valid(pa[v]) and (pc is None or _valid(pc[v]))]
    vmask = sum(1 << v for v in views)
    out = dict(mask=0, valid=vmask, cost_gap=np.inf, cost_rel=np.inf)
    n = 1 if pc is None else 2
    if len(views) < 2:
        out.update(xyz=np.full((n, 3), np.nan), w=np.array([_mean_w(p, views) for p in (pa, pc)[:n]], np.float32))
        return out
    if pc is None:
        X, _ = _solve_cost(pa, P, views)
        out.update(xyz=(X[:3] / X[3])[None], w=np.array([_mean_w(pa, views)], np.float32))
        return out
    anchor, seen, cands = views[0], {}, []
    for m in range(1 << V):
        if m & ~vmask or m >> anchor & 1:
            continue
        bit = np.array([m >> v & 1 for v in range(V)], bool)[:, None]
        qa, qc = np.where(bit, pc, pa), np.where(bit, pa, pc)
        key = qa[views].tobytes() + qc[views].tobytes()
        if key not in seen:                                  # the same points: the same arithmetic, bit for bit
            (Xa, ca), (Xc, cc) = _solve_cost(qa, P, views), _solve_cost(qc, P, views)
            cost = ca + cc
            seen[key] = (cost if cost < np.inf else np.inf, Xa, Xc, _mean_w(qa, views), _mean_w(qc, views))
        cands.append((seen[key][0], m, key))
    cands.sort(key=lambda t: t[:2])
    cost, m, key = cands[0]
    others = [t[0] for t in cands if t[2] != key]
    if others:
        with np.errstate(all='ignore'):
            out['cost_gap'] = others[0] - cost if cost < np.inf else 0.0
            out['cost_rel'] = np.inf if others[0] == np.inf and cost < np.inf else out['cost_gap'] / others[0]
    _, Xa, Xc, wa, wc = seen[key]
    out.update(mask=m, xyz=np.stack([Xa[:3] / Xa[3], Xc[:3] / Xc[3]]), w=np.array([wa, wc], np.float32))
    return out


def resolve(points, P, kps, world, perm, gt=None, image_size=256.0):
    """points [B,V,K,3], P [B,V,3,4], kps / world [B,V,Hy,K,3], perm [K], gt [B,V,K,3] or None -> dict of arrays:
    sel [B,V,K,3] f32, xyz [B,K,3] f64, w [B,K] f32, swap [B,K] u8, hyp [B,V,K] u8, named [B,K] u8 (with gt), valid [B,K] u8,
    and the margins cost_gap / cost_rel [B,K], hyp_margin [B,V,K], name_margin [B,K]."""
    points, P, kps, world = (np.asarray(t, np.float32) for t in (points, P, kps, world))
    B, V, K, _ = points.shape
    Hy = kps.shape[2]
    perm = [int(c) for c in perm]
    perm = [c if 0 <= c < K and perm[c] == k else k for k, c in enumerate(perm)]
    o = dict(sel=np.zeros((B, V, K, 3), np.float32), xyz=np.zeros((B, K, 3)), w=np.zeros((B, K), np.float32),
             swap=np.zeros((B, K), np.uint8), hyp=np.zeros((B, V, K), np.uint8), named=np.zeros((B, K), np.uint8),
             valid=np.zeros((B, K), np.uint8), cost_gap=np.full((B, K), np.inf), cost_rel=np.full((B, K), np.inf),
             hyp_margin=np.full((B, V, K), np.inf), name_margin=np.full((B, K), np.inf))
    if gt is not None:
        S = np.float32(image_size)
        g = np.asarray(gt, np.float32)[..., :2] / (S - np.float32(1)) * np.float32(2) - np.float32(1)
    for b in range(B):
        for a in range(K):
            c = perm[a]
            if c < a:
                continue
            ks = (a,) if c == a else (a, c)
            r = stage1(points[b, :, a], None if c == a else points[b, :, c], P[b])
            views = [v for v in range(V) if r['valid'] >> v & 1]
            for i, k in enumerate(ks):
                o['xyz'][b, k], o['w'][b, k], o['swap'][b, k], o['valid'][b, k] = r['xyz'][i], r['w'][i], r['mask'], r['valid']
                o['cost_gap'][b, k], o['cost_rel'][b, k] = r['cost_gap'], r['cost_rel']
                x = o['xyz'][b, k].astype(np.float32).astype(np.float64)             # the point as it is written
                for v in range(V):
                    s = perm[k] if r['mask'] >> v & 1 else k
                    h = 0
                    if np.isfinite(x).all():
                        d = ((world[b, v, :, s].astype(np.float64) - x) ** 2).sum(-1)
                        with np.errstate(all='ignore'):
                            h = int(np.argmin(np.where(np.isnan(d), np.inf, d))) if np.isfinite(d).any() else 0
                        if Hy > 1:
                            ds = np.sort(np.sqrt(np.where(np.isnan(d), np.inf, d)))
                            o['hyp_margin'][b, v, k] = ds[1] - ds[0] if np.isfinite(ds[0]) else 0.0
                    o['hyp'][b, v, k] = h
                    o['sel'][b, v, k] = kps[b, v, h, s]
            if gt is not None and c != a and len(views) >= 2:
                l1 = lambda k, kg: sum(np.float64(np.float32(abs(o['sel'][b, v, k, 0] - g[b, v, kg, 0]) + abs(o['sel'][b, v, k, 1] - g[b, v, kg, 1])))
                                      for v in views)
                own, oth = l1(a, a) + l1(c, c), l1(a, c) + l1(c, a)
                same = all(np.array_equal(o['sel'][b, v, a, :2], o['sel'][b, v, c, :2]) for v in views)
                o['name_margin'][b, [a, c]] = np.inf if same else abs(own - oth)      # the same terms in another order
                if oth < own:
                    for v in views:
                        o['sel'][b, v, [a, c]] = o['sel'][b, v, [c, a]]
                        o['hyp'][b, v, [a, c]] = o['hyp'][b, v, [c, a]]
                    o['xyz'][b, [a, c]], o['w'][b, [a, c]] = o['xyz'][b, [c, a]], o['w'][b, [c, a]]
                    o['swap'][b, [a, c]] ^= np.uint8(r['valid'])
                    o['named'][b, [a, c]] = 1
    return o


def check_decidable(o, what=''):
    """The condition on the inputs of every case: for every pair the runner-up cost exceeds the best by 1 px^2 and by 10 % of
    itself; for every (view, joint) the second-nearest hypothesis is 1 mm farther than the nearest; with labels, the two
    namings differ by MIN_NAME_MARGIN."""
    gap, rel, hm, nm = (float(np.min(o[k])) for k in ('cost_gap', 'cost_rel', 'hyp_margin', 'name_margin'))
    assert gap >= MIN_COST_GAP_PX2, '%s: a runner-up cost lies %.3g px^2 above the best (needs >= %.1f)' % (what, gap, MIN_COST_GAP_PX2)
    assert rel >= MIN_COST_REL, '%s: a runner-up cost exceeds the best by %.3g of itself (needs >= %.2f)' % (what, rel, MIN_COST_REL)
    assert hm >= MIN_HYP_MARGIN_MM, '%s: two hypotheses lie within %.3g mm of each other (needs >= %.1f)' % (what, hm, MIN_HYP_MARGIN_MM)
    assert nm >= MIN_NAME_MARGIN, '%s: the two namings differ by %.3g (needs >= %g)' % (what, nm, MIN_NAME_MARGIN)
    return gap, rel, hm, nm
