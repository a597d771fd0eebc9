"""Float64 numpy rasteriser written from the specification of xas_mesh_render (include/xas_hip.h): a loop over the faces,
vectorised over the pixels.  Every operation is an IEEE double operation in the order the header writes it, so coverage, the
winning face and the depth are decided exactly as the kernel must decide them.  Besides the kernel's outputs it returns, per
pixel, the gap between the nearest and the second-nearest covering depth (+inf with fewer than two covering faces): where that
gap is zero the face index decides, and where it is tiny a comparison in another precision could decide otherwise."""
import numpy as np


def edge(qx, qy, sx, sy, tx, ty):
    """E(q, s, t) = (s - q) x (t - q)."""
    return (sx - qx) * (ty - qy) - (sy - qy) * (tx - qx)


def face_shade(a, b, c, light, ambient, depth_scale):
    """ambient + (1 - ambient) max(0, n . l) of one face; a, b, c float64 [3]."""
    ds = np.float64(np.float32(depth_scale))
    e1 = np.array([b[0] - a[0], b[1] - a[1], (b[2] - a[2]) * ds])
    e2 = np.array([c[0] - a[0], c[1] - a[1], (c[2] - a[2]) * ds])
    n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    if n[2] > 0:
        n = -n
    with np.errstate(all='ignore'):
        nl = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        if light is None:
            l = np.array([0.0, 0.0, -1.0])
        else:
            l = np.asarray(light, np.float32).astype(np.float64)
            l = l / np.sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2])
        d = ((n[0] / nl) * l[0] + (n[1] / nl) * l[1]) + (n[2] / nl) * l[2]
    amb = np.float64(np.float32(ambient))
    return amb + (1.0 - amb) * (d if d > 0 else 0.0)


def render(verts, faces, face_rgb=None, light=None, ambient=0.35, depth_scale=1.0, background=0.0, size=16):
    """verts [B,Nv,3] float32, faces [F,3] int -> dict(img [B,3,S,S] float32, mask [B,1,S,S] float32, zbuf [B,S,S] float32,
    z64 [B,S,S] float64, face_id [B,S,S] int32, gap [B,S,S] float64, ncover [B,S,S] int32)."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces).reshape(-1, 3)
    B, Nv, S = verts.shape[0], verts.shape[1], int(size)
    py, px = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing='ij')
    img = np.full((B, 3, S, S), np.float32(background), np.float32)
    best = np.full((B, S, S), np.inf)
    second = np.full((B, S, S), np.inf)
    fid = np.full((B, S, S), -1, np.int32)
    ncover = np.zeros((B, S, S), np.int32)
    for b in range(B):
        v64 = verts[b].astype(np.float64)
        for f, (i0, i1, i2) in enumerate(faces):
            if not (0 <= i0 < Nv and 0 <= i1 < Nv and 0 <= i2 < Nv):
                continue
            a, bb, c = v64[i0], v64[i1], v64[i2]
            if not (np.isfinite(a).all() and np.isfinite(bb).all() and np.isfinite(c).all()):
                continue
            area = edge(a[0], a[1], bb[0], bb[1], c[0], c[1])
            if area == 0:
                continue
            xs, ys = (a[0], bb[0], c[0]), (a[1], bb[1], c[1])
            box = (px >= min(xs)) & (px <= max(xs)) & (py >= min(ys)) & (py <= max(ys))
            if not box.any():
                continue
            w0 = edge(bb[0], bb[1], c[0], c[1], px, py)
            w1 = edge(c[0], c[1], a[0], a[1], px, py)
            w2 = edge(a[0], a[1], bb[0], bb[1], px, py)
            cov = box & (((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) if area > 0 else ((w0 <= 0) & (w1 <= 0) & (w2 <= 0)))
            if not cov.any():
                continue
            with np.errstate(all='ignore'):
                z = ((w0 * a[2] + w1 * bb[2]) + w2 * c[2]) / area
            ncover[b] += cov
            win = cov & (z < best[b])
            # second-nearest: the old best where this face wins, else this face's depth where it is nearer than the old second
            lose = cov & ~win & (z < second[b])
            second[b] = np.where(win, best[b], np.where(lose, z, second[b]))
            best[b] = np.where(win, z, best[b])
            fid[b] = np.where(win, f, fid[b])
            if win.any():
                shade = face_shade(a, bb, c, light, ambient, depth_scale)
                for ch in range(3):
                    col = np.float32((1.0 if face_rgb is None else np.float64(np.float32(face_rgb[f][ch]))) * shade)
                    img[b, ch] = np.where(win, col, img[b, ch])
    hit = fid >= 0
    with np.errstate(invalid='ignore'):
        gap = np.where(np.isfinite(second), second - best, np.inf)
    return dict(img=img, mask=hit[:, None].astype(np.float32), zbuf=best.astype(np.float32), z64=best, face_id=fid, gap=gap,
                ncover=ncover)
