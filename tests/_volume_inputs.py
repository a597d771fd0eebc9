"""Synthetic inputs of the volumetric fusion's tests (xas_triangulate_volume) and of tools/bench_tri_volume.py: numpy only, seeded.

A rig is V cameras on a ring looking at a subject near the world origin, each with its own intrinsics, a crop affine with
rotation and scale that puts the subject's 2 m box on the S x S patch, and the subject's depth as `pelvis`.  The heat-map cubes
are log-Gaussians (sigma in cells) centred on each view's cube coordinates of a planted world point, plus seeded noise.
"""
import numpy as np

from _volume_oracle import world_to_cube

S, RECT = 256.0, 2000.0


def rig(B, V, seed, inside=None):
    """-> cams: dict of float32 arrays with a leading [V,B] (trans_image [..,2,3], k_mat [..,3,3], pelvis [..,3], rot_world
    [..,3,3], trans_world [..,3]).  Camera v stands at v * 360 / max(V, 4) degrees +- 10, 3-5 m out, -0.5..1 m up.
    `inside` = (v, distance_mm): camera v stands that close to the origin instead, inside a grid round the subject, so that some
    voxels lie behind it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cams = dict(trans_image=np.zeros((V, B, 2, 3), np.float32), k_mat=np.zeros((V, B, 3, 3), np.float32),
                pelvis=np.zeros((V, B, 3), np.float32), rot_world=np.zeros((V, B, 3, 3), np.float32),
                trans_world=np.zeros((V, B, 3), np.float32))
    for b in range(B):
        for v in range(V):
            a = 2 * np.pi * v / max(V, 4) + np.deg2rad(rng.uniform(-10, 10))
            dist = rng.uniform(3000, 5000)
            c = np.array([dist * np.cos(a), dist * np.sin(a), rng.uniform(-500, 1000)])
            if inside is not None and inside[0] == v:
                c *= inside[1] / np.linalg.norm(c)
            z = rng.uniform(-100, 100, 3) - c
            z /= np.linalg.norm(z)
            x = np.cross(z, [0.0, 0.0, 1.0])
            x /= np.linalg.norm(x)
            R = np.stack([x, np.cross(z, x), z])
            T = -(R @ c)
            fx, fy, cx, cy = rng.uniform(1100, 1200), rng.uniform(1100, 1200), rng.uniform(480, 540), rng.uniform(480, 540)
            scale = (S - 1.0) / (fx * RECT / T[2]) * rng.uniform(0.9, 1.1)       # the 2 m box at the origin's depth fills the patch
            rot = np.deg2rad(rng.uniform(-25, 25))
            A = scale * np.array([[np.cos(rot), -np.sin(rot)], [np.sin(rot), np.cos(rot)]])
            t = (S - 1.0) / 2.0 + rng.uniform(-8, 8, 2) - A @ np.array([fx * T[0] / T[2] + cx, fy * T[1] / T[2] + cy])
            cams['trans_image'][v, b] = np.concatenate([A, t[:, None]], 1)
            cams['k_mat'][v, b] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
            cams['pelvis'][v, b] = [rng.uniform(-50, 50), rng.uniform(-50, 50), T[2] + rng.uniform(-40, 40)]
            cams['rot_world'][v, b] = R
            cams['trans_world'][v, b] = T
    return cams


def cube_coords(cams, world, D):
    """Planted world points [B,K,3] -> their cube coordinates (w, h, d) in every view: [V,B,K,3] float64."""
    V, B = cams['pelvis'].shape[:2]
    out = np.zeros((V, B, world.shape[1], 3))
    for v in range(V):
        for b in range(B):
            w, h, d, _ = world_to_cube(cams, v, b, world[b].astype(np.float64), D, S, RECT)
            out[v, b] = np.stack([w, h, d], -1)
    return out


def log_gaussian(centre, D, sigma):
    """[H,W,D] float64: -|cell - centre|^2 / (2 sigma^2), centre = (w, h, d) in cells."""
    g = np.arange(D, dtype=np.float64)
    return -((g[:, None, None] - centre[1]) ** 2 + (g[None, :, None] - centre[0]) ** 2 + (g[None, None, :] - centre[2]) ** 2) / (2.0 * sigma ** 2)


def cubes(cams, world, D, seed, sigma=1.5, noise=0.05, second=None):
    """-> list of V float32 arrays [B,H,W,K*D] (the head's NHWC layout: channel k * D + d).  `second` = (v, cells): view
    v's heat-map of every joint gets a second mode of EQUAL mass `cells` away along w, towards the side of the cube with more
    room (log of the sum of two Gaussians)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    coords = cube_coords(cams, world, D)
    V, B, K = coords.shape[:3]
    out = []
    for v in range(V):
        L = np.zeros((B, D, D, K * D), np.float32)
        for b in range(B):
            for k in range(K):
                g = log_gaussian(coords[v, b, k], D, sigma)
                if second is not None and second[0] == v:
                    side = 1.0 if coords[v, b, k, 0] < (D - 1) / 2.0 else -1.0
                    g = np.logaddexp(g, log_gaussian(coords[v, b, k] + np.array([side * second[1], 0.0, 0.0]), D, sigma))
                L[b, :, :, k * D:(k + 1) * D] = g + noise * rng.normal(0.0, 1.0, g.shape)
        out.append(L)
    return out


def planted(B, K, seed, spread_mm=150.0):
    """Planted world points [B,K,3] float32 round the origin."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-spread_mm, spread_mm, (B, K, 3)).astype(np.float32)


def soft_argmax_points(logits, cams, D):
    """The detections every other triangulation starts from: the soft-argmax (w, h) of every cube, taken
    to image pixels through the inverse crop (A3), weight 1 -> points [B,V,K,3] and P [B,V,3,4] float32 for the DLT."""
    V, B = cams['pelvis'].shape[:2]
    K = logits[0].shape[3] // D
    pts, P = np.zeros((B, V, K, 3), np.float32), np.zeros((B, V, 3, 4), np.float32)
    g = np.arange(D, dtype=np.float64)
    for v in range(V):
        for b in range(B):
            A = cams['trans_image'][v, b].astype(np.float64)
            P[b, v] = (cams['k_mat'][v, b].astype(np.float64) @ np.concatenate(
                [cams['rot_world'][v, b].astype(np.float64), cams['trans_world'][v, b].astype(np.float64)[:, None]], 1)).astype(np.float32)
            for k in range(K):
                l = logits[v][b, :, :, k * D:(k + 1) * D].astype(np.float64)
                p = np.exp(l - l.max())
                p /= p.sum()
                wh = np.array([(p.sum(axis=(0, 2)) * g).sum(), (p.sum(axis=(1, 2)) * g).sum()]) * (S - 1.0) / D   # u', v'
                pts[b, v, k, :2] = np.linalg.solve(A[:, :2], wh - A[:, 2])
                pts[b, v, k, 2] = 1.0
    return pts, P


def case(B, V, K, D, seed, sigma=1.0, noise=0.02, second=None, inside=None):
    """One seeded problem: dict(cams, world [B,K,3] planted, logits, points, P, init [B,K,3] float32 = the DLT of the cubes'
    soft-argmax points in float64 (tests/_tri_oracle.py), rounded)."""
    from _tri_oracle import dlt
    cams = rig(B, V, seed, inside=inside)
    world = planted(B, K, seed + 1)
    logits = cubes(cams, world, D, seed + 2, sigma=sigma, noise=noise, second=second)
    points, P = soft_argmax_points(logits, cams, D)
    init = dlt(points, P).astype(np.float32) if V >= 2 else world + np.float32(20.0)
    return dict(cams=cams, world=world, logits=logits, points=points, P=P, init=init, D=D)
