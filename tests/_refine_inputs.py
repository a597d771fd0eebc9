"""Synthetic multi-view inputs of the refinement's tests and of tools/bench_tri_refine.py: numpy only, seeded."""
import numpy as np

SIGMA_PX = 2.0


def project(P, world, weight=None):
    """Exact (u, v) of world [B,K,3] in float64 through the float32 P [B,V,3,4]; weight = depth (what the reference uses)."""
    wh = np.concatenate([world.astype(np.float64), np.ones(world.shape[:2] + (1,))], -1)
    h = np.einsum('bvij,bkj->bvki', P.astype(np.float64), wh)
    w = h[..., 2] if weight is None else np.broadcast_to(weight, h[..., 2].shape)
    return np.stack([h[..., 0] / h[..., 2], h[..., 1] / h[..., 2], w], -1).astype(np.float32)


def ring_rig(B, V, K, seed, baseline_mm=None):
    """-> (exact points [B,V,K,3] with the depth as weight, P [B,V,3,4] float32, world [B,K,3]).  Camera v stands at the angle
    v * 360 / max(V, 4) degrees (so two cameras are 90 degrees apart, never opposite) +- 10, 3-5 m out, -0.5..1 m up, and looks
    at the subject.  `baseline_mm`: two cameras, the second one the first one moved sideways by that much."""
    rng = np.random.Generator(np.random.PCG64(seed))
    world = rng.normal(0.0, 350.0, (B, K, 3)).astype(np.float32)
    P = np.zeros((B, V, 3, 4), np.float32)
    for b in range(B):
        for v in range(V):
            a = 2 * np.pi * v / max(V, 4) + np.deg2rad(rng.uniform(-10, 10))
            d = rng.uniform(3000, 5000)
            c = np.array([d * np.cos(a), d * np.sin(a), rng.uniform(-500, 1000)])
            z = rng.uniform(-100, 100, 3) - c
            z /= np.linalg.norm(z)
            x = np.cross(z, [0.0, 0.0, 1.0])
            x /= np.linalg.norm(x)
            R = np.stack([x, np.cross(z, x), z])
            if baseline_mm is not None and v == 1:
                R, c = Rprev, cprev + baseline_mm * Rprev[0]
            Rprev, cprev = R, c
            fx, fy, cx, cy = rng.uniform(1100, 1200), rng.uniform(1100, 1200), rng.uniform(480, 540), rng.uniform(480, 540)
            P[b, v] = (np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]) @ np.concatenate([R, -(R @ c)[:, None]], 1)).astype(np.float32)
    return project(P, world), P, world


def noisy(rig, seed, sigma=SIGMA_PX):
    """Gaussian pixel noise of `sigma` on both axes of every point."""
    pts, P, world = rig
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = pts.copy()
    pts[..., :2] += (sigma * rng.normal(0.0, 1.0, pts.shape[:3] + (2,))).astype(np.float32)
    return pts, P, world
