"""Inputs of the multi-view consistency loss's tests and of tools/bench_multiview_loss.py, on top of the rigs of
tests/_refine_inputs.py: numpy only, seeded."""
import numpy as np

S = 256.0
SHIFTS_MM = (0.0, 150.0, -200.0)


def patch_case(rig, seed, Hy=3, weight=None, huber=0.0, compare=True):
    """Image points [B,V,K,3] of a rig -> kps_xy through a crop affine per (b, view), and Hy world hypotheses per view."""
    pts, P, world = rig
    B, V, K, _ = pts.shape
    rng = np.random.Generator(np.random.PCG64(seed))
    ti = np.zeros((B, V, 2, 3))
    for b in range(B):
        for v in range(V):
            s, th = rng.uniform(0.24, 0.32), rng.uniform(-0.2, 0.2)
            A = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
            ti[b, v, :, :2] = A
            ti[b, v, :, 2] = np.array([S / 2, S / 2]) + rng.uniform(-6, 6, 2) - A @ pts[b, v, :, :2].astype(np.float64).mean(0)
    ti = ti.astype(np.float32)
    patch = np.einsum('bvij,bvkj->bvki', ti[..., :2].astype(np.float64), pts[..., :2].astype(np.float64)) + ti[:, :, None, :, 2]
    kps_xy = (patch / (S - 1.0) * 2.0 - 1.0).astype(np.float32)
    M = P[..., :3].astype(np.float64)
    centre = -np.einsum('bvij,bvj->bvi', np.linalg.inv(M), P[..., 3].astype(np.float64))           # [B,V,3]
    ray = world[:, None].astype(np.float64) - centre[:, :, None]
    ray /= np.linalg.norm(ray, axis=-1, keepdims=True)                                              # [B,V,K,3]
    hyp = np.stack([world[:, None] + s * ray for s in SHIFTS_MM[:Hy]], 2) + rng.normal(0.0, 2.0, (B, V, Hy, K, 3))
    return dict(kps_xy=kps_xy, ti=ti, world=hyp.astype(np.float32), P=P, weight=weight, S=S, huber=huber, compare=compare,
                planted=world)
