"""Seeded synthetic rigs for the calibration tests: cameras on a ring looking at a 2 m volume, intrinsics like
xas_amd/synthetic.py's (f about 1150 px, principal point about 510 px), joints random in the volume.  The detections are the
true joints seen by the TRUE cameras plus pixel noise; the matrices handed to the solver belong to cameras that were bumped
(a fraction of a degree, a few mm), so there is something to calibrate.  init is the DLT under the bumped cameras.  numpy only."""
import numpy as np

CASES = {
    # name: N, V, K, sizes of the rigs, trials
    'minimum': dict(N=4, V=2, K=1, sizes=(4,), max_iter=3),
    'typical': dict(N=12, V=3, K=5, sizes=(9, 3), max_iter=3),
    'single_sample': dict(N=1, V=4, K=18, sizes=(1,), max_iter=3),
    'widest': dict(N=40, V=6, K=18, sizes=(14, 13, 13), max_iter=3),
    'cross_block': dict(N=40, V=4, K=18, sizes=(40,), max_iter=3),      # 720 points: 2 blocks of 256 and one of 208
}
VARIANTS = {'plain': (False, 0.0), 'weighted': (True, 0.0), 'huber': (False, 1.5), 'weighted_huber': (True, 1.5)}
SEEDS = {}       # case name -> seed, where the first seed gave a near-tie (test_calib_abi re-seeds on the CPU and says so)


def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def ring_cameras(V, rng, radius=4500.0):
    """-> K [V,3,3], R [V,3,3], t [V,3]: camera v looks at the origin from the ring, x_cam = R x + t."""
    Ks, Rs, ts = [], [], []
    for v in range(V):
        ang = 2 * np.pi * (v + 0.15 * rng.uniform(-1, 1)) / max(V, 3)
        c = np.array([radius * np.cos(ang), radius * np.sin(ang), 1500.0 + 400.0 * rng.uniform(-1, 1)])
        z = -c / np.linalg.norm(c)
        x = np.cross(z, [0.0, 0.0, 1.0]); x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        Ks.append(np.array([[1100 + 100 * rng.uniform(), 0, 480 + 60 * rng.uniform()],
                            [0, 1100 + 100 * rng.uniform(), 480 + 60 * rng.uniform()], [0, 0, 1.0]]))
        Rs.append(R); ts.append(-R @ c)
    return np.stack(Ks), np.stack(Rs), np.stack(ts)


def pmats(Ks, Rs, ts):
    return np.einsum('vij,vjk->vik', Ks, np.concatenate([Rs, ts[..., None]], -1))


def bump(Rs, ts, rng, deg, mm, keep0=True):
    """The cameras moved by up to `deg` degrees and `mm` mm each (camera 0 kept): P' = P T(-bump), roughly."""
    R2, t2 = Rs.copy(), ts.copy()
    for v in range(1 if keep0 else 0, len(Rs)):
        w = rng.normal(size=3); w *= np.deg2rad(deg) / np.linalg.norm(w)
        d = rng.normal(size=3); d *= mm / np.linalg.norm(d)
        E = rodrigues(w)
        R2[v] = Rs[v] @ E
        t2[v] = ts[v] + Rs[v] @ d
    return R2, t2


def dlt(points, P, used):
    """points [V,3], P [V,3,4], used [V] bool -> X [3] (float64)."""
    rows = []
    for v in np.nonzero(used)[0]:
        rows += [points[v, 0] * P[v, 2] - P[v, 0], points[v, 1] * P[v, 2] - P[v, 1]]
    if len(rows) < 4:
        return np.full(3, np.nan)
    _, _, Vt = np.linalg.svd(np.stack(rows))
    return Vt[-1, :3] / Vt[-1, 3]


def make(name, variant='plain', seed=None, noise_px=None, deg=0.3, mm=5.0, plant=True):
    spec = CASES[name]
    N, V, K, sizes = spec['N'], spec['V'], spec['K'], spec['sizes']
    weighted, huber = VARIANTS[variant]
    noise_px = spec.get('noise_px', 1.0) if noise_px is None else noise_px
    rng = np.random.default_rng(SEEDS.get(name, 20260 + sum(map(ord, name))) if seed is None else seed)
    R = len(sizes)
    rig_sorted = np.repeat(np.arange(R), sizes)
    perm = rng.permutation(N) if N > 1 else np.arange(N)
    rig = rig_sorted[perm]                                                  # any order: the wrapper sorts
    points = np.zeros((N, V, K, 3), np.float32)
    P = np.zeros((N, V, 3, 4), np.float32)
    truth = rng.uniform(-1000, 1000, size=(N, K, 3))
    cams = []
    for r in range(R):
        Ks, Rs, ts = ring_cameras(V, rng)
        Rb, tb = bump(Rs, ts, rng, deg, mm)
        cams.append((pmats(Ks, Rs, ts), pmats(Ks, Rb, tb)))
    for n in range(N):
        Pt, Pb = cams[rig[n]]
        h = np.einsum('vij,kj->vki', Pt, np.concatenate([truth[n], np.ones((K, 1))], 1))
        points[n, :, :, :2] = h[..., :2] / h[..., 2:] + noise_px * rng.normal(size=(V, K, 2))
        points[n, :, :, 2] = rng.uniform(0.5, 1.5, size=(V, K))
        P[n] = Pb
    views = None
    if plant and N * K >= 4:
        views = np.zeros((N, K), np.uint8)
        flat = views.reshape(-1)
        pick = rng.permutation(N * K)
        for j, i in enumerate(pick[:max(2, N * K // 6)]):                   # some masks; the rest stay 0 = all valid views
            flat[i] = [(1 << V) - 1, 0b11 | 0xC0, ((1 << V) - 2) | 0x80, 1][j % 4]   # bits >= V, and one view only
        if N * K >= 8:
            n, k = divmod(int(pick[-1]), K)
            points[n, 1:, k, 2] = [0.0, np.nan, -1.0, np.inf, 0.0][:V - 1]      # fewer than two valid views
            n, k = divmod(int(pick[-2]), K)
            points[n, 0, k, 2] = 0.0                                        # one view dropped, still free where V >= 3
    init = np.zeros((N, K, 4), np.float32)
    for n in range(N):
        for k in range(K):
            w = points[n, :, k, 2]
            used = (w > 0) & np.isfinite(w)
            if views is not None and views[n, k]:
                used &= np.array([(views[n, k] >> v) & 1 for v in range(V)], bool)
            init[n, k, :3] = dlt(points[n, :, k].astype(np.float64), P[n].astype(np.float64), used)
            init[n, k, 3] = w[used].mean() if used.any() else 0.0
    if plant and N * K >= 8:
        flat = init.reshape(-1, 4)
        flat[int(pick[-3]), 1] = np.nan                                     # a start that is not finite
        n, k = divmod(int(pick[-4]), K)                                     # a start behind camera 1
        Pn = P[n, 1].astype(np.float64)
        centre = -np.linalg.solve(Pn[:, :3], Pn[:, 3])
        init[n, k, :3] = centre + 2.0 * (centre - 0.0) / 4.5                # 2 m further out along the ray from the origin
    delta0 = np.zeros((R, V, 6))
    if 'start' in spec:
        delta0 = rng.normal(size=(R, V, 6)) * np.array([spec['start'][0]] * 3 + [spec['start'][1]] * 3)
        delta0[:, 0] = 0.0
    return dict(name=name, variant=variant, N=N, V=V, K=K, R=R, rig=rig, points=points, P=P, init=init, views=views,
                truth=truth, weighted=weighted, huber=huber, free_mask=((1 << V) - 1) & ~1, prior_rot=1e4, prior_trans=1e-2,
                delta0=delta0, max_iter=spec['max_iter'], true_P=[c[0] for c in cams])


def planted(seed=7):
    """Planted recovery: the typical shape (V = 3), cameras 1..2 bumped by 1 degree and 15 mm, noise-free detections, tiny priors."""
    c = make('typical', seed=seed, noise_px=0.0, deg=1.0, mm=15.0, plant=False)
    c.update(name='planted', prior_rot=1e-6, prior_trans=1e-9, max_iter=20)
    return c
