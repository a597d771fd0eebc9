"""Seeded synthetic stand-ins for the SMPL arrays, shaped like a body, for the SMPL-fit tests (no real SMPL file): a coarse
point cloud round 24 rest joints, small random blend shapes, skinning weights with at most 4 non-zeros per vertex that sum to
1, and joint / H36M regressors whose rows are convex combinations.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

# rough rest positions of the 24 SMPL joints in metres (y up), smpl_layer.KINTREE_PARENTS order
REST = np.array([
    [0.00, 0.00, 0.00], [0.07, -0.09, 0.00], [-0.07, -0.09, 0.00], [0.00, 0.11, -0.02], [0.10, -0.48, 0.01], [-0.10, -0.48, 0.01],
    [0.00, 0.25, -0.01], [0.09, -0.88, -0.03], [-0.09, -0.88, -0.03], [0.00, 0.30, 0.01], [0.11, -0.94, 0.12], [-0.11, -0.94, 0.12],
    [0.00, 0.51, -0.03], [0.08, 0.42, -0.02], [-0.08, 0.42, -0.02], [0.00, 0.58, 0.05], [0.17, 0.44, -0.02], [-0.17, 0.44, -0.02],
    [0.43, 0.43, -0.03], [-0.43, 0.43, -0.03], [0.68, 0.43, -0.02], [-0.68, 0.43, -0.02], [0.77, 0.42, -0.01], [-0.77, 0.42, -0.01]])
PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
# the SMPL joint each of the 17 regressed H36M rows sits at (row order of the regressor, before smpl_to_h36m's exchange)
H36M_AT = (0, 2, 5, 8, 1, 4, 7, 6, 12, 15, 15, 16, 18, 20, 17, 19, 21)
SIZES = (70, 300, 513)          # under one pass of 256 threads; a pass and a tail; two passes and one vertex
REGRESSORS = ('dense', 'nine')


def arrays(V, regressor='dense', seed=0):
    """-> dict with SMPL_Layer.from_arrays' keys, `h36m_regressor` [17,V] and `f` (a seeded face list), float32."""
    rng = np.random.Generator(np.random.PCG64(1000 * seed + V))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    home = np.arange(V) % 24                                              # every joint owns vertices (V >= 24)
    vt = REST[home] + 0.04 * rng.standard_normal((V, 3))
    w = np.zeros((V, 24))
    for v in range(V):
        others = rng.choice([j for j in range(24) if j != home[v]], size=int(rng.integers(0, 4)), replace=False)
        share = rng.random(len(others)) * 0.15
        w[v, others] = share
        w[v, home[v]] = 1.0 - share.sum()
    jr = np.zeros((24, V))
    for j in range(24):
        own = np.nonzero(home == j)[0]
        jr[j, own] = rng.random(len(own)) + 0.1
    jr /= jr.sum(1, keepdims=True)
    hr = np.zeros((17, V))
    if regressor == 'dense':
        for l, j in enumerate(H36M_AT):
            d2 = ((vt - REST[j] - (np.array([0, 0.1, 0]) if l == 10 else 0)) ** 2).sum(1)
            hr[l] = np.exp(-d2 / (2 * 0.05 ** 2)) + 1e-3 * rng.random(V) + 1e-4          # every column is non-zero
    elif regressor == 'nine':
        cols = rng.choice(V, size=9, replace=False)
        hr[:, cols] = rng.random((17, 9)) ** 3 + 1e-3
    else:
        raise ValueError(regressor)
    hr /= hr.sum(1, keepdims=True)
    return dict(v_template=f32(vt.reshape(1, V, 3)), shapedirs=f32(0.01 * rng.standard_normal((V, 3, 10))),
                posedirs=f32(0.003 * rng.standard_normal((V, 3, 207))), J_regressor=f32(jr), weights=f32(w),
                h36m_regressor=f32(hr), f=rng.integers(0, V, (2 * V, 3)), kintree_parents=list(PARENTS))


def random_params(B, seed, pose_amp=1.0, beta_amp=1.0):
    """-> x [B,85] float32-representable float64: omega (any direction, angle up to 2.5), t in mm, body pose with every angle
    in [-pose_amp, pose_amp], betas ~ beta_amp N(0, 1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    om = rng.standard_normal((B, 3))
    om *= (rng.uniform(0.2, 2.5, (B, 1)) / np.linalg.norm(om, axis=1, keepdims=True))
    t = rng.uniform(-1500, 1500, (B, 3)) + np.array([0, 0, 3000.0])
    th = rng.uniform(-pose_amp, pose_amp, (B, 69))
    be = beta_amp * rng.standard_normal((B, 10))
    return np.concatenate([om, t, th, be], axis=1).astype(np.float32).astype(np.float64)
