"""tests/_volume_oracle.py, the float64 specification of xas_triangulate_volume, against truths that do not depend on it.
CPU only: these pass without the kernel and say that the GPU tests compare with the right numbers."""
import numpy as np

import _volume_inputs as vi
import _volume_oracle as vo

BIMODAL = dict(B=2, V=4, K=3, D=12, seed=10, second=(0, 6))      # shared with tests/test_gpu_tri_volume.py
BIMODAL_GRID = dict(G=16, levels=2, side_mm=1000.0)


def test_hand_computed_voxel_pair():
    """G = 2, one level, two copies of one camera with R = I whose logits are a_v * d, linear in the depth cell alone.
    Trilinear interpolation of a linear function is exact, every voxel projects inside the cube (checked below by hand), so
    the score is beta * (a_0 + a_1) * d(Z): two planes of four voxels at Z = c -+ side / 4 whose scores differ by
    delta = beta (a_0 + a_1) (side / 2) S / rect / (S - 1) D / 2.  Hence z = c_z + (side / 4) tanh(delta / 2), x = c_x,
    y = c_y, cov = diag(q^2, q^2, q^2 (1 - tanh^2)), q = side / 4."""
    D, S, rect, side, beta = 8, 256.0, 2000.0, 200.0, 0.75
    a = (1.5, 0.5)
    cams = dict(trans_image=np.tile(np.array([[0.25, 0, 0], [0, 0.25, 0]], np.float32), (2, 1, 1, 1)),
                k_mat=np.tile(np.array([[1000, 0, 500], [0, 1000, 500], [0, 0, 1]], np.float32), (2, 1, 1, 1)),
                pelvis=np.tile(np.array([0, 0, 4000], np.float32), (2, 1, 1)),
                rot_world=np.tile(np.eye(3, dtype=np.float32), (2, 1, 1, 1)),
                trans_world=np.tile(np.array([0, 0, 4000], np.float32), (2, 1, 1)))
    # by hand: X, Y = c -+ 50 -> u = 1000 * (10 -+ 50) / (4000 -+ 50) + 500 in (489, 516); u' = u / 4; w = u' * 8 / 255 in (3.8, 4.1)
    for x in (-40.0, 60.0):
        for z in (3950.0, 4050.0):
            assert 0.0 < (1000.0 * x / z + 500.0) / 4.0 * D / (S - 1.0) < D - 1.0
    logits = [np.broadcast_to((av * np.arange(D, dtype=np.float32)), (1, D, D, D)).copy() for av in a]      # K = 1
    init = np.array([[[10.0, 10.0, 0.0]]], np.float32)
    r = vo.fuse(logits, None, cams, init, G=2, levels=1, side_mm=side, beta=beta, out_penalty=1.0, image_size=S, rect_width=rect)
    delta = beta * sum(a) * (side / 2.0) * S / rect / (S - 1.0) * D / 2.0
    q, t = side / 4.0, np.tanh(delta / 2.0)
    assert r['status'][0, 0] == 2                    # G = 2: every voxel lies on a face
    np.testing.assert_allclose(r['xyz'][0, 0], [10.0, 10.0, q * t], rtol=0, atol=1e-9)
    np.testing.assert_allclose(r['cov'][0, 0], [q * q, 0, 0, q * q, 0, q * q * (1 - t * t)], rtol=0, atol=1e-8)


def test_per_view_constant_changes_nothing():
    c = vi.case(2, 3, 3, 8, seed=5)
    kw = dict(G=7, levels=2, side_mm=1200.0)
    base = [(np.round(l * 1024.0) / 1024.0).astype(np.float32) for l in c['logits']]      # multiples of 2^-10: the shift is exact in float32
    r0 = vo.fuse(base, None, c['cams'], c['init'], **kw)
    shifted = [l + np.float32(4.0 * (v + 1)) for v, l in enumerate(base)]
    assert all(np.array_equal(s - np.float32(4.0 * (v + 1)), l) for v, (s, l) in enumerate(zip(shifted, base)))
    r1 = vo.fuse(shifted, None, c['cams'], c['init'], **kw)
    assert np.array_equal(r0['status'], r1['status'])
    np.testing.assert_allclose(r1['xyz'], r0['xyz'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(r1['cov'], r0['cov'], rtol=0, atol=1e-7)


def test_planted_unimodal_cubes_are_found():
    """A condition on the inputs as much as a test: at sigma = 1 cell and noise 0.02 the fused point lies within half a
    last-level voxel of the planted one, for every grid the GPU tests use on these rigs."""
    for D, V, G, levels, side in ((12, 4, 16, 2, 1000.0), (12, 3, 7, 3, 1000.0), (8, 5, 4, 1, 1200.0), (8, 2, 16, 1, 1600.0)):
        c = vi.case(2, V, 3, D, seed=40 + V)
        r = vo.fuse(c['logits'], None, c['cams'], c['init'], G=G, levels=levels, side_mm=side)
        err = np.linalg.norm(r['xyz'] - c['world'], axis=-1)
        voxel = side / G / 2 ** (levels - 1)
        print('D=%d V=%d G=%d levels=%d: fused within %.2f mm of the planted point, half a voxel = %.2f mm' % (D, V, G, levels, err.max(), voxel / 2))
        assert np.all(r['status'] == 0) and err.max() < voxel / 2


def test_bimodal_view_misleads_the_dlt_not_the_fusion():
    """View 0 of four carries a second mode of equal mass six cells away in w.  Its soft-argmax lies between the two modes, on
    neither.  At D = 12 (167 mm cells), G = 16, two levels from a 1000 mm grid (31.25 mm voxels at the last level), seed 10:
    the DLT of the four soft-argmax points misses the planted point by 208 .. 378 mm (more than two voxels = 62.5 mm on every
    joint), and the fused point, started from that DLT point, lies 3.4 .. 5.5 mm from it (half a voxel = 15.6 mm)."""
    c = vi.case(**BIMODAL)
    voxel = BIMODAL_GRID['side_mm'] / BIMODAL_GRID['G'] / 2 ** (BIMODAL_GRID['levels'] - 1)
    dlt_miss = np.linalg.norm(c['init'].astype(np.float64) - c['world'], axis=-1)
    r = vo.fuse(c['logits'], None, c['cams'], c['init'], **BIMODAL_GRID)
    fused_miss = np.linalg.norm(r['xyz'] - c['world'], axis=-1)
    print('DLT misses by %.1f .. %.1f mm, fusion by %.1f .. %.1f mm, voxel %.2f mm' % (dlt_miss.min(), dlt_miss.max(), fused_miss.min(),
                                                                                       fused_miss.max(), voxel))
    assert dlt_miss.min() > 2 * voxel
    assert fused_miss.max() < voxel / 2 and np.all(r['status'] == 0)
