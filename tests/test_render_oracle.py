"""The float64 rasteriser of tests/_render_oracle.py against the closed-form facts of the fixtures of tests/_render_inputs.py, and
the fixtures themselves against what tests/test_gpu_render.py assumes of them.  No GPU."""
import numpy as np
import pytest

import _render_inputs as ri
import _render_oracle as ro

GAP_REL = 1e-9          # of the fixture's depth range: under it a pixel may be left out of the GPU comparison ...
GAP_CAP = 1e-3          # ... up to this share of the fixture's covered pixels


def run(fix):
    return ro.render(**ri.render_args(fix))


def close_pixels(fix, o):
    """Covered pixels whose two nearest covering depths are closer than GAP_REL of the depth range (exact ties included)."""
    return (o['face_id'] >= 0) & (o['gap'] < GAP_REL * fix['depth_range'])


def test_quad_is_hit_once_and_the_diagonal_goes_to_the_lower_index():
    o = run(ri.quad())
    ys, xs = np.mgrid[0:16, 0:16]
    inside = (xs >= 2) & (xs <= 12) & (ys >= 2) & (ys <= 12)
    assert np.array_equal(o['mask'][0, 0] > 0, inside) and inside.sum() == 121
    expect = np.where(inside, np.where(ys <= xs, 0, 1), -1)              # face 0 is the side y <= x, diagonal included
    assert np.array_equal(o['face_id'][0], expect)
    diag = inside & (xs == ys)
    assert (o['ncover'][0][diag] == 2).all() and (o['ncover'][0][inside & ~diag] == 1).all() and (o['gap'][0][diag] == 0).all()
    assert (o['zbuf'][0][inside] == 5).all() and np.isposinf(o['zbuf'][0][~inside]).all()
    assert np.array_equal(o['img'][0, 0], np.where(expect == 0, 1, 0)) and np.array_equal(o['img'][0, 1], np.where(expect == 1, 1, 0))
    assert (o['img'][0, 2] == 0).all()


def test_crossing_triangles_are_decided_per_pixel():
    o = run(ri.crossing())
    ys, xs = np.mgrid[0:16, 0:16]
    inside = (xs >= 1) & (ys >= 1) & (xs + ys <= 16)
    assert np.array_equal(o['face_id'][0] >= 0, inside) and (o['ncover'][0][inside] == 2).all()
    assert np.array_equal(o['face_id'][0][inside], np.where(xs <= 8, 0, 1)[inside])          # equal at x = 8: the lower index
    assert np.array_equal(o['z64'][0][inside], np.minimum(xs - 1.0, 15.0 - xs)[inside])
    assert np.array_equal(o['gap'][0][inside], np.abs((xs - 1.0) - (15.0 - xs))[inside])
    assert set(np.unique(o['face_id'][0][inside])) == {0, 1}


@pytest.mark.parametrize('name', ri.EDGE_NAMES)
def test_edge_cases(name):
    fix = ri.edge_case(name)
    o = run(fix)
    S = fix['size']
    hit = o['face_id'][0] == 0
    assert set(np.unique(o['face_id'])) <= {-1, 0} and np.array_equal(o['mask'][0, 0] > 0, hit)
    assert (o['img'][0][:, ~hit] == np.float32(0.25)).all() and np.isposinf(o['zbuf'][0][~hit]).all()
    if name in ('zero_area', 'nan_vertex', 'index_nv', 'off_patch', 'sub_pixel'):
        assert not hit.any()
    elif name == 'whole_patch':
        assert hit.all()
        ys, xs = np.mgrid[0:S, 0:S]
        # z = 1 + (x + S) / (4 S) + 2 (y + S) / (4 S): the plane through the three vertices
        np.testing.assert_allclose(o['z64'][0], 1 + (xs + S) / (4.0 * S) + 2 * (ys + S) / (4.0 * S), rtol=1e-14)
    else:
        # clipped by the pixel grid only: the hit pixels are those of the same triangle rendered on a patch shifted so that it
        # lies wholly inside
        assert 0 < hit.sum() < S * S
        shift = 2 * S
        big = dict(fix, verts=fix['verts'] + np.float32([shift, shift, 0]), size=5 * S)
        ob = run(big)
        assert np.array_equal(ob['face_id'][0][shift:shift + S, shift:shift + S], o['face_id'][0])
        assert np.array_equal(ob['z64'][0][shift:shift + S, shift:shift + S], o['z64'][0])       # the shift is exact in fp32
        assert (ob['face_id'][0] == 0).sum() > hit.sum()                                          # part of it is off the patch
        edge = {'half_left': hit[:, 0], 'half_right': hit[:, -1], 'half_top': hit[0], 'half_bottom': hit[-1]}[name]
        assert edge.any()


def test_crowded_tile_fixture():
    """700 faces, every box meeting the tile of pixels 16..31: more than two chunks of 256 and a remainder; no covered pixel of
    it has two covering depths closer than the gap rule, tie or not, so it is compared in full."""
    fix = ri.crowded()
    F = len(fix['faces'])
    v = fix['verts'][0][fix['faces']]                                   # [F,3,3]
    lo, hi = np.ceil(v[..., :2].min(1)), np.floor(v[..., :2].max(1))
    assert F == 700 and ((lo <= 31) & (hi >= 16)).all() and (lo <= hi).all()
    o = run(fix)
    assert (o['ncover'] > 8).any() and len(np.unique(o['face_id'])) > 100
    assert (o['face_id'] >= ri.CHUNK * 2).any() and (o['face_id'][o['face_id'] >= 0] < ri.CHUNK).any()
    assert not close_pixels(fix, o).any()
    print('crowded: %d covered pixels, up to %d faces on one, %d distinct winners, smallest gap %.3g of the range' % (
        (o['face_id'] >= 0).sum(), o['ncover'].max(), len(np.unique(o['face_id'])) - 1, o['gap'].min() / fix['depth_range']))


def test_face_order_matters_only_at_exact_ties():
    rng = np.random.Generator(np.random.PCG64(2))
    for fix in (ri.crowded(), ri.ellipsoids(40, True, 0.35), ri.quad()):
        o = run(fix)
        perm = rng.permutation(len(fix['faces']))
        p = run(dict(fix, faces=fix['faces'][perm], face_rgb=None if fix['face_rgb'] is None else fix['face_rgb'][perm]))
        tie = o['gap'] == 0
        back = np.where(p['face_id'] >= 0, perm[np.maximum(p['face_id'], 0)], -1)
        assert np.array_equal(back[~tie], o['face_id'][~tie])
        assert np.array_equal(p['z64'], o['z64']) and np.array_equal(p['mask'], o['mask']) and np.array_equal(p['gap'], o['gap'])
        assert np.array_equal(p['img'][np.broadcast_to(~tie[:, None], p['img'].shape)], o['img'][np.broadcast_to(~tie[:, None], o['img'].shape)])
    assert tie.any()                                                     # the quad's diagonal


@pytest.mark.parametrize('size,coloured,ambient', ri.ELLIPSOID_CASES)
def test_ellipsoid_fixture_stays_within_the_cap(size, coloured, ambient):
    """The oracle alone: the pixels that the GPU comparison may leave out are at most 0.1 % of the covered ones."""
    fix = ri.ellipsoids(size, coloured, ambient)
    assert fix['verts'].shape[0] == 3 and len(fix['faces']) == 984
    o = run(fix)
    covered, close = (o['face_id'] >= 0).sum(), close_pixels(fix, o).sum()
    print('ellipsoids S=%d: %d covered pixels, %d under the gap, up to %d faces on one' % (size, covered, close, o['ncover'].max()))
    assert covered > 0.15 * 3 * size * size and close <= GAP_CAP * covered
    assert (o['ncover'] >= 4).any()                                      # the second ellipsoid pokes through: four layers somewhere
    assert all((o['face_id'][b] >= 816).any() and ((o['face_id'][b] >= 0) & (o['face_id'][b] < 816)).any() for b in range(3))
    assert not (o['face_id'][2][:, -1] < 0).all()                        # sample 2 runs off the patch's right side
    img = o['img']
    assert img.min() >= 0 and img.max() <= 1
    if ambient == 1.0 and not coloured:
        assert set(np.unique(img)) <= {0.0, 1.0}
