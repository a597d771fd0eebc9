"""xas_mesh_render on the GPU against the float64 rasteriser of tests/_render_oracle.py, on the fixtures of
tests/_render_inputs.py.

What is compared, per fixture:
  face_id, mask  EQUAL on every compared pixel.  A pixel is left out only where the oracle's two nearest covering depths are
                 closer than 1e-9 of the fixture's depth range, and only up to 0.1 % of the fixture's covered pixels.  The quad,
                 the crossing triangles, the edge cases and the crowded tile are compared in full (their close pixels are exact
                 ties, which the face index decides).  Counted with the oracle alone (tests/test_render_oracle.py), ellipsoid
                 seed 3: 188 / 1195 / 3076 covered pixels at S = 16 / 40 / 64 and 0 of them under the gap at every size.
  zbuf           within 4 fp32 ulp of the largest |depth| of the fixture; +inf exactly where the oracle hits nothing.
  img            within 1e-6 of the oracle on compared pixels; the background exactly elsewhere.
And every call: a second call gives the same bits, and so does a call into buffers pre-filled with NaN (every element is
written)."""
import functools

import numpy as np
import pytest
import torch

import _render_inputs as ri
import _render_oracle as ro
from test_render_oracle import GAP_CAP, close_pixels

pytestmark = pytest.mark.gpu
ALL = ('img', 'mask', 'zbuf', 'face_id')


@functools.lru_cache(maxsize=None)
def oracle(key):
    """(fixture, oracle result), computed once per fixture and shared; nobody writes to either."""
    kind, args = key[0], key[1:]
    fix = {'quad': ri.quad, 'crossing': ri.crossing, 'edge': ri.edge_case, 'crowded': ri.crowded, 'ellipsoids': ri.ellipsoids}[kind](*args)
    return fix, ro.render(**ri.render_args(fix))


def gpu_render(fix, want=ALL):
    from xas_amd import ops_render
    dev = 'cuda'
    rgb = None if fix['face_rgb'] is None else torch.from_numpy(fix['face_rgb']).to(dev)
    light = None if fix['light'] is None else torch.tensor(fix['light'], dtype=torch.float32, device=dev)
    out = ops_render.render_mesh(torch.from_numpy(fix['verts']).to(dev), torch.from_numpy(fix['faces']).to(dev), face_rgb=rgb, light=light,
                                 ambient=fix['ambient'], depth_scale=fix['depth_scale'], background=fix['background'],
                                 size=fix['size'], want=want)
    assert tuple(out) == tuple(k for k in ALL if k in want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(fix, o, g, full):
    covered = o['face_id'] >= 0
    close = np.zeros_like(covered) if full else close_pixels(fix, o)
    print('covered %d, left out %d (cap %.1f)' % (covered.sum(), close.sum(), GAP_CAP * covered.sum()))
    assert close.sum() <= GAP_CAP * covered.sum()
    cmp = ~close
    assert np.array_equal(g['face_id'][cmp], o['face_id'][cmp])
    assert np.array_equal(g['mask'][:, 0][cmp], o['mask'][:, 0][cmp]) and set(np.unique(g['mask'])) <= {0.0, 1.0}
    hit = covered & cmp
    assert np.isposinf(g['zbuf'][~covered]).all()
    finite = fix['verts'][..., 2][np.isfinite(fix['verts'][..., 2])]
    zmax = float(np.abs(finite).max()) if finite.size else 0.0
    tol = 4 * float(np.spacing(np.float32(zmax)))
    zerr = np.abs(g['zbuf'][hit].astype(np.float64) - o['z64'][hit]).max() if hit.any() else 0.0
    cm = np.broadcast_to(hit[:, None], g['img'].shape)
    ierr = np.abs(g['img'][cm].astype(np.float64) - o['img'][cm]).max() if hit.any() else 0.0
    print('zbuf error %.3g (tolerance %.3g), img error %.3g (tolerance 1e-6)' % (zerr, tol, ierr))
    assert zerr <= tol and ierr <= 1e-6
    bg = np.broadcast_to(~covered[:, None], g['img'].shape)
    assert (g['img'][bg] == np.float32(fix['background'])).all()


KEYS = [('quad',), ('crossing',)] + [('edge', n) for n in ri.EDGE_NAMES] + [('crowded',)]


@pytest.mark.parametrize('key', KEYS, ids=lambda k: '-'.join(str(p) for p in k))
def test_small_fixtures_in_full(key):
    fix, o = oracle(key)
    check(fix, o, gpu_render(fix), full=True)


@pytest.mark.parametrize('size,coloured,ambient', ri.ELLIPSOID_CASES)
def test_ellipsoids(size, coloured, ambient):
    fix, o = oracle(('ellipsoids', size, coloured, ambient))
    check(fix, o, gpu_render(fix), full=False)


@pytest.mark.parametrize('want', [('img', 'mask'), ('img', 'mask', 'zbuf'), ('img', 'mask', 'face_id'), ('mask',)])
def test_optional_outputs(want):
    fix, o = oracle(('ellipsoids', 40, True, 0.35))
    full, part = gpu_render(fix), gpu_render(fix, want)
    for k in want:
        assert np.array_equal(part[k], full[k])


def test_no_faces_and_no_samples():
    from xas_amd import ops_render
    v = torch.zeros(2, 4, 3, device='cuda')
    r = ops_render.render_mesh(v, torch.zeros(0, 3, dtype=torch.int32, device='cuda'), background=0.5, size=24, want=ALL)
    assert (r['img'] == 0.5).all() and (r['mask'] == 0).all() and torch.isposinf(r['zbuf']).all() and (r['face_id'] == -1).all()
    r = ops_render.render_mesh(v[:0], torch.tensor([[0, 1, 2]], device='cuda'), size=24, want=ALL)
    assert r['img'].shape == (0, 3, 24, 24) and r['face_id'].shape == (0, 24, 24)


@pytest.mark.selfcheck
@pytest.mark.parametrize('key', [('crowded',), ('ellipsoids', 40, True, 0.35), ('edge', 'half_right')], ids=lambda k: str(k[0]))
def test_bit_reproducible_and_every_element_written(key):
    from xas_amd import _lib
    fix, _ = oracle(key)
    a, b = gpu_render(fix), gpu_render(fix)
    for k in ALL:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    # straight through the C entry into buffers that hold NaN (and a face_id that holds a number no face has)
    dev = 'cuda'
    verts, faces = torch.from_numpy(fix['verts']).to(dev), torch.from_numpy(fix['faces']).to(dev)
    rgb = None if fix['face_rgb'] is None else torch.from_numpy(fix['face_rgb']).to(dev)
    light = None if fix['light'] is None else torch.tensor(fix['light'], dtype=torch.float32, device=dev)
    B, Nv, F, S = verts.shape[0], verts.shape[1], faces.shape[0], fix['size']
    nan = lambda *s: torch.full(s, float('nan'), device=dev)
    img, mask, zbuf, fid = nan(B, 3, S, S), nan(B, 1, S, S), nan(B, S, S), torch.full((B, S, S), 1 << 30, dtype=torch.int32, device=dev)
    ws = torch.full((_lib.query('xas_mesh_render_workspace_bytes', B, F, S),), 0xff, dtype=torch.uint8, device=dev)
    _lib.call('xas_mesh_render', _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(rgb), _lib.ptr(light), fix['ambient'], fix['depth_scale'],
              fix['background'], B, Nv, F, S, _lib.ptr(img), _lib.ptr(mask), _lib.ptr(zbuf), _lib.ptr(fid), _lib.ptr(ws))
    for k, t in zip(ALL, (img, mask, zbuf, fid)):
        assert np.array_equal(t.cpu().numpy().view(np.int32), a[k].view(np.int32)), k
