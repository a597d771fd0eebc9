"""Seeded inputs of the mesh-renderer tests (tests/test_render_oracle.py on the CPU, tests/test_gpu_render.py on the GPU; the mesh
builders also serve tools/bench_mesh_render.py): numpy only, no files, the smallest shapes at which xas_mesh_render can still go wrong.  Every fixture is a dict of render()'s arguments:
verts [B,Nv,3] float32, faces [F,3] int32, face_rgb [F,3] float32 or None, light, ambient, depth_scale, background, size;
plus `depth_range`, the spread of its finite depths (the unit of the oracle's depth-gap rule)."""
import functools

import numpy as np

TILE = 16          # the kernel's tile side and (squared) its compaction chunk
CHUNK = 256


def _fix(verts, faces, size, face_rgb=None, light=None, ambient=0.35, depth_scale=1.0, background=0.0):
    verts = np.asarray(verts, np.float32)
    if verts.ndim == 2:
        verts = verts[None]
    z = verts[..., 2][np.isfinite(verts[..., 2])]
    return dict(verts=verts, faces=np.asarray(faces, np.int32).reshape(-1, 3), face_rgb=None if face_rgb is None else np.asarray(face_rgb, np.float32),
                light=light, ambient=ambient, depth_scale=depth_scale, background=background, size=size,
                depth_range=float(z.max() - z.min()) if z.size else 0.0)


def quad():
    """Two triangles sharing the diagonal (2,2)-(12,12), which lies on pixel centres; vertices on integer pixels; both at one
    depth, so every pixel of the diagonal is an exact tie between face 0 and face 1."""
    v = [[2, 2, 5], [12, 2, 5], [12, 12, 5], [2, 12, 5]]
    return _fix(v, [[0, 1, 2], [0, 2, 3]], 16, face_rgb=[[1, 0, 0], [0, 1, 0]], ambient=1.0)


def crossing():
    """Two interpenetrating triangles over the same pixels: face 0 rises in depth with x, face 1 falls, so the nearer one
    changes at x = 8 (where the two are equal: the tie goes to face 0)."""
    v = [[1, 1, 0], [15, 1, 14], [1, 15, 0],         # face 0: z = x - 1
         [1, 1, 14], [15, 1, 0], [1, 15, 14]]        # face 1: z = 15 - x
    return _fix(v, [[0, 1, 2], [3, 4, 5]], 16, face_rgb=[[1, 0, 0], [0, 0, 1]], ambient=1.0)


EDGE_NAMES = ('zero_area', 'nan_vertex', 'index_nv', 'off_patch', 'half_left', 'half_right', 'half_top', 'half_bottom', 'sub_pixel',
              'whole_patch')


def edge_case(name, size=40):
    """One face each.  size = 40: three tiles a side, the last one partial."""
    S = size
    tri = {'zero_area': [[3, 3, 1], [9, 9, 1], [15, 15, 1]],
           'nan_vertex': [[3, 3, 1], [20, 4, 1], [5, np.nan, 1]],
           'index_nv': [[3, 3, 1], [20, 4, 1], [5, 22, 1]],
           'off_patch': [[-30, -5, 1], [-3, -8, 1], [-10, -40, 1]],
           'half_left': [[-9.5, 10, 1], [9.25, 4, 2], [8, 30.5, 3]],
           'half_right': [[S - 10.5, 3, 1], [S + 12.25, 17, 2], [S - 7, 33, 3]],
           'half_top': [[5, -11.5, 1], [31, -4, 2], [17.5, 12.25, 3]],
           'half_bottom': [[5, S - 12.5, 1], [33, S - 6, 2], [16.5, S + 14.25, 3]],
           'sub_pixel': [[7.2, 7.3, 1], [7.8, 7.4, 1], [7.5, 7.9, 1]],
           'whole_patch': [[-S, -S, 1], [3 * S, -S, 2], [-S, 3 * S, 3]]}[name]
    faces = [[0, 1, 3]] if name == 'index_nv' else [[0, 1, 2]]          # Nv = 3: index 3 is one past the end
    return _fix(tri, faces, S, background=0.25)


def crowded(F=700, seed=11):
    """F small faces whose boxes all meet the tile of pixels 16..31 x 16..31 at size 48: more than two compaction chunks, and F
    is no multiple of the chunk.  Every face spans at least two pixels each way (its box holds a pixel centre), the faces
    overlap a lot, and their order in depth is random against their index."""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.uniform(17.0, 30.0, (F, 1, 2))
    d = rng.uniform(-2.5, 2.5, (F, 3, 2))
    d[:, 0] = rng.uniform(-2.5, -1.0, (F, 2))
    d[:, 1, 0], d[:, 2, 1] = rng.uniform(1.0, 2.5, F), rng.uniform(1.0, 2.5, F)
    xy = np.round((c + d) * 8) / 8
    z = (rng.permutation(F * 3).reshape(F, 3) + 1) / 64.0
    v = np.concatenate([xy, z[..., None]], -1).reshape(F * 3, 3)
    rgb = rng.uniform(0.1, 1.0, (F, 3))
    assert F > 2 * CHUNK and F % CHUNK
    return _fix(v, np.arange(F * 3).reshape(F, 3), 48, face_rgb=rgb, ambient=0.35, light=(0.3, -0.5, -0.8))


def _ellipsoid(n_lat, n_lon, radii):
    """Closed latitude-longitude mesh: 2 poles + (n_lat - 1) rings of n_lon vertices; 2 n_lon (n_lat - 1) faces."""
    v = [[0, 0, radii[2]]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            v.append([radii[0] * np.sin(th) * np.cos(ph), radii[1] * np.sin(th) * np.sin(ph), radii[2] * np.cos(th)])
    v.append([0, 0, -radii[2]])
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    f = []
    for j in range(n_lon):
        f.append([0, ring(1, j), ring(1, j + 1)])
        f.append([len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            f.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    return np.array(v, np.float64), np.array(f, np.int32)


def _rot(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


ELLIPSOID_SEED = 3


@functools.lru_cache(maxsize=None)
def ellipsoids(size, coloured, ambient, seed=ELLIPSOID_SEED):
    """A closed ellipsoid of 2 * 24 * 17 = 816 faces and a smaller one of 2 * 12 * 7 = 168 poking through it (984 faces), B = 3
    with another rotation and offset per sample, in units of the patch size: partly off the patch in one sample."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v1, f1 = _ellipsoid(18, 24, (0.34, 0.22, 0.28))
    v2, f2 = _ellipsoid(8, 12, (0.12, 0.45, 0.1))
    faces = np.concatenate([f1, f2 + len(v1)])
    verts = []
    for b in range(3):
        R = _rot(rng)
        off = np.array([0.5, 0.5, 0.0]) + rng.uniform(-0.12, 0.12, 3) + (np.array([0.3, 0.0, 0.0]) if b == 2 else 0.0)
        v = np.concatenate([v1, v2 + rng.uniform(-0.05, 0.05, 3)]) @ R.T + off
        verts.append(v * size)
    rgb = rng.uniform(0.1, 1.0, (len(faces), 3)) if coloured else None
    return _fix(np.stack(verts), faces, size, face_rgb=rgb, ambient=ambient, light=(-0.4, -0.6, -0.7), depth_scale=0.75)


ELLIPSOID_CASES = [(16, False, 0.35), (16, True, 1.0), (40, True, 0.35), (40, False, 1.0), (64, True, 0.35), (64, False, 0.35), (64, True, 1.0)]


def render_args(fix):
    return {k: fix[k] for k in ('verts', 'faces', 'face_rgb', 'light', 'ambient', 'depth_scale', 'background', 'size')}
