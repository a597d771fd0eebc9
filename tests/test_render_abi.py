"""xas_mesh_render without a GPU: the two symbols are exported, declared under their comment and bound with a matching
argument list; the workspace size grows with B and F; every argument error answers with a status and a message before any
launch; B == 0 is valid and touches nothing."""
import ctypes
import inspect
import re
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, WS = 'xas_mesh_render', 'xas_mesh_render_workspace_bytes'
SIG, WS_SIG = ('ppppfffiiiipppppp', 'i'), ('iii', 'z')


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib, ops_render
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in ((NAME, SIG), (WS, WS_SIG)):
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
    assert len(_lib.fn(NAME).argtypes) == 17
    src = open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()
    decl = re.search(r'/\*((?:(?!\*/).)*)\*/\s*size_t\s+%s\s*\([^)]*\);\s*int\s+%s\s*\(' % (WS, NAME), src, re.S)
    assert decl, 'include/xas_hip.h does not declare the renderer under its comment'
    for phrase in ('double precision', 'no fused multiply-add', 'COVERED', 'closed box', 'z < best', 'smallest face index', 'SKIPPED',
                   'rounded once', 'every element written', 'no atomics', 'bit for bit', 'in face order', 'No back-face culling'):
        assert phrase.lower() in decl.group(1).lower(), 'the specification does not fix %r' % phrase
    assert _lib.fn('xas_abi_version')() == 3 == _lib.ABI_VERSION
    p = inspect.signature(ops_render.render_mesh).parameters
    assert list(p) == ['verts', 'faces', 'face_rgb', 'light', 'ambient', 'depth_scale', 'background', 'size', 'want']
    assert [p[n].default for n in list(p)[2:]] == [None, None, 0.35, 1.0, 0.0, 256, ('img', 'mask')]
    assert len(ops_render.PART_PALETTE) == 24 == len(set(ops_render.PART_PALETTE))
    assert all(len(c) == 3 and all(0 <= v <= 1 for v in c) for c in ops_render.PART_PALETTE)


def test_workspace_size_is_monotone():
    from xas_amd import _lib
    ws = _lib.fn(WS)
    assert ws(0, 100, 16) == 0 and ws(2, 0, 16) == 0 and ws(-1, 5, 16) == 0 and ws(2, -5, 16) == 0
    sizes = [[ws(B, F, 256) for F in (1, 7, 256, 257, 1000, 13776)] for B in (1, 2, 3, 32)]
    for row in sizes:
        assert all(a < b for a, b in zip(row, row[1:]))
    for lo, hi in zip(sizes, sizes[1:]):
        assert all(a < b for a, b in zip(lo, hi))
    assert ws(32, 13776, 256) >= 32 * 13776 * 72 and ws(32, 13776, 256) == ws(32, 13776, 64)      # per face and sample: box + record
    assert ws(1, 1, 16) % 16 == 0


def test_argument_errors_return_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    f = _lib.fn(NAME)
    one = ctypes.c_void_p(64)                      # aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()

    def call(B=2, Nv=5, F=3, S=16, verts=one, faces=one, img=one, mask=one, ws=one):
        return f(verts, faces, None, None, 0.35, 1.0, 0.0, B, Nv, F, S, img, mask, None, None, ws, None)
    for bad in (0, -3, 4097):
        assert call(S=bad) == 1 and 'S=%d' % bad in err()
    assert call(B=-1) == 1 and 'B=-1' in err()
    assert call(F=-2) == 1 and 'F=-2' in err()
    assert call(Nv=-1) == 1 and 'Nv=-1' in err()
    assert call(B=65536) == 1 and 'B <= 65535' in err()
    assert call(B=40000, F=60000) == 1 and 'B*F < 2^31' in err()
    for name in ('verts', 'faces', 'img', 'mask'):
        assert call(**{name: None}) == 1 and 'null buffer' in err(), name
    assert call(ws=None) == 1 and 'null workspace' in err()
    assert call(ws=ctypes.c_void_p(68)) == 1 and '16-byte aligned' in err()
    assert call(F=0, img=None) == 1 and 'null buffer' in err()
    # B == 0 is valid and returns before anything is looked at, the null pointers included
    assert call(B=0, verts=None, faces=None, img=None, mask=None, ws=None) == 0
