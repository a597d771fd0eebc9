"""World -> patch entries of the C ABI and the SMPL-side names of modules.util, without a GPU: the symbols exist with the
table's signatures, bad arguments come back as errors before any launch, and the mirror defines the functions itself."""
import ctypes
import inspect
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'x-as-supervision_amd')
FWD, BWD = 'xas_world_to_patch_fwd', 'xas_world_to_patch_bwd'


def test_symbols_and_signatures():
    from test_abi import header_prototypes
    from xas_amd import _lib, ops_head
    lib = _lib.load()
    protos = header_prototypes()
    assert _lib.SIGNATURES[FWD] == ('ppfipppppiiiffipp', 'i') == protos[FWD]
    assert _lib.SIGNATURES[BWD] == ('pppfipppppiiiffippp', 'i') == protos[BWD]
    for name in (FWD, BWD):
        assert hasattr(lib, name), 'library does not export %s' % name
        f = _lib.fn(name)
        assert len(f.argtypes) == len(_lib.SIGNATURES[name][0]) and f.restype is ctypes.c_int
    src = open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()
    for flag, value in (('XAS_GEO_NORM', ops_head.GEO_NORM), ('XAS_GEO_IMAGE', ops_head.GEO_IMAGE), ('XAS_GEO_WORLD', ops_head.GEO_WORLD)):
        assert '#define %s %d' % (flag, value) in src
    assert lib.xas_abi_version() == 3 == _lib.ABI_VERSION


def test_bad_arguments_return_errors_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                       # any non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    fwd, bwd = _lib.fn(FWD), _lib.fn(BWD)
    cams = (one, one, one, one, one)
    tail = (256.0, 2000.0, 1)
    assert fwd(None, None, 1.0, 0, *cams, 2, 1, 18, *tail, one, None) == 1 and 'null buffer' in err()
    assert fwd(one, None, 1.0, 0, *cams, 2, 1, 18, *tail, None, None) == 1 and 'null buffer' in err()
    assert fwd(one, None, 1.0, 0, one, one, one, None, one, 2, 1, 18, *tail, one, None) == 1 and 'null buffer' in err()
    assert fwd(one, None, 1.0, 0, None, one, one, one, one, 2, 1, 18, *tail, one, None) == 1 and 'crop' in err()
    assert fwd(one, None, 1.0, 1, one, one, None, one, one, 2, 1, 18, 256.0, 2000.0, 8, one, None) == 1 and 'pelvis' in err()
    for shape in ((0, 1, 18), (-3, 1, 18), (2, 0, 18), (2, 1, 0), (1 << 20, 1 << 10, 18)):
        assert fwd(one, None, 1.0, 0, *cams, *shape, *tail, one, None) == 1 and 'bad shape' in err(), shape
        assert bwd(one, one, None, 1.0, 0, *cams, *shape, *tail, one, None, None) == 1 and 'bad shape' in err(), shape
    assert fwd(one, None, 1.0, 0, *cams, 2, 1, 18, 256.0, 2000.0, 2, one, None) == 1 and 'unknown flag' in err()
    assert bwd(None, one, None, 1.0, 0, *cams, 2, 1, 18, *tail, one, None, None) == 1 and 'null buffer' in err()
    assert bwd(one, None, None, 1.0, 0, *cams, 2, 1, 18, *tail, one, None, None) == 1 and 'null buffer' in err()
    assert bwd(one, one, None, 1.0, 0, *cams, 2, 1, 18, *tail, None, None, None) == 1 and 'null buffer' in err()
    assert bwd(one, one, one, 1.0, 0, *cams, 2, 1, 18, *tail, one, None, None) == 1 and 'grad_pre_rot' in err()
    assert bwd(one, one, None, 1.0, 0, *cams, 2, 1, 18, *tail, one, one, None) == 1 and 'grad_pre_rot' in err()


def test_op_refuses_cpu_tensors_and_bad_shapes():
    import pytest
    import torch
    from xas_amd import ops_head
    x = {'cam_0_' + k: torch.zeros(s) for k, s in (('trans_image', (2, 2, 3)), ('k_mat', (2, 3, 3)), ('pelvis', (2, 3)),
                                                 ('rot_world', (2, 3, 3)), ('trans_world', (2, 3)), ('img', (2, 3, 256, 256)))}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops_head.world_to_patch(torch.zeros(2, 18, 3), x, 'cam_0')
    with pytest.raises(RuntimeError, match='points must be'):
        ops_head.world_to_patch(torch.zeros(2, 18, 2), x, 'cam_0')
    with pytest.raises(RuntimeError, match='pre_rot must be'):
        ops_head.world_to_patch(torch.zeros(2, 18, 3), x, 'cam_0', pre_rot=torch.zeros(3, 3))


def test_mirror_defines_the_smpl_side_itself():
    """In a child interpreter with nothing but the mirror on the path (no reference behind it): the three names are the
    mirror's own functions, with the reference's signatures, and the world -> patch names are still not defined there."""
    code = ("import sys, os, inspect, json; sys.path.insert(0, %r)\n"
            "import modules.util as u\n"
            "out = {}\n"
            "for n in ('project_smpl_to_patch_kps', 'convert_pelvis_to_world', 'flip_3D'):\n"
            "    f = vars(u)[n]\n"
            "    out[n] = [f.__module__, os.path.realpath(inspect.getsourcefile(f)), list(inspect.signature(f).parameters)]\n"
            "out['own'] = [n for n in ('convert_world_to_patch', 'convert_world_to_image', 'convert_image_to_patch') if n in vars(u)]\n"
            "print('RESULT ' + json.dumps(out))\n") % PKG
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd='/tmp', timeout=150,
                       env=dict(os.environ, PYTHONPATH='', PYTHONDONTWRITEBYTECODE='1'))
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
    want = {'project_smpl_to_patch_kps': ['global_rot_params', 'pose_params', 'shape_params', 'smpl_layer', 'h36m_regressor',
                                          'x', 'mode', 'convert_verts'],
            'convert_pelvis_to_world': ['x', 'mode'], 'flip_3D': ['keypoints']}
    for name, params in want.items():
        module, path, got = out[name]
        assert module == 'modules.util' and path == os.path.realpath(os.path.join(PKG, 'modules', 'util.py')), (name, module, path)
        assert got == params, (name, got)
    assert out['own'] == []
    from modules import util
    assert inspect.signature(util.project_smpl_to_patch_kps).parameters['convert_verts'].default is False

