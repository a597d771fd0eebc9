"""The flip test in the C ABI and the command line, without a GPU: the three entry points are exported by the built library,
declared in include/xas_hip.h (each under a comment that cites the reference lines it stands beside) and bound by the ctypes
table with matching argument lists; the argument checks answer before any launch; the pair table is checked on the host;
eval.py lists --flip and Eval takes flip_test."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'x-as-supervision_amd')
NAMES = ('xas_head_softargmax_flip_from_partials', 'xas_head_softargmax_fwd_flip', 'xas_nchw_to_nhwc_mirror_pair')
CODE = {'int': 'i', 'long': 'l', 'float': 'f', 'double': 'd', 'size_t': 'z', 'unsigned': 'u'}


def _header():
    return open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()


def _codes(params):
    """'const float* x, int B, ...' -> 'pi...' in the letters of _lib.SIGNATURES."""
    out = ''
    for p in params.split(','):
        p = re.sub(r'/\*.*?\*/', '', p).strip()
        out += 'p' if '*' in p else CODE[p.replace('const ', '').split()[0]]
    return out


@pytest.mark.parametrize('name', NAMES)
def test_symbol_is_exported_declared_and_bound(name):
    from xas_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name), 'library does not export %s' % name
    decl = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(([^;]*)\)\s*;' % name, _header(), re.S)
    assert decl, 'include/xas_hip.h does not declare %s under a comment' % name
    assert 'keypoint_detector_integral_multi.py:36-88' in decl.group(1)
    assert name in _lib.SIGNATURES
    args, ret = _lib.SIGNATURES[name]
    assert ret == 'i' and args == _codes(decl.group(2)), (args, _codes(decl.group(2)))
    assert len(_lib.fn(name).argtypes) == len(args)


def test_abi_version_is_unchanged():
    from xas_amd import _lib
    assert _lib.fn('xas_abi_version')() == 3 == _lib.ABI_VERSION


def test_argument_checks_return_errors_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)                       # any aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    f = _lib.fn('xas_head_softargmax_flip_from_partials')
    #        partial B  K  D  nchunk hy nb perm kps  z_idx dmap groups stream
    assert f(one, 1, 2, 10, 1, 3, 15, one, one, one, one, 1, None) == 1 and 'multiple of 4 in [4,128]' in err()
    assert f(one, 0, 2, 16, 1, 3, 15, one, one, one, one, 1, None) == 1 and 'need 0 < B' in err()
    assert f(one, 1, 0, 16, 1, 3, 15, one, one, one, one, 1, None) == 1 and 'K > 0' in err()
    assert f(one, 1, 2, 16, 1, 3, 15, None, one, one, one, 1, None) == 1 and 'null buffer' in err()
    assert f(None, 1, 2, 16, 1, 3, 15, one, one, one, one, 1, None) == 1 and 'null buffer' in err()
    assert f(one, 1, 2, 16, 0, 3, 15, one, one, one, one, 1, None) == 1 and 'null buffer' in err()
    assert f(one, 1, 2, 16, 1, 3, 15, one, one, None, one, 1, None) == 1 and 'z_idx required' in err()
    assert f(one, 1, 2, 16, 1, 7, 15, one, one, one, one, 1, None) == 1 and 'num_hypo' in err()
    assert f(one, 1, 2, 16, 1, 2, 0, one, one, one, one, 1, None) == 1 and 'single-hypothesis' in err()
    assert f(one, 3, 2, 16, 1, 3, 15, one, one, one, one, 2, None) == 1 and 'B=3 does not split into 2 groups' in err()
    g = _lib.fn('xas_head_softargmax_fwd_flip')
    #        logits B  K  D  hy nb perm kps  z_idx dmap groups partial stream
    assert g(one, 1, 2, 132, 3, 15, one, one, one, one, 1, one, None) == 1 and 'multiple of 4 in [4,128]' in err()
    assert g(one, -1, 2, 16, 3, 15, one, one, one, one, 1, one, None) == 1 and 'need 0 < B' in err()
    assert g(one, 1, 2, 16, 3, 15, one, one, one, one, 1, None, None) == 1 and 'null buffer' in err()
    assert g(one, 1, 2, 16, 3, 15, None, one, one, one, 1, one, None) == 1 and 'null buffer' in err()
    assert g(ctypes.c_void_p(68), 1, 2, 16, 3, 15, one, one, one, one, 1, one, None) == 1 and '16-byte aligned' in err()
    assert g(one, 2, 2, 16, 3, 15, one, one, one, one, 3, one, None) == 1 and 'does not split' in err()
    m = _lib.fn('xas_nchw_to_nhwc_mirror_pair')
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0)):
        assert m(one, *bad, ctypes.c_void_p(128), None) == 1 and 'bad arguments' in err()
    assert m(None, 1, 3, 8, 8, one, None) == 1 and m(one, 1, 3, 8, 8, None, None) == 1
    assert m(one, 1, 3, 8, 8, one, None) == 1                          # in place: the mirrored half would overwrite its source


def test_pair_table_is_checked_on_the_host():
    import torch
    from xas_amd import ops_head
    pairs = [[1, 4], [2, 5], [3, 6], [14, 11], [15, 12], [16, 13]]
    perm = ops_head.flip_perm(pairs, 18, 'cpu')
    assert perm.dtype == torch.int32
    assert perm.tolist() == [0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13, 17]
    assert ops_head.flip_perm([], 3, 'cpu').tolist() == [0, 1, 2]
    for bad in ([[1, 18]], [[-1, 2]], [[1, 2], [2, 3]], [[4, 4]]):
        with pytest.raises(RuntimeError, match='flip pair'):
            ops_head.flip_perm(bad, 18, 'cpu')
    hm = torch.zeros(2, 2 * 4, 4, 4)
    for bad in ([0, 2], [0, -1], [0], [0, 1, 1]):                        # refused before anything touches the device
        with pytest.raises(RuntimeError, match=r'perm must hold 2 joint indices in \[0, 2\)'):
            ops_head.softargmax_flip(hm, 2, 1, 0, bad)
    with pytest.raises(RuntimeError, match='followed by their B mirrors'):
        ops_head.softargmax_flip(torch.zeros(3, 2 * 4, 4, 4), 2, 1, 0, [1, 0])
    with pytest.raises(RuntimeError, match='inference path'):
        ops_head.softargmax_flip(hm.clone().requires_grad_(True), 2, 1, 0, [1, 0])


def test_eval_lists_the_flag_and_takes_the_argument():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'eval.py'), '--help'], capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr
    assert '--flip' in r.stdout and '--ema' in r.stdout
    import eval as xeval
    p = inspect.signature(xeval.Eval.__init__).parameters
    assert 'flip_test' in p and p['flip_test'].default is False
    assert dict(xeval.CLI)['--flip']['default'] is False
