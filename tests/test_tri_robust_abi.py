"""The robust triangulation without a GPU: the entry point is exported, declared in include/xas_hip.h and bound by the ctypes
table with a matching argument list; its argument checks answer before any launch and name the limit; eval.py knows --tri and
--tri_thresh; and the inputs of every case of tests/test_gpu_tri_robust.py meet the oracle's decidability condition, so that
they are validated here before any GPU visit."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'x-as-supervision_amd')
NAME = 'xas_triangulate_robust'


def _header():
    return open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()


def test_symbol_is_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, NAME), 'library does not export %s' % NAME
    protos = header_prototypes()
    assert NAME in protos and protos[NAME] == ('ppiiifpppp', 'i')
    assert _lib.SIGNATURES[NAME] == protos[NAME]
    assert len(_lib.fn(NAME).argtypes) == 10
    decl = re.search(r'/\*((?:(?!\*/).)*)\*/\s*#define XAS_TRI_MAX_VIEWS (\d+)\s*int\s+%s\s*\(' % NAME, _header(), re.S)
    assert decl, 'include/xas_hip.h does not declare %s under its comment and limit' % NAME
    assert 'modules/util.py:198-230' in decl.group(1)                # the comment says what it stands beside
    from xas_amd import ops_eval
    assert int(decl.group(2)) == 6 == ops_eval.TRI_MAX_VIEWS


def test_abi_version_is_unchanged():
    from xas_amd import _lib
    assert _lib.fn('xas_abi_version')() == 3 == _lib.ABI_VERSION


def test_argument_checks_return_errors_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)                       # any aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    f = _lib.fn(NAME)
    #        points P   B  V  K  thr   out  inliers resid stream
    assert f(one, one, 2, 1, 5, 20.0, one, one, one, None) == 1 and 'V=1 views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6)' in err()
    assert f(one, one, 2, 7, 5, 20.0, one, one, one, None) == 1 and 'V=7 views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6)' in err()
    for bad in (0.0, -1.0, float('nan')):
        assert f(one, one, 2, 4, 5, bad, one, None, None, None) == 1 and 'needs a threshold > 0 px' in err()
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert f(args[0], args[1], 2, 4, 5, 20.0, args[2], one, one, None) == 1 and 'null buffer' in err()
    assert f(one, one, 0, 4, 5, 20.0, one, one, one, None) == 1 and 'bad shape B=0 K=5' in err()
    assert f(one, one, 1 << 16, 4, 1 << 15, 20.0, one, one, one, None) == 1 and 'B*K < 2^31' in err()


def test_eval_knows_the_flags_and_defaults_to_dlt():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'eval.py'), '--help'], capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr
    assert '--tri {dlt,robust}' in r.stdout and '--tri_thresh PX' in r.stdout
    import eval as xeval
    from xas_amd import ops_eval
    cli = dict(xeval.CLI)
    assert cli['--tri']['default'] == 'dlt' and cli['--tri']['choices'] == ['dlt', 'robust']
    assert cli['--tri_thresh']['default'] == ops_eval.TRI_ROBUST_PX == 20.0
    p = inspect.signature(xeval.Eval.__init__).parameters
    assert p['tri'].default == 'dlt' and p['tri_thresh'].default == ops_eval.TRI_ROBUST_PX


def test_util_signatures_extend_the_reference_ones():
    from modules import util as mu
    p = inspect.signature(mu.batch_triangulate).parameters
    assert list(p) == ['keypoints_', 'Pall', 'robust_px'] and p['robust_px'].default is None
    p = inspect.signature(mu.triangulation).parameters
    assert list(p) == ['keypoints', 'params', 'cam_id_list', 'is_norm', 'RECT_WIDTH', 'robust_px', 'return_inliers']
    assert p['robust_px'].default is None and p['return_inliers'].default is False


def _case_names():
    import test_gpu_tri_robust as t
    return list(t.CASES) + ['eval']


@pytest.mark.parametrize('name', _case_names())
def test_gpu_case_inputs_are_decidable(name):
    """Every case of the GPU file: no residual of any candidate subset within 1 px of the threshold, and a best candidate with
    strictly more inliers than any candidate with another inlier set.  Also what the cases claim about themselves."""
    import _tri_oracle as to
    import test_gpu_tri_robust as t
    c, o = t.case(name)
    margin = to.check_decidable(o, name)
    B, V, K, _ = c['points'].shape
    full = (1 << V) - 1
    print('%s: B=%d V=%d K=%d, threshold margin %.3g px, count gap %s' % (name, B, V, K, margin, o['min_count_gap']))
    if name in t.CLEAN:
        assert (o['mask'] == full).all() and o['resid'].max() < 0.05
    if name in t.PLANTED:
        hit = c['planted'] != 0
        assert np.array_equal(o['mask'], full & ~c['planted'])
        assert np.linalg.norm(o['xyz'] - c['world'], axis=-1).max() < 0.5
        assert np.linalg.norm(to.dlt(c['points'], c['P']) - c['world'], axis=-1)[hit].min() > 5.0
    if name == 'inconsistent':
        assert (o['mask'] == 0).all() and (o['used'] == full).all()
    if name == 'eval':
        assert (o['mask'] != 0).all() and (o['mask'] != full).sum() >= B * K // 4


def test_oracle_is_the_plain_dlt_where_all_views_agree():
    """The restatement against the project's pinned oracle of the reference's DLT (oracle/evalpath.py, float32 SVD)."""
    import torch
    import _tri_oracle as to
    import test_gpu_tri_robust as t
    from oracle import evalpath as ev
    c, o = t.case('hm36_clean')
    want = ev.batch_triangulate(torch.from_numpy(c['points']), torch.from_numpy(c['P'])).numpy()
    assert np.abs(o['xyz'] - want[..., :3]).max() < 0.3              # the float32 SVD's own distance from the float64 solution
    np.testing.assert_allclose(o['w'], want[..., 3], rtol=1e-6)
    assert np.abs(to.dlt(c['points'], c['P']) - o['xyz']).max() < 1e-9
