"""The label-free resolution without a GPU: xas_multiview_resolve is exported, declared in include/xas_hip.h under its comment
and bound by the ctypes table with a matching argument list; its argument checks answer before any launch and name the limit;
eval.py knows --resolve and leaves --tri as it was; and the inputs of every case of tests/test_gpu_resolve.py meet the oracle's
decidability condition, so that they are validated here before any GPU visit."""
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
NAME = 'xas_multiview_resolve'
TRI_HELP = 'triangulation: the DLT over all cameras, or over the largest set of cameras that agree within --tri_thresh'


def _header():
    return open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()


def test_symbol_is_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, NAME), 'library does not export %s' % NAME
    protos = header_prototypes()
    assert NAME in protos and protos[NAME] == ('ppppppiiiifpppppp', 'i')
    assert _lib.SIGNATURES[NAME] == protos[NAME]
    assert len(_lib.fn(NAME).argtypes) == 17
    decl = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(' % NAME, _header(), re.S)
    assert decl, 'include/xas_hip.h does not declare %s under its comment' % NAME
    for cite in ('eval_utils.py:7-29', 'eval.py:129-148', 'modules/util.py:198-230'):      # what it stands beside
        assert cite in decl.group(1), cite
    assert re.search(r'#define XAS_EVAL_NO_SWITCH 8\b', _header())
    from xas_amd import ops_eval
    assert ops_eval.EVAL_NO_SWITCH == 8
    assert not ops_eval.EVAL_NO_SWITCH & (ops_eval.EVAL_CONFIDENT | ops_eval.EVAL_SWITCH_ALL | ops_eval.EVAL_GT_NORMALISED)


def test_abi_version_is_unchanged():
    from xas_amd import _lib
    assert _lib.fn('xas_abi_version')() == 3 == _lib.ABI_VERSION


def test_argument_checks_return_errors_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)                       # any aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    f = _lib.fn(NAME)

    def call(B=2, V=4, Hy=3, K=5, size=256.0, sel=one, bufs=(one,) * 5, gt=None):
        #        points P kps world perm  gt  B  V  Hy  K  size  sel  xyzw swap hyp named stream
        return f(*bufs, gt, B, V, Hy, K, size, sel, one, one, one, None, None)

    assert call(V=1) == 1 and 'V=1 views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6)' in err()
    assert call(V=7) == 1 and 'V=7 views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6)' in err()
    assert call(K=65) == 1 and 'K=65 joints (needs 1 <= K <= 64)' in err()
    assert call(K=0) == 1 and 'K=0 joints (needs 1 <= K <= 64)' in err()
    assert call(sel=None) == 1 and 'null buffer (points, P, kps, world, perm and sel are required)' in err()
    for i in range(5):
        assert call(bufs=tuple(None if j == i else one for j in range(5))) == 1 and 'null buffer' in err()
    assert call(B=0) == 1 and 'bad shape B=0 K=5 (B > 0, B*K < 2^31)' in err()
    assert call(B=1 << 26, K=64) == 1 and 'B*K < 2^31' in err()
    assert call(Hy=0) == 1 and 'Hy=0 hypotheses (needs 1 <= Hy <= 255)' in err()
    assert call(Hy=256) == 1 and 'Hy=256 hypotheses' in err()
    assert call(gt=one, size=1.0) == 1 and 'image_size' in err()


def test_eval_knows_the_flag_and_defaults_to_gt():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'eval.py'), '--help'], capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr
    text = ' '.join(r.stdout.split())
    assert '--resolve {gt,views}' in text and '--tri {dlt,robust}' in text
    assert TRI_HELP in text                                                   # the --tri help text is unchanged
    assert 'ignored with --resolve views' in text
    import eval as xeval
    cli = dict(xeval.CLI)
    assert cli['--resolve']['default'] == 'gt' and cli['--resolve']['choices'] == ['gt', 'views']
    assert cli['--tri']['help'] == TRI_HELP and cli['--tri']['default'] == 'dlt'
    assert cli['--multi_hypo']['default'] == 'best'
    p = inspect.signature(xeval.Eval.__init__).parameters
    assert list(p)[-1] == 'resolve' and p['resolve'].default == 'gt'
    assert list(p)[:-1] == ['self', 'config', 'detector', 'eval_data', 'log_dir', 'img_size', 'flip_test', 'tri', 'tri_thresh']


def test_host_signatures():
    from modules import util as mu
    from xas_amd import ops_eval
    p = inspect.signature(mu.resolve_views).parameters
    assert list(p) == ['kps_by_cam', 'params', 'cam_id_list', 'pairs', 'gt', 'RECT_WIDTH']
    assert p['gt'].default is True and p['RECT_WIDTH'].default == 2000
    p = inspect.signature(ops_eval.multiview_resolve).parameters
    assert list(p) == ['points', 'pmat', 'kps', 'world', 'pairs', 'gt', 'image_size', 'want']
    assert p['pairs'].default == ops_eval.SWITCH_PAIRS and p['gt'].default is None and p['image_size'].default == 256.0
    p = inspect.signature(ops_eval.eval_select).parameters
    assert list(p)[-1] == 'no_switch' and p['no_switch'].default is False


def _case_names():
    import test_gpu_resolve as t
    return [(n, False) for n in t.CASES] + [(n, True) for n in t.WITH_GT]


@pytest.mark.parametrize('name,gt', _case_names())
def test_gpu_case_inputs_are_decidable(name, gt):
    """Every case of the GPU file, without and (where the GPU file passes them) with labels: the oracle's condition, and what
    the cases claim about themselves."""
    import _resolve_oracle as ro
    import test_gpu_resolve as t
    c, o = t.case(name, gt)
    margins = ro.check_decidable(o, name)
    B, V, K, _ = c['points'].shape
    assert 2 <= V <= 6 and K <= 64 and B == 2
    print('%s%s: B=%d V=%d K=%d Hy=%d, margins (px^2, rel, mm, naming) %s' % (name, ' +gt' if gt else '', B, V, K, c['kps'].shape[2], margins))
    paired = np.array(c['perm']) != np.arange(K)
    full = (1 << V) - 1
    if name in t.CLEAN + t.PLANTED + ('k64', 'k1', 'hy1', 'identity', 'eval') or (name == 'anchor' and gt):
        assert np.array_equal(o['swap'], c['planted'])
        assert np.array_equal(o['sel'], t.truth(c))
        assert np.array_equal(o['hyp'], np.broadcast_to(c['slot'], o['hyp'].shape))
        assert np.linalg.norm(o['xyz'] - c['wp'], axis=-1).max() < t.WORLD_TOL_MM
    if name in t.PLANTED:
        assert (c['planted'] != 0).any() and not (c['planted'] & 1).any()
        assert np.bitwise_or.reduce(c['planted'].ravel()) == full & ~1       # every view but the anchor carries an exchange
    if name == 'anchor':
        assert (c['planted'][:, paired] & 1).all()
        if not gt:
            assert np.array_equal(o['swap'][:, paired], c['planted'][:, paired] ^ full)
            assert np.array_equal(o['sel'], t.truth(c)[:, :, c['perm']])
        else:
            assert np.array_equal(o['named'], np.broadcast_to(paired, o['named'].shape).astype(np.uint8))
    if name == 'coincident':
        assert (o['swap'] == 0).all() and np.isinf(o['cost_gap'][:, [1, 4]]).all() and np.isfinite(o['cost_gap'][:, [0, 2]]).all()
    if name == 'dead_view':
        assert np.array_equal(o['swap'], c['planted']) and not (o['swap'] & 4).any() and o['valid'][1, 0] == 0b1010
        assert not gt or not o['named'].any()
    if name == 'one_valid':
        assert np.isnan(o['xyz']).all() and not o['swap'].any() and not o['hyp'].any() and np.isnan(o['w'][1, 3])
    if name == 'eval':
        assert (c['planted'][1, [1, 2, 3]] & 1).all() and not (c['planted'][0] & 1).any()
        assert not gt or (o['named'][1, [1, 2, 3, 4, 5, 6]].all() and o['named'].sum() == 6)


def test_oracle_is_the_plain_dlt_for_unpaired_joints():
    import _resolve_oracle as ro
    import _tri_oracle as to
    import test_gpu_resolve as t
    c, o = t.case('identity')
    assert np.abs(to.dlt(c['points'], c['P']) - o['xyz']).max() < 1e-9
    assert np.isinf(o['cost_gap']).all() and (o['valid'] == 15).all()


def test_eval_case_is_what_the_labels_choose():
    """The eval case on the CPU: the reference's selection by the labels ('best') returns, per camera, exactly what the
    oracle's label-free resolution returns, and hypothesis 0 ('confident') does not."""
    import torch
    import test_gpu_resolve as t
    from oracle import evalpath as ev
    x, c = t.eval_case()
    _, o = t.case('eval', True)
    differ = 0
    for i, cam in enumerate((0, 1, 2, 3)):
        kps, joints = torch.from_numpy(c['kps'][:, i]), x['cam_%d_joints' % cam]
        assert np.array_equal(ev.select_hypothesis(kps, joints, 'best')[0].numpy(), o['sel'][:, i])
        differ += int(not np.array_equal(ev.select_hypothesis(kps, joints, 'confident')[0].numpy(), o['sel'][:, i]))
    assert differ == 4
