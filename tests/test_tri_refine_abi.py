"""The reprojection-error refinement without a GPU: the entry point is exported, declared in include/xas_hip.h under its
comment and bound by the ctypes table with a matching argument list; its argument checks answer before any launch and name the
limit; eval.py knows --tri-refine and --tri-huber and leaves the older flags as they were; and the inputs of every case of
tests/test_gpu_tri_refine.py are validated here with the oracle alone: the condition number of every compared joint, what the
cases claim about themselves, and the oracle's own self-checks."""
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
NAME = 'xas_triangulate_refine'
SIG = ('ppppiiiifippppp', 'i')


def _header():
    return open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()


def test_symbol_is_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib, ops_eval
    lib = _lib.load()
    assert hasattr(lib, NAME), 'library does not export %s' % NAME
    protos = header_prototypes()
    assert NAME in protos and protos[NAME] == SIG
    assert _lib.SIGNATURES[NAME] == SIG
    assert len(_lib.fn(NAME).argtypes) == 15
    decl = re.search(r'/\*((?:(?!\*/).)*)\*/\s*#define XAS_REFINE_WEIGHTED (\d+)[^\n]*\n\s*int\s+%s\s*\(' % NAME, _header(), re.S)
    assert decl, 'include/xas_hip.h does not declare %s under its comment and flag' % NAME
    spec = decl.group(1)
    for phrase in ('in double', 'lambda diag(H)', 'lambda = 1e-3', 'lambda *= 0.1', 'lambda *= 10', 'strictly decreases', '1e-5',
                   'lambda > 1e12', 'PASSED THROUGH', 'bit for bit', 'mm^2', 'C(out) <= C(init)'):
        assert phrase in spec, 'the specification does not fix %r' % phrase
    assert int(decl.group(2)) == 1 == ops_eval.REFINE_WEIGHTED
    p = inspect.signature(ops_eval.triangulate_refine).parameters
    assert list(p) == ['points', 'pmat', 'init', 'views', 'weighted', 'huber_px', 'max_iter', 'want']
    assert (p['views'].default, p['weighted'].default, p['huber_px'].default, p['max_iter'].default, p['want'].default) == (
        None, False, 0.0, 20, ('resid',))


def test_abi_version_is_unchanged():
    from xas_amd import _lib
    assert _lib.fn('xas_abi_version')() == 3 == _lib.ABI_VERSION


def test_argument_checks_return_errors_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)                       # any aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    f = _lib.fn(NAME)
    #        points P  init views B  V  K  flags huber iters out resid cov status stream
    call = lambda V=4, B=2, K=5, flags=0, iters=20, bufs=(one, one, one, one): f(
        bufs[0], bufs[1], bufs[2], None, B, V, K, flags, 0.0, iters, bufs[3], None, None, None, None)
    assert call(V=1) == 1 and 'V=1 views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6)' in err()
    assert call(V=7) == 1 and 'V=7 views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6)' in err()
    assert call(B=0) == 1 and 'bad shape B=0 K=5' in err()
    assert call(K=0) == 1 and 'bad shape B=2 K=0' in err()
    assert call(B=1 << 16, K=1 << 15) == 1 and 'B*K < 2^31' in err()
    for bad in (0, -1, 65):
        assert call(iters=bad) == 1 and 'max_iter=%d trials (needs 1 <= max_iter <= 64)' % bad in err()
    for i in range(4):
        bufs = [one] * 4
        bufs[i] = None
        assert call(bufs=bufs) == 1 and 'null buffer (points, P, init and out are required)' in err()
    for bad in (2, 3, 1 << 30, -2):
        assert call(flags=bad) == 1 and 'unknown flag bits' in err()


def test_eval_knows_the_flags_and_leaves_the_others_alone():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'eval.py'), '--help'], capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr
    assert '--tri-refine {none,lm}' in r.stdout and '--tri-huber PX' in r.stdout
    import eval as xeval
    from xas_amd import ops_eval
    cli = dict(xeval.CLI)
    assert cli['--tri-refine']['default'] == 'none' and cli['--tri-refine']['choices'] == ['none', 'lm']
    assert cli['--tri-huber']['default'] == 0.0 and cli['--tri-huber']['type'] is float
    # the older flags, word for word
    assert cli['--tri'] == dict(default='dlt', choices=['dlt', 'robust'], help='triangulation: the DLT over all cameras, or over '
                                'the largest set of cameras that agree within --tri_thresh')
    assert cli['--resolve'] == dict(default='gt', choices=['gt', 'views'], help='left/right exchange and depth hypothesis of every '
                                    'view: by the labels as the reference does, or by the agreement of the cameras (labels only '
                                    'name each pair; --multi_hypo is ignored)')
    assert cli['--tri-weight'] == dict(default='depth', choices=['depth', 'spread'], dest='tri_weight', help="weight of every view "
                                       "in the triangulation and in --resolve views: the joint's depth in mm as the reference has "
                                       'it, or 1 / sigma of its heat-map in image pixels')
    p = inspect.signature(xeval.Eval.__init__).parameters
    assert list(p) == ['self', 'config', 'detector', 'eval_data', 'log_dir', 'img_size', 'flip_test', 'tri', 'tri_thresh', 'resolve']
    assert 'tri_refine' not in p and 'tri_huber' not in p
    assert p['tri'].default == 'dlt' and p['tri_thresh'].default == ops_eval.TRI_ROBUST_PX and p['resolve'].default == 'gt'


def test_util_signatures_are_unchanged_and_the_new_one_stands_beside_them():
    from modules import util as mu
    p = inspect.signature(mu.batch_triangulate).parameters
    assert list(p) == ['keypoints_', 'Pall', 'robust_px'] and p['robust_px'].default is None
    p = inspect.signature(mu.triangulation).parameters
    assert list(p) == ['keypoints', 'params', 'cam_id_list', 'is_norm', 'RECT_WIDTH', 'robust_px', 'return_inliers']
    p = inspect.signature(mu.triangulation_weighted).parameters
    assert list(p) == ['keypoints', 'params', 'cam_id_list', 'weights', 'is_norm', 'RECT_WIDTH', 'robust_px', 'return_inliers', 'inputs']
    p = inspect.signature(mu.triangulation_refined).parameters
    assert list(p) == ['keypoints', 'params', 'cam_id_list', 'weights', 'is_norm', 'RECT_WIDTH', 'robust_px', 'huber_px', 'want', 'inputs']
    assert [p[n].default for n in list(p)[3:]] == [None, True, 2000, None, 0.0, (), None]


def _names():
    import test_gpu_tri_refine as t
    return list(t.CASES)


@pytest.mark.parametrize('name', _names())
def test_gpu_case_inputs_are_well_conditioned(name):
    """Every case of the GPU file: each joint whose position is compared has cond <= 1e3, no case but the one built to be
    ill-conditioned excludes a joint on that ground, the oracle's minimum costs no more than the DLT start, and what the cases
    claim about themselves."""
    import test_gpu_tri_refine as t
    import _refine_oracle as ro
    c, o = t.case(name)
    B, V, K, _ = c['points'].shape
    solved = ~o['passed']
    cmp = t.compared(name)
    excluded = solved & ~cmp
    print('%s: B=%d V=%d K=%d, %d passed through, %d excluded, cond max %.3g' % (
        name, B, V, K, o['passed'].sum(), excluded.sum(), np.nanmax(o['cond']) if solved.any() else np.nan))
    assert (o['cond'][cmp] <= ro.COND_MAX).all()
    if name == 'illcond':
        assert excluded.all() and (o['cond'] > ro.COND_MAX).all()
    else:
        assert not excluded.any(), 'share excluded: %.3g' % excluded.mean()
    assert (o['C'][solved] <= o['C_init'][solved]).all()                      # C(oracle) <= C(DLT)
    assert np.array_equal(o['passed'], np.ones((B, K), bool)) == (name in t.PASSED_THROUGH)
    # 3-5 m from a subject of about 1 m
    centre = -np.einsum('bvij,bvj->bvi', np.linalg.inv(c['P'][..., :3].astype(np.float64)), c['P'][..., 3].astype(np.float64))
    dist = np.linalg.norm(centre, axis=-1)
    assert 2900 < dist.min() and dist.max() < 5200 and np.abs(c['world']).max() < 1600
    if name in t.CLEAN:
        assert (np.linalg.norm(o['xyz'] - c['world'], axis=-1) <= t.planted_tol(c, o)).all()    # the planted point
        assert o['resid'].max() < 1e-3
    if name in t.NOISY:
        assert 0.2 < np.sqrt((o['resid'][..., 0] ** 2).mean()) < 2 * t.SIGMA_PX * np.sqrt(2)
    if name == 'nan_init':
        assert o['passed'].sum() == 3 and o['passed'][0, 1] and o['passed'][1, 3] and o['passed'][1, 4]
    if name == 'mask_2of4':
        assert np.array_equal(o['used'], c['views']) and all(bin(int(m)).count('1') == 2 for m in c['views'].ravel())
    if name == 'robust':
        import _tri_oracle as to
        to.check_decidable(c['robust'], name)
        assert np.array_equal(o['used'], c['robust']['used']) and np.array_equal(c['robust']['mask'], 15 & ~c['planted'])


def test_oracle_claims_of_the_weighted_and_huber_cases():
    import test_gpu_tri_refine as t
    import _refine_oracle as ro
    c, o = t.case('weighted')
    w = c['points'][..., 2]
    assert 9.0 < w.max() / w.min() < 12.0                                     # weights spanning 10x
    plain = ro.refine(c['points'], c['P'], c['init'], None, False, 0.0)
    tol = 1e-4 + 2 * t.ulp32(np.abs(o['xyz']).max(-1))
    assert (np.abs(o['xyz'] - plain['xyz']).max(-1) > 10 * tol).all()
    c, o = t.case('huber')
    c0, o0 = t.case('huber_off')
    assert np.array_equal(c['points'], c0['points']) and c['huber'] == 3.0 and c0['huber'] == 0.0
    d, d0 = np.linalg.norm(o['xyz'] - c['world'], axis=-1), np.linalg.norm(o0['xyz'] - c['world'], axis=-1)
    print('huber: %.3g mm off the planted point at most, %.3g mm without' % (d.max(), d0.max()))
    assert (d < d0).all()
    # one view of every joint is 40 px off: its residual at the minimum is in Huber's linear part, the others' are not all
    assert (o['resid'][..., 1] > 3.0).all()


def test_oracle_minimum_is_a_minimum():
    """Independent of its own minimiser: scipy-free, by probing.  At the returned point no step of 1e-3 mm along an axis lowers
    the cost, and the gradient is 1e-8 of the start's or less (noisy cases, where float64 resolves it)."""
    import test_gpu_tri_refine as t
    import _refine_oracle as ro
    for name in ('noisy_b2v4k5', 'weighted', 'huber', 'mask_2of4'):
        c, o = t.case(name)
        for b in range(c['points'].shape[0]):
            for k in range(c['points'].shape[2]):
                F = ro.views_used(c['points'][b, :, k], 0 if c['views'] is None else int(c['views'][b, k]))
                args = (c['points'][b, :, k], c['P'][b])
                C, _, _, g, _ = ro.terms(*args, o['xyz'][b, k], F, c['weighted'], c['huber'])
                g0 = ro.terms(*args, c['init'][b, k, :3].astype(np.float64), F, c['weighted'], c['huber'])[3]
                assert np.linalg.norm(g) <= 1e-8 * np.linalg.norm(g0)
                for d in np.concatenate([np.eye(3), -np.eye(3)]) * 1e-3:
                    assert ro.terms(*args, o['xyz'][b, k] + d, F, c['weighted'], c['huber'])[0] > C


def test_restated_schedule_agrees_with_the_minimiser_where_it_converges():
    """The header's loop in float64 (_refine_oracle.schedule) against the independent minimiser: the same point within the
    position tolerance wherever the loop stopped on its step rule; status 0 on noise-free points, 1 after a single trial, 2 where
    the oracle passes through; and under Huber's loss 64 trials reach the minimum where the default 20 may not."""
    import test_gpu_tri_refine as t
    import _refine_oracle as ro
    sched = lambda c, n=20: ro.schedule(c['points'], c['P'], c['init'], c['views'], c['weighted'], c['huber'], max_iter=n)
    for name in ('clean_b2v4k5', 'noisy_b2v4k5', 'weighted', 'mask_2of4', 'nan_init', 'one_valid'):
        c, o = t.case(name)
        s = sched(c)
        assert np.array_equal(s['status'] == 2, o['passed']), name
        done = s['status'] == 0
        assert (np.abs(s['xyz'][done] - o['xyz'][done]).max(-1) <= 1e-4).all(), name
        if name.startswith('clean'):
            assert done.all()
    c, o = t.case('noisy_b2v4k5')
    assert (sched(c, 1)['status'] == 1).all()
    c, o = t.case('huber')
    far, near = sched(c, 20), sched(c, 64)
    d = lambda s: np.abs(s['xyz'] - o['xyz']).max(-1)
    print('huber: the loop stands %.3g mm from the minimum after 20 trials at most, %.3g mm after 64 (trials used: %d)' % (
        d(far).max(), d(near).max(), near['trials'].max()))
    assert (d(near) <= 1e-4).all() and near['trials'].max() < 64
    assert (d(far) >= d(near) - 1e-9).all()
