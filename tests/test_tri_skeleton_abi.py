"""The skeleton-level refinement without a GPU: the entry point is exported, declared in include/xas_hip.h under its comment and
bound by the ctypes table with a matching argument list; its argument checks answer before any launch and name the limit; the
limb table is the training loss's; eval.py knows --tri-skeleton and --tri-sym and leaves --tri-refine as it was; and the inputs of every case of
tests/test_gpu_tri_skeleton.py are validated here with the oracle alone: which joints are free and which pairs active, the
condition number of every compared sample, and the two parts of the position tolerance (the stop rule's remainder from the
restated loop's convergence rate, and the cost's resolution)."""
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
NAME = 'xas_triangulate_skeleton'
SIG = ('pppppiiiiiffipppppp', 'i')


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
    assert len(_lib.fn(NAME).argtypes) == 19
    decl = re.search(r'/\*((?:(?!\*/).)*)\*/\s*#define XAS_SKEL_MAX_JOINTS (\d+)\s*#define XAS_SKEL_MAX_LIMBS (\d+)\s*int\s+%s\s*\(' % NAME,
                     _header(), re.S)
    assert decl, 'include/xas_hip.h does not declare %s under its comment and limits' % NAME
    spec = decl.group(1)
    for phrase in ('in double', 'lambda diag(H)', 'Cholesky', 'lambda = 1e-3', 'lambda *= 0.1', 'lambda *= 10', 'strictly decreases',
                   '1e-5', 'lambda > 1e12', 'FREE', 'FIXED', 'ACTIVE', 'bit for bit', '1e-9 mm', 'C(out) <= C(init)', 'HOST array',
                   'no covariance', 'One wave per sample', 'pure function'):
        assert phrase in spec, 'the specification does not fix %r' % phrase
    assert (int(decl.group(2)), int(decl.group(3))) == (24, 16) == (ops_eval.SKEL_MAX_JOINTS, ops_eval.SKEL_MAX_LIMBS)
    p = inspect.signature(ops_eval.triangulate_skeleton).parameters
    assert list(p) == ['points', 'pmat', 'init', 'views', 'limbs', 'weighted', 'huber_px', 'sym_w', 'max_iter', 'want']
    assert (p['views'].default, p['limbs'].default, p['weighted'].default, p['huber_px'].default, p['sym_w'].default,
            p['max_iter'].default, p['want'].default) == (None, ops_eval.SYM_LIMBS, False, 0.0, 0.1, 20, ('resid',))


def test_abi_version_is_unchanged():
    from xas_amd import _lib
    assert _lib.fn('xas_abi_version')() == 3 == _lib.ABI_VERSION


def test_limb_table_is_the_training_losss():
    from modules.base_losses import loss_func as lf
    from xas_amd import ops_eval
    import test_gpu_tri_skeleton as t
    far, near = lf._LIMB_FAR, lf._LIMB_NEAR                           # arm / leg of one side, then of the other, two limbs each
    table = tuple((far[g + i], near[g + i], far[g + i + 2], near[g + i + 2]) for g in (0, 4) for i in (0, 1))
    assert ops_eval.SYM_LIMBS == table == t.SYM_LIMBS == ((16, 15, 13, 12), (15, 14, 12, 11), (3, 2, 6, 5), (2, 1, 5, 4))
    perm = dict(ops_eval.SWITCH_PAIRS)                                # every pair is a limb and its left/right mirror
    perm.update({b: a for a, b in ops_eval.SWITCH_PAIRS})
    assert all(perm[fa] == fb and perm[na] == nb for fa, na, fb, nb in table)


def test_argument_checks_return_errors_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    one, two = ctypes.c_void_p(64), ctypes.c_void_p(128)              # aligned non-null pointers: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    f = _lib.fn(NAME)
    table = lambda rows: (ctypes.c_int * (4 * len(rows)))(*[j for r in rows for j in r])

    def call(V=4, B=2, K=5, limbs=((1, 0, 3, 2),), L=None, flags=0, sym_w=0.1, iters=20, bufs=(one, one, one, two)):
        return f(bufs[0], bufs[1], bufs[2], None, table(limbs) if limbs else None, B, V, K, len(limbs) if L is None else L, flags,
                 0.0, sym_w, iters, bufs[3], None, None, None, None, None)
    assert call(V=1) == 1 and 'V=1 views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6)' in err()
    assert call(V=7) == 1 and 'V=7 views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6)' in err()
    assert call(K=25) == 1 and 'K=25 joints (needs 3 <= K <= XAS_SKEL_MAX_JOINTS = 24)' in err()
    assert call(K=2, limbs=()) == 1 and 'K=2 joints' in err()
    assert call(limbs=((1, 0, 3, 2),) * 17) == 1 and 'L=17 limb pairs (needs 0 <= L <= XAS_SKEL_MAX_LIMBS = 16)' in err()
    assert call(L=-1) == 1 and 'L=-1 limb pairs' in err()
    assert call(limbs=((1, 0, 3, 5),)) == 1 and 'limbs[0][3] = 5 is no joint (needs 0 <= index < K = 5)' in err()
    assert call(limbs=((1, 0, 3, 2), (-1, 0, 3, 2))) == 1 and 'limbs[1][0] = -1 is no joint' in err()
    assert call(limbs=(), L=1) == 1 and 'null limbs with L=1' in err()
    for bad in (-0.5, float('nan'), float('inf')):
        assert call(sym_w=bad) == 1 and 'needs a finite sym_w >= 0' in err()
    for bad in (0, 65):
        assert call(iters=bad) == 1 and 'max_iter=%d trials (needs 1 <= max_iter <= 64)' % bad in err()
    assert call(bufs=(one, one, one, one)) == 1 and 'out must not overlap init' in err()
    assert call(B=0) == 1 and 'bad shape B=0 K=5' in err()
    assert call(B=1 << 28, K=24) == 1 and 'B*K < 2^31' in err()
    for i in range(4):
        bufs = [one, one, one, two]
        bufs[i] = None
        assert call(bufs=bufs) == 1 and 'null buffer (points, P, init and out are required)' in err()
    for bad in (2, 1 << 30, -2):
        assert call(flags=bad) == 1 and 'unknown flag bits' in err()


def test_eval_knows_the_choice_and_the_weight():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'eval.py'), '--help'], capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr
    assert '--tri-refine {none,lm}' in r.stdout and '--tri-skeleton' in r.stdout and '--tri-sym W' in r.stdout
    import eval as xeval
    from modules import util as mu
    from xas_amd import ops_eval
    cli = dict(xeval.CLI)
    assert cli['--tri-refine']['default'] == 'none' and cli['--tri-refine']['choices'] == ['none', 'lm']     # the older flag as it was
    assert cli['--tri-skeleton'] == dict(default=False, action='store_true', dest='tri_skeleton', help=cli['--tri-skeleton']['help'])
    assert cli['--tri-sym']['default'] == 0.1 == ops_eval.TRI_SYM_W
    assert cli['--tri-sym']['type'] is float and cli['--tri-sym']['dest'] == 'tri_sym'
    assert [f for f, _ in xeval.CLI][-2:] == ['--tri-skeleton', '--tri-sym']       # after every older flag
    p = inspect.signature(xeval.Eval.__init__).parameters
    assert list(p) == ['self', 'config', 'detector', 'eval_data', 'log_dir', 'img_size', 'flip_test', 'tri', 'tri_thresh', 'resolve']
    p = inspect.signature(mu.triangulation_skeleton).parameters
    assert list(p) == ['keypoints', 'params', 'cam_id_list', 'weights', 'is_norm', 'RECT_WIDTH', 'robust_px', 'huber_px', 'sym_w',
                       'limbs', 'want', 'inputs']
    assert [p[n].default for n in list(p)[3:]] == [None, True, 2000, None, 0.0, 0.1, ops_eval.SYM_LIMBS, (), None]


def test_oracle_reprojection_terms_are_the_per_joint_oracles():
    """Term for term: the vectorised reprojection part of _skeleton_oracle against _refine_oracle.terms, joint by joint, under
    weights and under Huber's loss."""
    import test_gpu_tri_skeleton as t
    import _refine_oracle as ro
    import _skeleton_oracle as so
    for name in ('w0.1_weighted', 'w0.1_huber', 'fixed'):
        c, o = t.case(name)
        for b in range(min(2, c['points'].shape[0])):
            sp = so.Sample(c['points'][b], c['P'][b], c['init'][b], None, c['limbs'], c['weighted'], c['huber'], c['sym_w'])
            X = sp.start()
            Ck, r2, Hk, gk, front, _ = sp.reproj(X)
            for k in np.flatnonzero(sp.free):
                F = ro.views_used(c['points'][b, :, k], 0)
                C, rr, H, g, fr = ro.terms(c['points'][b, :, k], c['P'][b], X[k], F, c['weighted'], c['huber'])
                np.testing.assert_allclose([Ck[k], r2[k]], [C, rr], rtol=1e-13)
                np.testing.assert_allclose(Hk[k], H, rtol=1e-12, atol=1e-15)
                np.testing.assert_allclose(gk[k], g, rtol=1e-11, atol=1e-12)
                assert fr and front[k]


def _names():
    import test_gpu_tri_skeleton as t
    return list(t.CASES)


@pytest.mark.parametrize('name', _names())
def test_gpu_case_inputs(name):
    """Every case of the GPU file, with the oracle alone: free joints and active pairs as the case claims, at least 90 % of the
    samples of a compared case inside COND_MAX, the minimum costs no more than the start, and for every compared sample the
    two parts of the position tolerance sum to at most 1e-4 mm and the restated loop ends that close to the minimum."""
    import test_gpu_tri_skeleton as t
    import _skeleton_oracle as so
    c, o = t.case(name)
    B, V, K, _ = c['points'].shape
    assert (B, V, K, len(c['limbs'])) in [s for s in t.SHAPES] + [(3, 6, 18, 4), (2, 2, 18, 4)]
    cmp = t.compared(name)
    s = so.schedule(c['points'], c['P'], c['init'], max_iter=c['max_iter'], **t._kw(c))
    has = o['free'].any(1)
    stop = 1e-5 * s['rate'] / (1 - np.minimum(s['rate'], 0.999))
    with np.errstate(invalid='ignore'):
        left = np.where(o['free'][..., None], np.abs(s['xyz'] - o['xyz']), 0.0).reshape(B, -1).max(1)    # fixed joints: init, maybe NaN
    print('%s: B=%d V=%d K=%d L=%d, %d of %d joints free, %d of %d pairs active, cond max %.3g, %d samples compared; rate max %.3g, '
          'stop remainder + cost floor max %.3g mm, restated loop ends %.3g mm from the minimum at most after %d trials at most' % (
              name, B, V, K, len(c['limbs']), o['free'].sum(), o['free'].size, o['active'].sum(), o['active'].size,
              np.nanmax(o['cond']) if has.any() else np.nan, cmp.sum(), s['rate'].max(), (stop + o['floor'])[cmp].max() if cmp.any() else 0,
              np.nanmax(left[cmp]) if cmp.any() else 0, s['trials'].max()))
    assert (o['cost'][:, 1] <= o['cost'][:, 0]).all()
    if c['compare']:
        assert (o['cond'][has] <= so.COND_MAX).mean() >= 0.9 and cmp[has].mean() >= 0.9
        assert (s['rate'][cmp] <= 0.9).all() and ((stop + o['floor'])[cmp] <= 1e-4).all()
        assert (left[cmp] <= 1e-4).all()
        assert s['trials'][cmp].max() < c['max_iter'] or (left[cmp] <= o['floor'][cmp] + 1e-6).all()
    if name in t.COUPLED:
        assert o['free'].all() and o['active'].all() and c['sym_w'] in (0.1, 10.0) and len(c['limbs']) > 0
        limb = lambda w, f, n: np.linalg.norm(w[:, f].astype(np.float64) - w[:, n], axis=-1)
        for fa, na, fb, nb in c['limbs']:                             # planted exactly symmetric
            assert np.array_equal(limb(c['world'], fa, na), limb(c['world'], fb, nb))
        if 'clean' in name:
            assert np.abs(o['xyz'] - c['world']).max() < 1e-2 and np.abs(o['sym']).max() < 1e-2
        if 'noisy' in name:
            assert 0.2 < np.sqrt((o['resid'][..., 0] ** 2).mean()) < 2 * 2.0 * np.sqrt(2)
            assert np.abs(o['sym'][..., 0]).mean() > 1.0              # noise leaves the DLT's limbs millimetres apart
        if 'huber' in name:
            assert (o['resid'][..., 1] > 3.0).all() and c['max_iter'] == 64
        if 'weighted' in name:
            w = c['points'][..., 2]
            assert 3.0 < w.max() / w.min() < 4.0 and c['weighted']
        if 'robust' in name:
            import _tri_oracle as to
            to.check_decidable(c['robust'], name)
            assert np.array_equal(c['robust']['mask'], 15 & ~c['planted']) and np.count_nonzero(c['planted']) == 8
    if name in t.DECOUPLED:
        assert c['sym_w'] == 0.0 or len(c['limbs']) == 0
    if name == 'fixed':
        for b, joints in t.FIXED_JOINTS.items():
            assert tuple(np.flatnonzero(~o['free'][b])) == joints
        assert o['active'].tolist() == [[False] * 4, [False] * 4, [True] * 4] and cmp.tolist() == [True, False, True]
    if name == 'behind':
        assert tuple(np.flatnonzero(~o['free'][0])) == (3, 16) and o['free'][1].all()
        assert o['active'].tolist() == [[False, True, False, True], [True] * 4]
    if name == 'flat':
        assert np.array_equal(c['init'][0, 16], c['init'][0, 15]) and o['sym'][0, 0, 0] < -100 and np.isfinite(o['xyz']).all()
    if name == 'illcond':
        assert (o['cond'] > so.COND_MAX).all() and not cmp.any()
    if name == 'one_trial':
        assert (s['status'] == 1).all() and (s['trials'] == 1).all()


def test_oracle_minimum_is_a_minimum():
    """Independent of its own minimiser, by probing: at the returned point no step of 1e-3 mm along any free axis lowers the cost."""
    import test_gpu_tri_skeleton as t
    import _skeleton_oracle as so
    for name in ('w10_noisy_b2v4k18l4', 'w10_huber', 'behind'):
        c, o = t.case(name)
        sp = so.Sample(c['points'][0], c['P'][0], c['init'][0], None if c['views'] is None else c['views'][0], c['limbs'],
                       c['weighted'], c['huber'], c['sym_w'])
        X = np.where(sp.free[:, None], o['xyz'][0], 0.0)
        C = sp.terms(X)[0]
        for i in range(sp.n):
            for sgn in (1e-3, -1e-3):
                d = np.zeros(sp.n)
                d[i] = sgn
                assert sp.terms(sp.moved(X, d))[0] > C
