"""The heat-map spread without a GPU: the two entry points are exported, declared in include/xas_hip.h and bound by the ctypes
table; their argument checks answer before any launch and name the range; eval.py knows --tri-weight; the old util and Eval
signatures stay as the existing tests pin them and the weighted variants stand beside them; the float64 restatement
(tests/_spread_oracle.py) meets the closed forms; the float32 model of the kernel's scheme stays inside the tolerance taken from
it; and, the point of the feature, a float64 weighted DLT lands closer to the truth with spread weights than with the
reference's depth weights when one view per joint is displaced and broad."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _spread_oracle as so
import _tri_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'x-as-supervision_amd')
NAMES = {'xas_head_spread_workspace_floats': ('iii', 'z'), 'xas_head_spread': ('piiippp', 'i')}


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib, ops_head
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in NAMES.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
        assert len(_lib.fn(name).argtypes) == len(sig[0])
    header = open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()
    m = re.search(r'#define XAS_HEAD_SPREAD (\d+)\s*size_t\s+xas_head_spread_workspace_floats', header)
    assert m and int(m.group(1)) == 5 == ops_head.HEAD_SPREAD


def test_abi_version_is_unchanged():
    from xas_amd import _lib
    assert _lib.fn('xas_abi_version')() == 3 == _lib.ABI_VERSION


def test_argument_checks_return_errors_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)                       # any aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    f, ws = _lib.fn('xas_head_spread'), _lib.fn('xas_head_spread_workspace_floats')
    for B, K, D in ((2, 3, 6), (2, 3, 132)):
        assert f(one, B, K, D, one, one, None) == 1 and 'multiple of 4 in [4,128]' in err()
        assert ws(B, K, D) == 0 and 'multiple of 4 in [4,128]' in err()
    assert f(one, 2, 0, 8, one, one, None) == 1 and 'K > 0' in err()
    assert ws(2, 0, 8) == 0
    assert f(one, 2, 3, 8, None, one, None) == 1 and 'head spread: null buffer' in err()
    for D, K, B in so.SHAPES:                       # [B][nchunk][K][7]
        assert ws(B, K, D) == B * so.policy_of(D, K)['nchunk'] * K * 7


def test_eval_knows_the_flag_and_defaults_to_depth(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'eval.py'), '--help'], capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr
    assert '--tri-weight {depth,spread}' in r.stdout
    import eval as xeval
    cli = dict(xeval.CLI)
    assert cli['--tri-weight']['default'] == 'depth' and cli['--tri-weight']['choices'] == ['depth', 'spread']
    assert 'tri_weight' not in inspect.signature(xeval.Eval.__init__).parameters      # model_params.tri_weight carries it
    cfg = lambda **mp: {'model_params': dict(cam_id_list=[0, 1], **mp), 'dataset_params': {'dataset': {'name': 'h36m'}}}
    with pytest.raises(ValueError, match='Unknown triangulation weight: entropy'):
        xeval.Eval(cfg(tri_weight='entropy'), None, [], str(tmp_path))


def test_weighted_variants_stand_beside_the_old_signatures():
    from modules import util as mu
    p = inspect.signature(mu.triangulation).parameters
    assert list(p) == ['keypoints', 'params', 'cam_id_list', 'is_norm', 'RECT_WIDTH', 'robust_px', 'return_inliers']
    q = inspect.signature(mu.triangulation_weighted).parameters
    assert list(q) == ['keypoints', 'params', 'cam_id_list', 'weights', 'is_norm', 'RECT_WIDTH', 'robust_px', 'return_inliers', 'inputs']
    assert all(q[n].default == p[n].default for n in list(p)[3:])
    p = inspect.signature(mu.resolve_views).parameters
    assert list(p) == ['kps_by_cam', 'params', 'cam_id_list', 'pairs', 'gt', 'RECT_WIDTH']
    q = inspect.signature(mu.resolve_views_weighted).parameters
    assert list(q) == ['kps_by_cam', 'params', 'cam_id_list', 'pairs', 'weights', 'gt', 'RECT_WIDTH']
    assert all(q[n].default == p[n].default for n in list(p)[4:])
    p = inspect.signature(mu.spread_weight).parameters
    assert list(p) == ['spread', 'trans_image', 'cell_px'] and p['cell_px'].default == 4.0
    for cls in ('keypoint_detector_integral.KPDetector3D', 'keypoint_detector_integral_multi.KPDetector3DMulti'):
        mod, name = cls.split('.')
        det = getattr(__import__('modules.' + mod, fromlist=[name]), name)
        p = inspect.signature(det.forward_spread).parameters
        assert list(p) == ['self', 'x', 'flip_pairs'] and p['flip_pairs'].default is None


# ---- the float64 restatement against closed forms ----------------------------------------------------------------------------
@pytest.mark.parametrize('D', [4, 12, 64])
def test_oracle_uniform_logits(D):
    s = so.spread64(np.zeros((1, 2 * D, D, D), np.float32), 2)
    np.testing.assert_allclose(s[..., :2], (D - 1) / 2, rtol=1e-12)
    np.testing.assert_allclose(s[..., 2:4], (D * D - 1) / 12, rtol=1e-12)
    assert np.abs(s[..., 4]).max() < 1e-12


def test_oracle_one_hot_map_and_its_weight():
    D = 16
    s = so.spread64(so.spike(D) * 10.0, 1)                                    # logit 800: one-hot in float64
    np.testing.assert_allclose(s[0, 0], [D - 1, D - 1, 0, 0, 0], atol=1e-12)
    trans = np.array([[[0.5, 0.1, 3.0], [-0.1, 0.5, 7.0]]])
    scale = 1 / np.sqrt(0.5 * 0.5 + 0.1 * 0.1)
    np.testing.assert_allclose(so.spread_weight64(s, trans), 1 / np.sqrt(2 / 12 * (4 * scale) ** 2), rtol=1e-12)


def test_oracle_two_equal_spikes():
    D, a, b = 16, 3, 12
    l = np.zeros((1, 1, D, D, D), np.float32)
    l[0, 0, 2, 5, a] = l[0, 0, 9, 5, b] = 800.0
    s = so.spread64(l.reshape(1, D, D, D), 1)[0, 0]
    np.testing.assert_allclose(s, [(a + b) / 2, 5, (a - b) ** 2 / 4, 0, 0], atol=1e-12)


def test_oracle_flip_is_the_mixture_formula():
    """spread_flip64 forms the averaged heat-map explicitly; the closed mixture formula of ops_head.spread_flip must agree."""
    import torch
    from xas_amd import ops_head
    D, K, perm = 8, 4, [0, 2, 1, 3]
    l = so.logits(D, K, 4, seed=7)
    want = so.spread_flip64(l, K, perm)
    got = ops_head.spread_flip(torch.from_numpy(so.spread64(l, K)), torch.tensor(perm), D).numpy()
    np.testing.assert_allclose(got, want, atol=1e-12)


def test_spread_weight_is_the_restatement():
    import torch
    from modules import util as mu
    rng = np.random.Generator(np.random.PCG64(3))
    sp = np.abs(rng.standard_normal((3, 5, 5))) * 4
    trans = rng.standard_normal((3, 2, 3))
    got = mu.spread_weight(torch.from_numpy(sp), torch.from_numpy(trans)).numpy()
    np.testing.assert_allclose(got, so.spread_weight64(sp, trans), rtol=1e-12)
    got = mu.spread_weight(torch.from_numpy(sp), torch.from_numpy(trans), cell_px=2.0).numpy()
    np.testing.assert_allclose(got, so.spread_weight64(sp, trans, 2.0), rtol=1e-12)


# ---- the float32 model of the kernel's scheme: where the GPU test's tolerance comes from ------------------------------------------
def test_policy_table_reaches_every_launch_path():
    p = {s: so.policy_of(s[0], s[1]) for s in so.SHAPES}
    assert [p[s]['pow2'] for s in so.SHAPES] == [False, False, True, True, False, True, False, False]
    assert p[(12, 2, 2)]['G'] == 3 and p[(64, 2, 1)]['nchunk'] == 32 and p[(44, 94, 1)]['ntile'] == 2
    assert p[(128, 1, 1)]['nchunk'] == 128 > 64                               # the second pass takes its chunks 64 at a time
    assert not so.policy_of(8, 2, general=True)['pow2']


@pytest.mark.parametrize('shape', so.SHAPES[:6])
def test_model_error_is_within_what_the_tolerance_was_taken_from(shape):
    (_, path, em, e2), = so.model_errors([shape])
    print('%s %s: mean %.3e  second moments %.3e' % (shape, path, em, e2))
    assert em <= so.MODEL_ERR_MEAN and e2 <= so.MODEL_ERR_MOM2
    assert so.TOL_MEAN == 8 * so.MODEL_ERR_MEAN and so.TOL_MOM2 == 8 * so.MODEL_ERR_MOM2


def test_model_keeps_a_far_spike_and_a_far_narrow_peak():
    """A spike at w = h = 127, and a peak one cell wide beside it: the centred records keep the variance non-negative and
    within the tolerance, and nearer the float64 value than E[w^2] - E[w]^2 summed in float32 over exact marginals."""
    D = 128
    w, h = np.arange(D)[None, :], np.arange(D)[:, None]
    peak = np.broadcast_to(-((w - 126.4) ** 2 + (h - 126.4) ** 2) / (2 * 0.5 ** 2), (1, D, D, D)).astype(np.float32)
    for l in (so.spike(D), peak):
        s = so.model32(l, 1)[0, 0]
        want = so.spread64(l, 1)[0, 0]
        assert (s[2:4] >= 0).all()
        assert np.abs(s[:2] - want[:2]).max() <= so.TOL_MEAN and np.abs(s[2:] - want[2:]).max() <= so.TOL_MOM2
    q = so.marginal64(peak, 1)[0, 0].astype(np.float32)
    wf = np.arange(D, dtype=np.float32)[None, :]
    naive = np.float32((q * wf * wf).sum(dtype=np.float32)) - np.float32((q * wf).sum(dtype=np.float32)) ** 2
    print('one-cell peak at 126.4: Var w %.7f, model %.7f, naive float32 %.7f' % (want[2], s[2], naive))
    assert abs(float(s[2]) - want[2]) < abs(float(naive) - want[2])


# ---- the point of the feature ----------------------------------------------------------------------------------------------------
def scene(V=4, K=6, D=8, seed=11):
    """V cameras on a ring at different distances, looking at K joints near the origin.  View k % V of joint k is displaced by
    30 px and has a broad heat-map (sigma 2.5 cells); every other view is exact with a sharp one (sigma 0.5 cells).
    -> points [1,V,K,3] (u, v, depth mm), P [1,V,3,4], world [1,K,3], logits [V, K*D, D, D], trans_image [V,2,3]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    world = rng.uniform(-500, 500, (K, 3))
    pts, P = np.zeros((V, K, 3)), np.zeros((V, 3, 4))
    for v in range(V):
        a, dist = 2 * np.pi * v / V + 0.3, 3000.0 + 1000.0 * v
        c = np.array([dist * np.cos(a), dist * np.sin(a), 400.0 * (v - 1.5)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        Km = np.array([[1150.0, 0, 500], [0, 1150.0, 500], [0, 0, 1]])
        P[v] = Km @ np.concatenate([R, (-R @ c)[:, None]], axis=1)
        cam = world @ R.T - R @ c
        pts[v, :, :2] = (cam @ Km.T)[:, :2] / cam[:, 2:]
        pts[v, :, 2] = cam[:, 2]
    logits = np.zeros((V, K, D, D, D))
    w, h = np.arange(D)[None, :], np.arange(D)[:, None]
    for k in range(K):
        bad = k % V
        ang = rng.uniform(0, 2 * np.pi)
        pts[bad, k, :2] += 30.0 * np.array([np.cos(ang), np.sin(ang)])
        for v in range(V):
            sig = 2.5 if v == bad else 0.5
            logits[v, k] = (-((w - 3.3 - 0.2 * k) ** 2 + (h - 4.1) ** 2) / (2 * sig * sig))[None]
    trans = np.tile(np.array([[0.25, 0.0, 10.0], [0.0, 0.25, 20.0]]), (V, 1, 1))
    f32 = lambda a: a.astype(np.float32)
    return f32(pts[None]), f32(P[None]), world[None], f32(logits.reshape(V, K * D, D, D)), trans


def test_spread_weights_beat_depth_weights_on_every_joint():
    pts, P, world, logits, trans = scene()
    V, K = pts.shape[1:3]
    wgt = so.spread_weight64(so.spread64(logits, K), trans)                   # [V,K]
    assert wgt.max() / wgt.min() > 3                                          # broad maps do count less
    weighted = pts.copy()
    weighted[0, :, :, 2] = wgt
    e_depth = np.linalg.norm(to.dlt(pts, P) - world, axis=-1)[0]
    e_spread = np.linalg.norm(to.dlt(weighted, P) - world, axis=-1)[0]
    print('error with depth weights %s mm\nerror with spread weights %s mm' % (np.round(e_depth, 2), np.round(e_spread, 2)))
    assert (e_spread < e_depth).all()
    assert e_depth.min() > 5.0                                                # the displaced view does pull the plain DLT away
