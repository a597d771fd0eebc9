"""Heat-map spread on the device (xas_head_spread) against the float64 definition of tests/_spread_oracle.py, on the smallest
shapes that reach each launch path of csrc/head.hip, and the layers above it: ops_head.spread_flip, the detectors'
forward_spread, triangulation_weighted / resolve_views_weighted of modules/util.py and Eval with model_params.tri_weight.

Tolerance: 8 x the largest distance of the kernel's scheme, evaluated in float32 numpy on the CPU (_spread_oracle.model32), from
the float64 definition over the same inputs - 8 x 8.807e-06 cells for the means, 8 x 2.925e-04 cells^2 for the second moments
(tests/test_head_spread_abi.py re-runs the small shapes; DESIGN.md records the whole run).  Absolute, for every shape."""
import functools

import numpy as np
import pytest
import torch

import _spread_oracle as so
from test_gpu_head_flip import HM36_PAIRS, perm_of

pytestmark = pytest.mark.gpu
TOL_MEAN = so.TOL_MEAN          # 7.05e-05 cells
TOL_MOM2 = so.TOL_MOM2          # 2.34e-03 cells^2


def dev(l):
    return torch.from_numpy(np.ascontiguousarray(l)).cuda().contiguous(memory_format=torch.channels_last)


def run(l, K):
    from xas_amd import ops_head
    return ops_head.heatmap_spread(l if isinstance(l, torch.Tensor) else dev(l), K).cpu().numpy()


@functools.lru_cache(maxsize=None)
def want(shape):
    D, K, B = shape
    return so.spread64(so.logits(D, K, B), K)


def check(got, ref, what):
    em, e2 = np.abs(got[..., :2] - ref[..., :2]).max(), np.abs(got[..., 2:] - ref[..., 2:]).max()
    print('%s: |mean - f64| %.3e cells (bar %.3e)  |second moments - f64| %.3e cells^2 (bar %.3e)' % (what, em, TOL_MEAN, e2, TOL_MOM2))
    assert got.dtype == np.float32 and (got[..., 2:4] >= 0).all()
    assert em <= TOL_MEAN and e2 <= TOL_MOM2


@pytest.mark.parametrize('shape', so.SHAPES, ids=lambda s: 'D%d-K%d-B%d' % s)
def test_random_logits_vs_float64(shape):
    D, K, B = shape
    got = run(so.logits(D, K, B), K)
    assert got.shape == (B, K, 5)
    check(got, want(shape), '%s %s' % (shape, 'pow2' if so.policy_of(D, K)['pow2'] else 'general'))


def test_general_policy_at_a_power_of_two_side():
    from xas_amd import _lib
    shape = (8, 2, 3)
    _lib.query('xas_set_tuning', _lib.TUNE_GENERAL_KERNELS)
    try:
        got = run(so.logits(*shape), shape[1])
    finally:
        _lib.query('xas_set_tuning', 0)
    check(got, want(shape), '%s general by tuning flag' % (shape,))


@pytest.mark.parametrize('D', [64, 128])
def test_far_spike_has_no_negative_variance(D):
    l = so.spike(D)
    check(run(l, 1), so.spread64(l, 1), 'spike of 80 at (%d, %d)' % (D - 1, D - 1))


@pytest.mark.parametrize('D', [8, 12])
def test_uniform_logits_closed_form(D):
    got = run(np.zeros((2, 2 * D, D, D), np.float32), 2)
    ref = np.broadcast_to(np.array([(D - 1) / 2, (D - 1) / 2, (D * D - 1) / 12, (D * D - 1) / 12, 0.0]), got.shape)
    check(got, ref, 'uniform D=%d' % D)


@pytest.mark.parametrize('shape', [(8, 2, 3), (12, 2, 2)], ids=lambda s: 'D%d-K%d-B%d' % s)
def test_shift_by_1e4_changes_nothing(shape):
    D, K, B = shape
    l = so.logits(D, K, B)
    shifted = l + np.float32(1e4)
    assert np.array_equal(shifted.astype(np.float64), l.astype(np.float64) + 1e4)     # the shifted inputs are exact
    check(run(shifted, K), want(shape), '%s + 1e4' % (shape,))


def test_a_nan_joint_is_nan_and_alone():
    shape = (8, 2, 3)
    D, K, B = shape
    l = so.logits(D, K, B).copy()
    l.reshape(B, K, D, D, D)[1, 1] = np.nan
    got = run(l, K)
    assert np.isnan(got[1, 1]).all()
    keep = np.ones((B, K), bool)
    keep[1, 1] = False
    assert np.array_equal(got[keep], run(so.logits(D, K, B), K)[keep])
    ref = so.spread64(l, K)
    assert np.isnan(ref[1, 1]).all() and np.isfinite(ref[keep]).all()


@pytest.mark.selfcheck
@pytest.mark.parametrize('shape', [(8, 2, 3), (44, 94, 1)], ids=lambda s: 'D%d-K%d-B%d' % s)
def test_two_calls_are_bit_identical(shape):
    from xas_amd import ops_head
    D, K, B = shape
    l = dev(so.logits(D, K, B))
    assert torch.equal(ops_head.heatmap_spread(l, K), ops_head.heatmap_spread(l, K))


def test_binding_takes_nchw_storage_and_refuses_other_shapes():
    from xas_amd import ops_head
    D, K, B = 8, 2, 3
    l = torch.from_numpy(so.logits(D, K, B)).cuda()                                   # NCHW storage: converted inside
    assert torch.equal(ops_head.heatmap_spread(l, K), ops_head.heatmap_spread(dev(so.logits(D, K, B)), K))
    l.requires_grad_(True)
    assert not ops_head.heatmap_spread(l, K).requires_grad
    with pytest.raises(RuntimeError, match='heat-map cube'):
        ops_head.heatmap_spread(l[:, :, :, :6], K)
    with pytest.raises(RuntimeError, match=r'multiple of 4 in \[4,128\]'):
        ops_head.heatmap_spread(torch.zeros(1, 12, 6, 6, device='cuda'), 2)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_spread_flip_vs_the_explicit_average():
    from xas_amd import ops_head
    D, K, B = 8, 4, 2
    perm = perm_of([(1, 2)], K)
    l = so.logits(D, K, 2 * B, seed=5)
    got = ops_head.spread_flip(ops_head.heatmap_spread(dev(l), K), torch.as_tensor(perm), D).cpu().numpy()
    assert got.shape == (B, K, 5)
    # (Va + Vb) / 2 carries the second moments' tolerance; (ua - ub)^2 / 4 moves by |ua - ub| / 2 * (|d ua| + |d ub|), at most
    # D * TOL_MEAN for two means in [0, D) that each carry the means' tolerance
    ref = so.spread_flip64(l, K, perm)
    em, e2 = np.abs(got[..., :2] - ref[..., :2]).max(), np.abs(got[..., 2:] - ref[..., 2:]).max()
    print('spread_flip: mean %.3e (bar %.3e)  second moments %.3e (bar %.3e)' % (em, TOL_MEAN, e2, TOL_MOM2 + D * TOL_MEAN))
    assert em <= TOL_MEAN and e2 <= TOL_MOM2 + D * TOL_MEAN


@pytest.mark.parametrize('multi', [True, False], ids=['multi', 'single'])
def test_forward_spread_is_forward_plus_the_spread(multi):
    from test_gpu_eval_flip import D, K, detector, images
    from xas_amd import ops_head, ops_nn
    det, x = detector(multi), images()
    with torch.no_grad():
        kps, dmap = det(x)
        logits = det.net(x)
    k2, d2, spread = det.forward_spread(x)
    assert torch.equal(k2, kps) and torch.equal(d2, dmap)
    assert spread.shape == (x.shape[0], K, 5) and not spread.requires_grad
    assert torch.equal(spread, ops_head.heatmap_spread(logits, K))
    check(spread.cpu().numpy(), so.spread64(logits.cpu().numpy(), K), 'detector logits, D=%d' % D)
    with torch.no_grad():
        kf, df = det.forward_flip(x, HM36_PAIRS)
        l2 = det.net(ops_nn.mirror_pair_nchw(x))
    k3, d3, sf = det.forward_spread(x, HM36_PAIRS)
    assert torch.equal(k3, kf) and torch.equal(d3, df)
    assert torch.equal(sf, ops_head.spread_flip(ops_head.heatmap_spread(l2, K), det._flip_perm, D))
    with pytest.raises(RuntimeError, match='square input patches'):
        det.forward_spread(x[:, :, :32])


def _cfg(cams, tri_weight=None):
    """tri_weight: the key eval.py's --tri-weight sets in model_params (None: the key is absent, as in the shipped configs)."""
    mp = {'cam_id_list': list(cams), 'flip_pairs': HM36_PAIRS}
    if tri_weight is not None:
        mp['tri_weight'] = tri_weight
    return {'model_params': mp, 'dataset_params': {'dataset': {'name': 'mpi_inf_3dhp'}}}


@functools.lru_cache(maxsize=None)
def eval_inputs():
    from test_gpu_eval_flip import B, S
    from xas_amd.synthetic import synthetic_eval_batch
    cams = [0, 1, 2]
    return cams, synthetic_eval_batch(B, cams, torch.device('cuda'), seed=5, S=S)


def _stacked(sel, x, cams, is_norm=True):
    from xas_amd import ops_eval
    pts, pm = [], []
    for c in cams:
        m = 'cam_%d' % c
        pts.append(ops_eval.patch_to_image(sel[m], x[m + '_trans_image'], x[m + '_pelvis'], image_size=x[m + '_img'].shape[-1],
                                           rect_width=2000, is_norm=is_norm))
        pm.append(ops_eval.projection_matrix(x[m + '_k_mat'], x[m + '_rot_world'], x[m + '_trans_world']))
    return torch.stack(pts, dim=1), torch.stack(pm, dim=1)


def test_triangulation_weights_keyword():
    from modules import util as mu
    from xas_amd import ops_eval
    cams, x = eval_inputs()
    sel = {'cam_%d' % c: x['cam_%d_joints' % c] for c in cams}             # the labels, in patch pixels
    plain = mu.triangulation(sel, x, cams, is_norm=False)
    assert bool(torch.isfinite(plain).all())
    assert torch.equal(mu.triangulation_weighted(sel, x, cams, None, is_norm=False), plain)
    B, K = plain.shape[:2]
    gen = torch.Generator().manual_seed(3)
    weights = {m: (torch.rand(B, K, generator=gen) + 0.1).cuda() for m in sel}
    pts, P = _stacked(sel, x, cams, is_norm=False)
    pts[..., 2] = torch.stack([weights['cam_%d' % c] for c in cams], dim=1)
    got = mu.triangulation_weighted(sel, x, cams, weights, is_norm=False)
    assert torch.equal(got, ops_eval.triangulate_dlt(pts, P)[..., :3]) and not torch.equal(got, plain)
    rob, used = mu.triangulation_weighted(sel, x, cams, weights, is_norm=False, robust_px=20.0, return_inliers=True)
    r = ops_eval.triangulate_robust(pts, P, threshold_px=20.0, want=('inliers',))
    assert torch.equal(rob, r['xyzw'][..., :3]) and torch.equal(used, r['inliers'])


def test_eval_batch_depth_is_the_default_and_spread_is_the_composition(tmp_path):
    import eval as xeval
    from modules import util as mu
    from test_gpu_eval_flip import S, detector
    from xas_amd import ops_eval, ops_head
    cams, x = eval_inputs()
    det = detector(True)
    mk = lambda tri_weight=None, **kw: xeval.Eval(_cfg(cams, tri_weight), det, [], str(tmp_path), img_size=float(S), **kw)
    default, depth, spread = (mk(w).eval_batch(x, 'best') for w in (None, 'depth', 'spread'))
    assert set(depth) == set(default) and all(torch.equal(depth[k], default[k]) for k in default)
    assert set(spread) == set(default) | {'tri_sigma'}
    for k in default:                                                         # nothing but the triangulated pose moves
        if 'tri' not in k:
            assert torch.equal(spread[k], default[k]), k
    sel, weights = {}, {}
    with torch.no_grad():
        for c in cams:
            m = 'cam_%d' % c
            logits = det.net(x[m + '_img'])
            kps = ops_head.softargmax_multi(logits, det.num_kp, det.num_hypo, det.neighbor_size)[0]
            sel[m] = ops_eval.eval_select(kps, x[m + '_joints'], image_size=float(S), mode='best')['sel3d']
            weights[m] = mu.spread_weight(ops_head.heatmap_spread(logits, det.num_kp), x[m + '_trans_image'])
    pts, P = _stacked(sel, x, cams)
    pts[..., 2] = torch.stack([weights['cam_%d' % c] for c in cams], dim=1)
    assert torch.equal(spread['world_tri'], ops_eval.triangulate_dlt(pts, P)[..., :3])
    assert not torch.equal(spread['world_tri'], default['world_tri'])
    sigma = torch.stack([1.0 / weights['cam_%d' % c] for c in cams]).mean()
    assert torch.equal(spread['tri_sigma'], sigma) and float(sigma) > 0
    for kw in (dict(flip_test=True), dict(tri='robust'), dict(resolve='views')):   # the other modes take the weights too
        a, b = mk(**kw).eval_batch(x, 'best'), mk('spread', **kw).eval_batch(x, 'best')
        assert set(b) == set(a) | {'tri_sigma'} and bool(torch.isfinite(b['world_tri']).all()), kw
        assert not torch.equal(a['world_tri'], b['world_tri']), kw


def test_result_file_gains_one_line_with_spread(tmp_path):
    import eval as xeval
    from test_gpu_eval_flip import S, detector
    cams, x = eval_inputs()
    det = detector(True)
    texts = {}
    for tag, w in (('none', None), ('depth', 'depth'), ('spread', 'spread')):
        e = xeval.Eval(_cfg(cams, w), det, [dict(x), dict(x)], str(tmp_path / tag), img_size=float(S))
        lines = e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt', 'rb').read()
        assert texts[tag].decode().strip().split('\n') == lines
    assert texts['depth'] == texts['none']
    old, new = (texts[t].decode().strip().split('\n') for t in ('none', 'spread'))
    assert len(new) == len(old) + 1 and new[-1].startswith('TRI weight spread: mean sigma ') and new[-1].endswith(' px')
    assert float(new[-1].split()[-2]) > 0
    cut = old.index('---Tri3D-----')
    assert new[:cut] == old[:cut] and new[cut + 1:-1] != old[cut + 1:]        # only the triangulated figures move
    with pytest.raises(ValueError, match='Unknown triangulation weight'):
        xeval.Eval(_cfg(cams, 'entropy'), det, [], str(tmp_path))
