"""xas_triangulate_refine on the MI355X against its float64 restatement (tests/_refine_oracle.py), from the kernel up to
Eval.eval_batch and the result file.

Every input is built on the CPU (CASES): V cameras on a ring round the subject, 3-5 m from world points of about 1 m extent,
exact projections through the float32 projection matrices, then seeded pixel noise, weights, displaced views, dead views and
view masks on top.  The start point of every case is the float64 DLT over the views used, rounded to float32
(_refine_oracle.dlt_start), so that tests/test_tri_refine_abi.py validates exactly these inputs without a GPU: the condition
number of every compared joint, and what the cases claim about themselves.  The device's own DLT and robust results are
the start where a test is about them.

Tolerances (derived, not tuned):
  position  kernel and oracle both minimise in double; they differ by the kernel's stop rule (an accepted step under 1e-5 mm:
            with convergence at a rate r the distance left is that times r / (1 - r); r ~ 1e-3 for least squares, up to 0.6 under
            Huber's loss) and one rounding of the output to float32: |d|_inf <= 1e-4 mm + 2 ulp_fp32(max |coordinate|), for
            joints with cond <= 1e3.
  resid     4 float32 ulp of the value + 1e-6 px at the start point (the same float32 numbers on both sides).  At the result, in
            every case, that + the oracle's own change of resid when its point moves by the position tolerance, 1e-4 mm
            (`resid_shift`, computed as `cov_shift` is): kernel and oracle are allowed to stand that far apart, and resid is read
            at each one's own point.  Where the cost is the plain sum of squared pixels the RMS is stationary at the minimum and
            the term is ~1e-10 px; under weights or Huber it is not, and the term is up to 0.4 px/mm * 1e-4 mm = 4e-5 px.
            Measured on the MI355X there was no excess over the bound without that term: the largest distance after refinement
            was 0.21 of it (huber), 0.081 (weighted) and 0.094 or less in every other case.
  cov       4 float32 ulp of the largest entry of the joint's matrix + the oracle's own change of cov under a 1e-4 mm shift.
  cost      C(out) <= C(init) in double from the float32 outputs, with the slack of one float32 rounding of out
            (_refine_oracle.cost_at).
"""
import functools

import numpy as np
import pytest
import torch

import _refine_oracle as ro
import _tri_oracle as to
from _refine_inputs import SIGMA_PX, noisy, project, ring_rig
from test_gpu_tri_robust import PlantedDetector, _cfg, eval_case, plant

pytestmark = pytest.mark.gpu
SHAPES = ((2, 2, 1), (2, 4, 5), (2, 6, 64), (2, 2, 64), (2, 6, 1), (3, 4, 5))       # (B, V, K); B*K = 15 leaves the block partial
THR = 20.0


# ------------------------------------------------------------------------------------------------ inputs (CPU only)
def _case(rig, views=None, weighted=False, huber=0.0, init=None, compare=True):
    pts, P, world = rig
    return dict(points=pts, P=P, world=world, views=views, weighted=weighted, huber=huber, compare=compare,
                init=ro.dlt_start(pts, P, views) if init is None else init)


def _weighted():
    """Every view has its own sigma, 0.5 to 5 px over the views, noise of that size, and 1 / sigma as its weight."""
    pts, P, world = ring_rig(2, 4, 5, 31)
    rng = np.random.Generator(np.random.PCG64(131))
    sigma = np.array([0.5, 5.0, 1.5, 3.0])[None, :, None] * rng.uniform(0.9, 1.0, (2, 4, 5))
    pts[..., :2] += (sigma[..., None] * rng.normal(0.0, 1.0, (2, 4, 5, 2))).astype(np.float32)
    pts[..., 2] = (1.0 / sigma).astype(np.float32)
    return _case((pts, P, world), weighted=True)


def _huber(huber):
    pts, P, world = noisy(ring_rig(2, 4, 5, 32), 132)
    for b in range(2):
        for k in range(5):
            pts[b, (b + k) % 4, k, :2] += np.float32(40.0) * np.array([0.6, -0.8], np.float32)        # 40 px off
    return _case((pts, P, world), huber=huber)


def _mask_2of4():
    rig = noisy(ring_rig(2, 4, 5, 33), 133)
    pairs = (0b0011, 0b0110, 0b1100, 0b1001)                          # neighbours on the ring: 90 degrees apart
    views = np.array([[pairs[(b + k) % 4] for k in range(5)] for b in range(2)], np.uint8)
    return _case(rig, views=views)


def _invalid_bit():
    pts, P, world = noisy(ring_rig(2, 4, 5, 34), 134)
    pts[:, 2, :, :2] += 300.0                                         # garbage in a view whose weight says so
    pts[:, 2, :, 2] = 0.0
    return _case((pts, P, world), views=np.full((2, 5), 0b1111, np.uint8))


def _dead_weights():
    pts, P, world = noisy(ring_rig(2, 6, 5, 35), 135)
    for k, bad in enumerate((0.0, np.nan, -1.0, np.inf, -np.inf)):    # joint k loses view k, and view k + 1 the same way
        for v in (k, k + 1):
            pts[:, v, k, :2] += 300.0
            pts[:, v, k, 2] = bad
    return _case((pts, P, world))


def _one_valid():
    pts, P, world = noisy(ring_rig(2, 3, 5, 36), 136)
    pts[:, 1:, :, 2] = 0.0
    init = np.concatenate([world, np.ones((2, 5, 1), np.float32)], -1).astype(np.float32)
    init[1, 2, :3] = np.nan                                           # what the robust kernel writes there
    return _case((pts, P, world), init=init)


def _nan_init():
    c = _case(noisy(ring_rig(2, 4, 5, 37), 137))
    c['init'][0, 1, 0] = np.nan
    c['init'][1, 3, 2] = np.inf
    c['init'][1, 4, :3] = np.nan
    return c


def _behind():
    pts, P, world = ring_rig(2, 4, 5, 38)
    P[:, 1, 2, :] = -P[:, 1, 2, :]                                    # view 1 looks the other way: every point is behind it
    pts = project(P, world)
    pts[..., 2] = np.abs(pts[..., 2])
    init = np.concatenate([world, np.ones((2, 5, 1), np.float32)], -1).astype(np.float32)
    return _case((pts, P, world), init=init)


def _robust():
    """Half a pixel of noise, then one view of 8 joints moved far out (test_gpu_tri_robust.plant: decidable for the robust
    oracle).  `views` and `init` are the robust ORACLE's here; the GPU test feeds the device's."""
    pts, P, world = noisy(ring_rig(2, 4, 12, 39), 139, sigma=0.5)
    pts, planted = plant(pts, P, 1, 8, thr=THR, cover=False)
    o = to.robust(pts, P, THR)
    c = _case((pts, P, world), views=o['mask'])
    c.update(planted=planted, robust=o)
    return c


def _illcond():
    """Two cameras 1 cm apart: a disparity of 1100 px * 10 mm / 4 m = 2.8 px.  Noise of 2 px would leave half of the joints
    with rays that never meet (a minimum at infinity, a DLT point behind the cameras), so the noise is 0.2 px here and the start
    is the planted point moved by a few cm, not the DLT.  The depth stays next to undetermined: cond ~ 1e5."""
    pts, P, world = noisy(ring_rig(2, 2, 5, 40, baseline_mm=10.0), 140, sigma=0.2)
    init = np.concatenate([world + np.array([20.0, -10.0, 30.0], np.float32), np.ones((2, 5, 1), np.float32)], -1).astype(np.float32)
    return _case((pts, P, world), init=init, compare=False)


CASES = {}
for _B, _V, _K in SHAPES:
    CASES['clean_b%dv%dk%d' % (_B, _V, _K)] = functools.partial(lambda B, V, K: _case(ring_rig(B, V, K, 100 * V + K + B)), _B, _V, _K)
    CASES['noisy_b%dv%dk%d' % (_B, _V, _K)] = functools.partial(
        lambda B, V, K: _case(noisy(ring_rig(B, V, K, 200 * V + K + B), 300 * V + K + B)), _B, _V, _K)
CASES.update({
    'weighted': _weighted,
    'huber': lambda: _huber(3.0),
    'huber_off': lambda: _huber(0.0),              # the same inputs under plain least squares
    'mask_2of4': _mask_2of4,
    'invalid_bit': _invalid_bit,
    'dead_weights': _dead_weights,
    'one_valid': _one_valid,
    'nan_init': _nan_init,
    'behind': _behind,
    'robust': _robust,
    'illcond': _illcond,
})
CLEAN = tuple(n for n in CASES if n.startswith('clean'))
NOISY = tuple(n for n in CASES if n.startswith('noisy'))
PASSED_THROUGH = ('one_valid', 'behind')           # every joint; nan_init: three of its joints


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, oracle result) of one case, computed once per process and shared; treat both as read-only."""
    c = CASES[name]()
    return c, ro.refine(c['points'], c['P'], c['init'], c['views'], c['weighted'], c['huber'])


def compared(name):
    """[B,K] bool: the joints whose position is compared with the oracle's."""
    c, o = case(name)
    return ~o['passed'] & (o['cond'] <= ro.COND_MAX) if c['compare'] else np.zeros(o['passed'].shape, bool)


# ------------------------------------------------------------------------------------------------ the device side
WANT = ('resid', 'cov', 'status')


def run(c, init=None, views='case', max_iter=20, want=WANT, **kw):
    from xas_amd import ops_eval
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = ops_eval.triangulate_refine(d(c['points']), d(c['P']), d(c['init'] if init is None else init),
                                      views=d(c['views'] if isinstance(views, str) else views), weighted=kw.get('weighted', c['weighted']),
                                      huber_px=kw.get('huber', c['huber']), max_iter=max_iter, want=want)
    return {k: v.cpu() for k, v in out.items()}


def ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def bits(t):
    return t.contiguous().unsqueeze(-1).view(torch.uint8)


def planted_tol(c, o):
    """[B,K] mm: how far the minimum of a noise-free case may lie from the planted point.  The points are the exact projections
    rounded to float32, so every residual component at the planted point is at most half an ulp of the pixel coordinate, and to
    first order the minimum moves by (J^T J)^-1 J^T dr, whose norm is at most |dr|_2 / sigma_min(J) = |dr|_2 sqrt(lambda_max(cov))
    (unweighted, no Huber: cov = (J^T J)^-1); second order is smaller by |dr| / depth.  + the kernel's distance from the oracle."""
    cov = np.zeros(o['cov'].shape[:2] + (3, 3))
    iu = np.triu_indices(3)
    cov[..., iu[0], iu[1]] = o['cov']
    cov[..., iu[1], iu[0]] = o['cov']
    dr = np.sqrt(2.0 * c['points'].shape[1]) * ulp32(np.abs(c['points'][..., :2]).max()) / 2
    return np.sqrt(np.linalg.eigvalsh(cov)[..., -1]) * dr + 1e-4 + 2 * ulp32(np.abs(c['world']).max(-1))


def check_cost(c, got, init=None, views='case', name=''):
    """C(out) <= C(init), both evaluated in double from the float32 numbers."""
    v = c['views'] if isinstance(views, str) else views
    C1, slack = ro.cost_at(c['points'], c['P'], got['xyzw'][..., :3].numpy(), v, c['weighted'], c['huber'])
    C0, _ = ro.cost_at(c['points'], c['P'], (c['init'] if init is None else init)[..., :3], v, c['weighted'], c['huber'])
    solved = (got['status'].numpy() != 2)
    over = (C1 - C0 - slack)[solved]
    print('%s: C(out) - C(init) max %.3g (slack %.3g)' % (name, (C1 - C0)[solved].max(), slack[solved].max()))
    assert (over <= 0).all(), (name, over.max())


def check_vs_oracle(name, got=None, o=None):
    """What every case asserts: status 2 and init's bits exactly where the oracle passes through, elsewhere the oracle's
    position (joints with cond <= 1e3), resid and cov within the bounds of the docstring, and the cost never above init's."""
    c, o_case = case(name)
    o = o_case if o is None else o
    got = run(c) if got is None else got
    st = got['status'].numpy()
    assert got['status'].dtype == torch.uint8 and np.array_equal(st == 2, o['passed']), (name, st)
    through = torch.from_numpy(o['passed'])
    assert torch.equal(bits(got['xyzw'])[through], bits(torch.from_numpy(c['init']))[through])
    assert torch.isnan(got['resid'][through]).all() and torch.isnan(got['cov'][through]).all()
    assert torch.equal(bits(got['xyzw'][..., 3]), bits(torch.from_numpy(c['init'][..., 3])))         # the fourth entry is copied
    if o['passed'].all():
        return c, o, got
    solved = ~o['passed']
    assert np.isfinite(got['xyzw'].numpy()[solved]).all() and np.isfinite(got['resid'].numpy()[solved]).all()
    assert np.isfinite(got['cov'].numpy()[solved]).all()
    cmp = compared(name)
    xyz = got['xyzw'][..., :3].double().numpy()
    with np.errstate(invalid='ignore'):                               # NaN where a NaN start was passed through
        err = np.abs(xyz - o['xyz']).max(-1)
    tol = 1e-4 + 2 * ulp32(np.abs(o['xyz']).max(-1))
    resid = got['resid'].double().numpy()
    e0 = np.abs(resid[..., 0] - o['resid'][..., 0])
    e1 = np.abs(resid[..., 1] - o['resid'][..., 1])
    rtol = lambda a: 4 * ulp32(a) + 1e-6
    cov = got['cov'].double().numpy()
    ecov = np.abs(cov - o['cov']).max(-1)
    ctol = 4 * ulp32(np.abs(o['cov']).max(-1)) + o['cov_shift']
    assert (e0[solved] <= rtol(o['resid'][..., 0])[solved]).all(), (name, e0[solved].max())
    if cmp.any():
        print('%s: %d of %d joints compared, |xyz - oracle| max %.3g mm (tolerance %.3g), resid before %.3g after %.3g px, '
              'cov %.3g of its tolerance, cond max %.3g, status %s' % (
                  name, cmp.sum(), cmp.size, err[cmp].max(), tol[cmp].min(), e0[cmp].max(), e1[cmp].max(),
                  (ecov / ctol)[cmp].max(), o['cond'][cmp].max(), np.bincount(st.ravel(), minlength=3)))
        assert (err[cmp] <= tol[cmp]).all(), (name, err[cmp].max())
        r1tol = rtol(o['resid'][..., 1]) + o['resid_shift']
        print('%s: resid after refinement off by %.3g of its bound, %.3g of the bound without the shift term' % (
            name, (e1 / r1tol)[cmp].max(), (e1 / rtol(o['resid'][..., 1]))[cmp].max()))
        assert (e1[cmp] <= r1tol[cmp]).all(), (name, e1[cmp].max())
        assert (ecov[cmp] <= ctol[cmp]).all(), (name, (ecov / ctol)[cmp].max())
    check_cost(c, got, name=name)
    return c, o, got


@pytest.mark.parametrize('name', CLEAN)
def test_exact_projections_stay_at_the_planted_point(name):
    from xas_amd import ops_eval
    c, o, got = check_vs_oracle(name)
    assert (got['status'] == 0).all()
    assert (got['resid'][..., 1] <= got['resid'][..., 0]).all()
    tol = planted_tol(c, o)
    print('%s: off the planted point by %.3g mm at most (tolerance %.3g)' % (
        name, np.abs(got['xyzw'][..., :3].double().numpy() - c['world']).max(), tol.min()))
    assert (np.abs(got['xyzw'][..., :3].double().numpy() - c['world']).max(-1) <= tol).all()
    # init is the DLT: the device's own
    dlt = ops_eval.triangulate_dlt(torch.from_numpy(c['points']).cuda(), torch.from_numpy(c['P']).cuda()).cpu().numpy()
    dev = run(c, init=dlt)
    assert (dev['status'] == 0).all() and (dev['resid'][..., 1] <= dev['resid'][..., 0]).all()
    assert (np.abs(dev['xyzw'][..., :3].double().numpy() - c['world']).max(-1) <= tol).all()
    check_cost(c, dev, init=dlt, name=name + ' from the device DLT')


@pytest.mark.parametrize('name', NOISY)
def test_noisy_points_reach_the_oracles_minimum(name):
    c, o, got = check_vs_oracle(name)
    # status 0 or 1: next to the minimum a step of ~1e-6 mm changes a cost of ~50 px^2 by less than double precision resolves, so
    # a joint may spend its remaining trials on rejected steps and end as "out of trials" at the same point
    assert (got['status'] != 2).all()
    assert (got['resid'][..., 1] <= got['resid'][..., 0]).all()


def test_weights_scale_the_residuals():
    c, o, got = check_vs_oracle('weighted')
    plain = ro.refine(c['points'], c['P'], c['init'], None, False, 0.0)
    tol = 1e-4 + 2 * ulp32(np.abs(o['xyz']).max(-1))
    assert (np.abs(o['xyz'] - plain['xyz']).max(-1) > 10 * tol).all()                 # the two minima are different points
    unw = run(c, weighted=False)
    assert (np.abs(unw['xyzw'][..., :3].double().numpy() - plain['xyz']).max(-1) <= tol).all()
    assert (np.abs(got['xyzw'][..., :3].double().numpy() - plain['xyz']).max(-1) > 10 * tol).all()


def test_huber_holds_a_displaced_view_back():
    # under Huber's loss the IRLS weights make the convergence linear (a rate of up to 0.6 on these inputs, where noise of 2 px
    # puts inliers next to delta = 3 px too), so the step rule needs more than the default 20 trials: with 64 every joint comes
    # within 1e-5 * 0.6 / 0.4 mm of the minimum (status 0, or 1 where the last steps fall under what the cost resolves, as in the
    # noisy cases)
    c, _ = case('huber')
    c, o, got = check_vs_oracle('huber', got=run(c, max_iter=64))
    assert (got['status'] != 2).all()
    c0, o0, got0 = check_vs_oracle('huber_off')
    assert np.array_equal(c['points'], c0['points'])
    d = lambda g: np.linalg.norm(g['xyzw'][..., :3].double().numpy() - c['world'], axis=-1)
    print('huber: off the planted point by %.3g mm at most, %.3g mm without' % (d(got).max(), d(got0).max()))
    assert (d(got) < d(got0)).all()


def test_huber_at_the_default_trials_stands_where_the_specified_loop_stands():
    """max_iter = 20 is what eval.py runs.  There the slow joints have not converged, so the minimum is the wrong yardstick; the
    header's loop restated in float64 (_refine_oracle.schedule) is the right one.  Both run the same trials in double, and a
    contracting iteration does not amplify their rounding differences; only a trial whose acceptance hangs on the last bits of the
    cost can be decided differently, and such a trial is shorter than the step rule's 1e-5 mm.  So |d|_inf <= 1e-5 mm + 2 ulp_fp32.
    From the minimum the kernel then stands no farther than the restated loop does, + that."""
    c, o = case('huber')
    got = run(c)
    want = ro.schedule(c['points'], c['P'], c['init'], c['views'], c['weighted'], c['huber'], max_iter=20)
    xyz = got['xyzw'][..., :3].double().numpy()
    tol = 1e-5 + 2 * ulp32(np.abs(want['xyz']).max(-1))
    err = np.abs(xyz - want['xyz']).max(-1)
    left = np.abs(want['xyz'] - o['xyz']).max(-1)
    print('huber at 20 trials: |xyz - restated loop| max %.3g mm (tolerance %.3g); the loop stands %.3g mm from the minimum at most, '
          'the kernel %.3g; status %s, restated %s' % (err.max(), tol.min(), left.max(), np.abs(xyz - o['xyz']).max(),
                                                        np.bincount(got['status'].numpy().ravel(), minlength=3),
                                                        np.bincount(want['status'].ravel(), minlength=3)))
    assert (err <= tol).all(), err.max()
    assert (np.abs(xyz - o['xyz']).max(-1) <= left + tol).all()
    assert (got['status'] != 2).all()
    check_cost(c, got, name='huber at 20 trials')


def test_view_masks_select_the_views():
    c, o, got = check_vs_oracle('mask_2of4')
    assert np.array_equal(o['used'], c['views'])
    full = run(c, views=None)
    assert not torch.equal(full['xyzw'], got['xyzw'])                                 # the mask does something
    c, _ = case('noisy_b2v4k5')
    a, z = run(c, views=None), run(c, views=np.zeros((2, 5), np.uint8))               # byte 0 = NULL = all valid views
    for k in a:
        assert torch.equal(bits(a[k]), bits(z[k])), k


def test_invalid_views_are_skipped_whatever_the_mask_says():
    c, o, got = check_vs_oracle('invalid_bit')
    assert (o['used'] == 0b1011).all()
    for views in (None, np.full((2, 5), 0b1011, np.uint8), np.full((2, 5), 0b11111011, np.uint8)):   # bits >= V are ignored too
        other = run(c, views=views)
        for k in got:
            assert torch.equal(bits(other[k]), bits(got[k])), k
    c, o, got = check_vs_oracle('dead_weights')
    assert [int(m) for m in o['used'][0]] == [0b111100, 0b111001, 0b110011, 0b100111, 0b001111]


def test_pass_through_is_bit_identical():
    for name in PASSED_THROUGH:
        c, o, got = check_vs_oracle(name)
        assert (got['status'] == 2).all(), name
        assert torch.equal(bits(got['xyzw']), bits(torch.from_numpy(c['init']))), name
    c, o, got = check_vs_oracle('nan_init')
    assert got['status'][0, 1] == 2 and got['status'][1, 3] == 2 and got['status'][1, 4] == 2 and (got['status'] == 2).sum() == 3


def test_one_trial_still_lowers_the_cost():
    c, _ = case('noisy_b2v4k5')
    got = run(c, max_iter=1)
    assert (got['status'] == 1).all()
    check_cost(c, got, name='max_iter=1')
    assert (got['resid'][..., 1] < got['resid'][..., 0]).all()


def test_after_the_robust_solver():
    from xas_amd import ops_eval
    c, o = case('robust')
    r = ops_eval.triangulate_robust(torch.from_numpy(c['points']).cuda(), torch.from_numpy(c['P']).cuda(), threshold_px=THR)
    assert np.array_equal(r['inliers'].cpu().numpy(), c['robust']['mask'])
    full = (1 << c['points'].shape[1]) - 1
    assert np.array_equal(c['robust']['mask'], full & ~c['planted']) and np.count_nonzero(c['planted']) == 8
    init, views = r['xyzw'].cpu().numpy(), r['inliers'].cpu().numpy()
    got = run(c, init=init, views=views)                              # fed straight in
    want = ro.refine(c['points'], c['P'], init, views, False, 0.0)
    cmp = want['cond'] <= ro.COND_MAX
    assert cmp.all()
    err = np.abs(got['xyzw'][..., :3].double().numpy() - want['xyz']).max(-1)
    assert (err <= 1e-4 + 2 * ulp32(np.abs(want['xyz']).max(-1))).all(), err.max()
    assert (got['status'] != 2).all()
    # resid before = the robust kernel's resid, but at its point ROUNDED to float32: the DLT point is no minimum of the pixel
    # error, so the RMS moves with it, by at most the steepest view's f / depth = 1200 px / 2900 mm per mm, over a rounding of
    # at most sqrt(3) / 2 ulp of the largest coordinate
    moved = 1200.0 / 2900.0 * np.sqrt(3.0) / 2 * ulp32(np.abs(init[..., :3]).max(-1))
    np.testing.assert_array_less(np.abs(got['resid'][..., 0].numpy() - r['resid'].cpu().numpy()),
                                 4 * ulp32(r['resid'].cpu().numpy()) + 1e-6 + moved)
    check_cost(c, got, init=init, views=views, name='robust')


def test_ill_conditioned_pair_only_lowers_the_cost():
    c, o, got = check_vs_oracle('illcond')                            # compares no position
    assert (o['cond'] > ro.COND_MAX).all()
    for k in ('xyzw', 'resid', 'cov'):
        assert torch.isfinite(got[k]).all(), k


def test_optional_outputs_and_two_launches():
    c, _ = case('noisy_b3v4k5')
    full, again, bare = run(c), run(c), run(c, want=())
    assert set(bare) == {'xyzw'} and torch.equal(bits(bare['xyzw']), bits(full['xyzw']))
    for k in full:
        assert torch.equal(bits(full[k]), bits(again[k])), k
    only = run(c, want=('cov',))
    assert set(only) == {'xyzw', 'cov'} and torch.equal(only['cov'], full['cov'])


def test_refusals_name_the_limit():
    from xas_amd import ops_eval
    t = lambda *s: torch.ones(*s).cuda()
    args = lambda V, K=3: (t(1, V, K, 3), t(1, V, 3, 4), t(1, K, 4))
    with pytest.raises(RuntimeError, match=r'V=1 views \(needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6\)'):
        ops_eval.triangulate_refine(*args(1))
    with pytest.raises(RuntimeError, match=r'V=7 views \(needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6\)'):
        ops_eval.triangulate_refine(*args(7))
    for bad in (0, 65):
        with pytest.raises(RuntimeError, match=r'max_iter=%d trials \(needs 1 <= max_iter <= 64\)' % bad):
            ops_eval.triangulate_refine(*args(3), max_iter=bad)
    p, P, i = args(3)
    with pytest.raises(RuntimeError, match='do not match points'):
        ops_eval.triangulate_refine(p, t(1, 4, 3, 4), i)
    with pytest.raises(RuntimeError, match='start points .* do not match'):
        ops_eval.triangulate_refine(p, P, t(1, 4, 4))
    with pytest.raises(RuntimeError, match='views .* are not the'):
        ops_eval.triangulate_refine(p, P, i, views=t(1, 3))


# ------------------------------------------------------------------------------------------------ Eval
def _eval_setup():
    x, kps, _ = eval_case()
    cams = [0, 1, 2, 3]
    xd = {k: v.cuda() for k, v in x.items()}
    det = PlantedDetector()
    det.kps = {}
    for i, c in enumerate(cams):
        xd['cam_%d_img' % c] = torch.full((1, 3, 256, 256), float(i), device='cuda')
        det.kps[i] = kps[c][1].cuda()
    return cams, xd, det


def _cfg_with(cams, **keys):
    cfg = _cfg(cams)
    cfg['model_params'].update(keys)
    return cfg


@pytest.mark.parametrize('tri', ['dlt', 'robust'])
def test_eval_batch_refines_only_when_asked(tmp_path, tri):
    import eval as xeval
    from modules import util as mu
    from xas_amd import ops_eval
    cams, xd, det = _eval_setup()
    mk = lambda **keys: xeval.Eval(_cfg_with(cams, **keys), det, [], str(tmp_path), tri=tri)
    today, none = mk().eval_batch(xd, 'best'), mk(tri_refine='none').eval_batch(xd, 'best')
    assert set(none) == set(today) and all(torch.equal(bits(none[k]), bits(today[k])) for k in today)
    lm = mk(tri_refine='lm').eval_batch(xd, 'best')
    assert set(lm) == set(today) | {'tri_refine_px', 'tri_refine_gain_px'}
    assert lm['tri_refine_px'].dim() == 0 and lm['tri_refine_px'].is_cuda
    assert float(lm['tri_refine_gain_px']) >= 0 and float(lm['tri_refine_px']) >= 0
    sel = {'cam_%d' % c: ops_eval.eval_select(det.kps[i], xd['cam_%d_joints' % c], mode='best')['sel3d'] for i, c in enumerate(cams)}
    tri_px = THR if tri == 'robust' else None
    direct, r = mu.triangulation_refined(sel, xd, cams, robust_px=tri_px, want=('resid', 'status'))
    assert torch.equal(lm['world_tri'], direct) and not torch.equal(lm['world_tri'], today['world_tri'])
    assert (r['status'] != 2).all()
    want = float(r['resid'][..., 1].double().mean())                          # a float32 mean of n terms: n ulp at the worst
    assert abs(float(lm['tri_refine_px']) - want) <= r['resid'][..., 1].numel() * 2.0 ** -23 * want
    for k in today:                                                           # nothing but the triangulated pose moves
        if 'tri' not in k:
            assert torch.equal(lm[k], today[k]), k
    if tri == 'robust':
        assert torch.equal(lm['tri_inlier_views'], today['tri_inlier_views']) and torch.equal(r['inliers'], mu.triangulation(
            sel, xd, cams, robust_px=THR, return_inliers=True)[1])


def test_result_file_gains_one_line_with_lm_only(tmp_path):
    import eval as xeval
    cams, xd, det = _eval_setup()
    texts = {}
    for tag, keys in (('today', {}), ('none', dict(tri_refine='none')), ('lm', dict(tri_refine='lm', tri_huber=3.0))):
        e = xeval.Eval(_cfg_with(cams, **keys), det, [dict(xd), dict(xd)], str(tmp_path / tag))
        lines = e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt', 'rb').read()
        assert texts[tag].decode().strip().split('\n') == lines
    assert texts['none'] == texts['today']
    old, new = texts['today'].decode().strip().split('\n'), texts['lm'].decode().strip().split('\n')
    assert len(new) == len(old) + 1 and new[-1].startswith('TRI refine lm (huber 3.0): reprojection RMS ') and ' px, gained ' in new[-1]
    with pytest.raises(ValueError, match='Unknown triangulation refinement: gn'):
        xeval.Eval(_cfg_with(cams, tri_refine='gn'), det, [], str(tmp_path))
    with pytest.raises(ValueError, match="tri_refine='lm' refines over at most 6 cameras; cam_id_list has 7"):
        xeval.Eval(_cfg_with(list(range(7)), tri_refine='lm'), det, [], str(tmp_path))
