"""xas_triangulate_skeleton on the MI355X against its float64 restatement (tests/_skeleton_oracle.py), from the kernel up to
Eval.eval_batch and the result file.

Inputs are built on the CPU (CASES) from tests/_refine_inputs.py: the ring of cameras, and skeletons whose b-side joints are the
exact mirror images (x negated, exact in float32) of their a-side joints, so every planted limb pair is symmetric to the last
bit; then seeded pixel noise, weights, a displaced view, dead views, view masks.  The start is the float64 DLT rounded to
float32 (_refine_oracle.dlt_start), so tests/test_tri_skeleton_abi.py validates these very inputs without a GPU.

Tolerances (derived, not tuned):
  position, decoupled (sym_w = 0 or L = 0): the problem is xas_triangulate_refine's, joint by joint, and so is the bound of
            tests/test_gpu_tri_refine.py: 1e-4 mm + 2 ulp_fp32(max |coordinate|) for joints with cond <= 1e3.
  position, coupled: the same form, 1e-4 mm + 2 ulp_fp32.  The 1e-4 mm has two parts, both taken from the oracle on the CPU
            and asserted there for every compared case (test_tri_skeleton_abi.py):  (a) the stop rule: the loop ends on an
            accepted step whose largest coordinate is under 1e-5 mm; at a linear rate r the distance left is at most that times
            r / (1 - r).  r is read off the accepted steps of `_skeleton_oracle.schedule`, the header's loop in float64 (never
            off the kernel).  (b) the cost's resolution: a step from distance d lowers C by at least lambda_min(H) d^2, and each
            of the two costs compared carries a rounding error of up to ~16 eps C, so a trial can be refused wrongly only within
            d <= sqrt(32 eps C / lambda_min) of the minimum (`floor`).  The CPU file asserts 1e-5 r / (1 - r) + floor <= 1e-4 mm
            for every sample compared (cond <= 1e3), and that the restated loop itself ends within it.
  resid, sym, cost: at init 4 float32 ulp of the value (+ 1e-6 px for resid): both sides read the same float32 numbers.  At the
            result that + the oracle's own change when every coordinate moves by the position tolerance (`*_shift`).
  cost does not rise: C(out) <= C(init) in float64 from the float32 outputs, with the slack of one rounding of out
            (_skeleton_oracle.cost_at).
The largest share of the position bound that each case used on the device is in profiles/tri_skeleton_check.txt.
"""
import functools
import os

import numpy as np
import pytest
import torch

import _refine_oracle as ro
import _skeleton_oracle as so
import _tri_oracle as to
from _refine_inputs import noisy, project, ring_rig

pytestmark = pytest.mark.gpu
SYM_LIMBS = ((16, 15, 13, 12), (15, 14, 12, 11), (3, 2, 6, 5), (2, 1, 5, 4))
# 24 joints, b side = a side + 12; 16 limb pairs over the a side: a chain and five chords, so joints stand in up to four pairs
LIMBS_MAX = tuple((i + 1, i, i + 13, i + 12) for i in range(11)) + tuple((i + 2, i, i + 14, i + 12) for i in range(5))
MIRROR = {4: ((2, 0), (3, 1)), 18: ((4, 1), (5, 2), (6, 3), (11, 14), (12, 15), (13, 16)), 24: tuple((i + 12, i) for i in range(12))}
LIMBS = {(4, 1): ((1, 0, 3, 2),), (18, 4): SYM_LIMBS, (24, 16): LIMBS_MAX, (18, 0): ()}
SHAPES = ((1, 2, 4, 1), (2, 4, 18, 4), (3, 6, 24, 16), (65, 4, 18, 4), (2, 4, 18, 0))
THR = 20.0
CHECK_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'tri_skeleton_check.txt')


# ------------------------------------------------------------------------------------------------ inputs (CPU only)
def sym_rig(B, V, K, seed, **kw):
    """ring_rig with the b-side joints mirrored from the a side: every limb pair of LIMBS is exactly symmetric."""
    _, P, world = ring_rig(B, V, K, seed, **kw)
    for dst, src in MIRROR[K]:
        world[:, dst] = world[:, src] * np.array([-1.0, 1.0, 1.0], np.float32)
    return project(P, world), P, world


def _case(rig, L, sym_w, views=None, weighted=False, huber=0.0, init=None, compare=True, max_iter=20):
    pts, P, world = rig
    return dict(points=pts, P=P, world=world, views=views, weighted=weighted, huber=huber, compare=compare, sym_w=sym_w,
                limbs=LIMBS[(pts.shape[2], L)], max_iter=max_iter, init=ro.dlt_start(pts, P, views) if init is None else init)


def _weighted(sym_w):
    """Every view has its own sigma, 0.3 to 1 px over the views, noise of that size, and 1 / sigma as its weight.  (A wider span,
    such as the 0.5 to 5 px of test_gpu_tri_refine.py, leaves the depth along the sharpest view to views that weigh 1 / 100 of it;
    against sym_w = 10 that alone puts the condition number over COND_MAX.)"""
    pts, P, world = sym_rig(2, 4, 18, 51)
    rng = np.random.Generator(np.random.PCG64(151))
    sigma = np.array([0.3, 1.0, 0.5, 0.7])[None, :, None] * rng.uniform(0.9, 1.0, (2, 4, 18))
    pts[..., :2] += (sigma[..., None] * rng.normal(0.0, 1.0, (2, 4, 18, 2))).astype(np.float32)
    pts[..., 2] = (1.0 / sigma).astype(np.float32)
    return _case((pts, P, world), 4, sym_w, weighted=True)


def _huber(sym_w):
    pts, P, world = noisy(sym_rig(2, 4, 18, 62), 162, sigma=1.0)      # 1 px: few inliers in Huber's linear part, so H keeps its rank
    for b in range(2):
        for k in range(18):
            pts[b, (b + k) % 4, k, :2] += np.float32(40.0) * np.array([0.6, -0.8], np.float32)        # 40 px off
    return _case((pts, P, world), 4, sym_w, huber=3.0, max_iter=64)


def _robust(sym_w):
    """Half a pixel of noise, one view of 8 joints moved far out; `views` and `init` are the robust ORACLE's here, the GPU
    test feeds the device's own."""
    from test_gpu_tri_robust import plant
    pts, P, world = noisy(sym_rig(2, 4, 18, 53), 153, sigma=0.5)
    pts, planted = plant(pts, P, 1, 8, thr=THR, cover=False)
    o = to.robust(pts, P, THR)
    c = _case((pts, P, world), 4, sym_w, views=o['mask'])
    c.update(planted=planted, robust=o)
    return c


def _fixed():
    """Sample 0: joint k loses two views to a dead weight (0, NaN, -1, +inf, -inf) and stays free on the other four; joint 6
    keeps one valid view, joint 12 has a NaN x at init, joint 15 an inf z, joint 2 all-NaN init: fixed.  Sample 1: every joint
    down to one valid view: nothing is free.  Sample 2: untouched."""
    pts, P, world = noisy(sym_rig(3, 6, 18, 54), 154)
    for k, bad in enumerate((0.0, np.nan, -1.0, np.inf, -np.inf)):
        for v in (k, k + 1):
            pts[0, v, 7 + k, :2] += 300.0
            pts[0, v, 7 + k, 2] = bad
    pts[0, 1:, 6, 2] = 0.0
    pts[1, 1:, :, 2] = 0.0
    c = _case((pts, P, world), 4, 0.1)
    c['init'][0, 12, 0] = np.nan
    c['init'][0, 15, 2] = np.inf
    c['init'][0, 2, :3] = np.nan
    c['init'][1, :, :3] = world[1]
    c['init'][1, :, 3] = 1.0
    c['init'][1, 5, :3] = np.nan
    return c


FIXED_JOINTS = {0: (2, 6, 12, 15), 1: tuple(range(18)), 2: ()}


def _behind():
    """Joints 3 and 16 of sample 0 start behind camera 1 (on its ray through the planted point, 1.5 times as far on the other
    side of its centre): both are fixed, which switches pairs 0 and 2 off and leaves pairs 1 and 3 to pull."""
    pts, P, world = noisy(sym_rig(2, 4, 18, 55), 155)
    c = _case((pts, P, world), 4, 10.0)
    c['init'][0, 3, :3] = world[0, 3] + (world[0, 3] - _centre(P[0, 1])) * np.float32(-2.5)           # beyond camera 1
    c['init'][0, 16, :3] = world[0, 16] + (world[0, 16] - _centre(P[0, 1])) * np.float32(-2.5)
    return c


def _centre(Pm):
    return (-np.linalg.inv(Pm[:, :3].astype(np.float64)) @ Pm[:, 3].astype(np.float64)).astype(np.float32)


def _flat():
    """Joints 16 and 15 start on the same point: limb a of pair 0 has length 0 at init."""
    c = _case(noisy(sym_rig(2, 4, 18, 56), 156), 4, 10.0, compare=False)
    c['init'][0, 16] = c['init'][0, 15]
    return c


def _illcond():
    """Two cameras 1 cm apart (the case of test_gpu_tri_refine.py): the depth is next to undetermined, cond ~ 1e5."""
    pts, P, world = noisy(sym_rig(2, 2, 18, 57, baseline_mm=10.0), 157, sigma=0.2)
    init = np.concatenate([world + np.array([20.0, -10.0, 30.0], np.float32), np.ones((2, 18, 1), np.float32)], -1).astype(np.float32)
    return _case((pts, P, world), 4, 0.1, init=init, compare=False)


CASES = {}
for _w in (0.1, 10.0):
    _t = 'w%g_' % _w
    CASES[_t + 'clean'] = functools.partial(lambda w: _case(sym_rig(2, 4, 18, 41), 4, w), _w)
    for _B, _V, _K, _L in SHAPES[:3]:
        CASES[_t + 'noisy_b%dv%dk%dl%d' % (_B, _V, _K, _L)] = functools.partial(
            lambda B, V, K, L, w: _case(noisy(sym_rig(B, V, K, 400 * V + K + B), 500 * V + K + B), L, w), _B, _V, _K, _L, _w)
    CASES[_t + 'weighted'] = functools.partial(_weighted, _w)
    CASES[_t + 'huber'] = functools.partial(_huber, _w)
    CASES[_t + 'robust'] = functools.partial(_robust, _w)
CASES['w0.1_noisy_b65v4k18l4'] = lambda: _case(noisy(sym_rig(65, 4, 18, 42), 142), 4, 0.1)
COUPLED = tuple(CASES)
CASES.update({
    'decoupled_w0': lambda: _case(noisy(sym_rig(2, 4, 18, 43), 143), 4, 0.0),
    'decoupled_l0': lambda: _case(noisy(sym_rig(2, 4, 18, 44), 144), 0, 10.0),
    'fixed': _fixed,
    'behind': _behind,
    'flat': _flat,
    'illcond': _illcond,
    'one_trial': lambda: _case(noisy(sym_rig(2, 4, 18, 45), 145), 4, 0.1, compare=False, max_iter=1),
})
DECOUPLED = ('decoupled_w0', 'decoupled_l0')


def _kw(c):
    return dict(views=c['views'], limbs=c['limbs'], weighted=c['weighted'], huber=c['huber'], sym_w=c['sym_w'])


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, oracle result) of one case, computed once per process and shared; treat both as read-only."""
    c = CASES[name]()
    return c, so.refine(c['points'], c['P'], c['init'], **_kw(c))


def compared(name):
    """[B] bool: the samples whose positions are compared with the oracle's."""
    c, o = case(name)
    return (o['cond'] <= so.COND_MAX) if c['compare'] else np.zeros(len(o['cond']), bool)


# ------------------------------------------------------------------------------------------------ the device side
WANT = ('resid', 'sym', 'cost', 'status')


def run(c, init=None, views='case', want=WANT, poison=None, **kw):
    from xas_amd import ops_eval
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = ops_eval.triangulate_skeleton(d(c['points']), d(c['P']), d(c['init'] if init is None else init),
                                        views=d(c['views'] if isinstance(views, str) else views), limbs=c['limbs'],
                                        weighted=c['weighted'], huber_px=c['huber'], sym_w=kw.get('sym_w', c['sym_w']),
                                        max_iter=kw.get('max_iter', c['max_iter']), want=want)
    return {k: v.cpu() for k, v in out.items()}


def ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def bits(t):
    return t.contiguous().unsqueeze(-1).view(torch.uint8)


def note(name, text):
    """One line per case in profiles/tri_skeleton_check.txt (rewritten case by case, kept sorted)."""
    lines = {}
    if os.path.exists(CHECK_FILE):
        lines = dict(l.rstrip('\n').split(': ', 1) for l in open(CHECK_FILE) if ': ' in l and not l.startswith('#'))
    lines[name] = text
    if not os.access(os.path.dirname(CHECK_FILE), os.W_OK):           # a read-only checkout: the figures are printed above
        return
    with open(CHECK_FILE, 'w') as f:
        f.write('# xas_triangulate_skeleton on the MI355X against tests/_skeleton_oracle.py: per case of tests/test_gpu_tri_skeleton.py\n'
                '# the largest |xyz - oracle| over its position bound (1e-4 mm + 2 ulp_fp32), and the same for resid, sym and cost\n')
        for k in sorted(lines):
            f.write('%s: %s\n' % (k, lines[k]))


def check_cost(c, got, init=None, views='case', name=''):
    v = c['views'] if isinstance(views, str) else views
    i = c['init'] if init is None else init
    kw = dict(_kw(c), views=v)
    C1, slack = so.cost_at(c['points'], c['P'], i, got['xyzw'][..., :3].numpy(), **kw)
    C0, _ = so.cost_at(c['points'], c['P'], i, i[..., :3], **kw)
    print('%s: C(out) - C(init) max %.3g (slack %.3g)' % (name, (C1 - C0).max(), slack.max()))
    assert (C1 - C0 - slack <= 0).all(), (name, (C1 - C0 - slack).max())


def check_vs_oracle(name, got=None, o=None, c=None):
    """What every case asserts: fixed joints are init's bits with status 2 and NaN resid, pairs that are not active have NaN
    sym; and for the samples compared, position, resid, sym and cost within the bounds of the docstring; the cost never rises."""
    if c is None:
        c, o = case(name)
    got = run(c) if got is None else got
    init = torch.from_numpy(c['init'])
    free, act = o['free'], o['active']
    st = got['status'].numpy()
    assert got['status'].dtype == torch.uint8 and np.array_equal(st != 2, free), (name, st)
    fixed = torch.from_numpy(~free)
    assert torch.equal(bits(got['xyzw'])[fixed], bits(init)[fixed])
    assert torch.isnan(got['resid'][fixed]).all() and torch.isfinite(got['resid'][~fixed]).all()
    assert torch.equal(bits(got['xyzw'][..., 3]), bits(init[..., 3]))
    assert np.array_equal(np.isnan(got['sym'].numpy()), np.repeat(~act[..., None], 2, -1))
    assert torch.isfinite(got['xyzw'][~fixed]).all() and torch.isfinite(got['cost']).all()
    for b in range(free.shape[0]):                                    # one status for the free joints of a sample
        assert len(set(st[b][free[b]])) <= 1
    f4 = lambda a: 4 * ulp32(a)
    resid, sym, cost = got['resid'].double().numpy(), got['sym'].double().numpy(), got['cost'].double().numpy()
    assert (np.abs(resid[..., 0] - o['resid'][..., 0])[free] <= (f4(o['resid'][..., 0]) + 1e-6)[free]).all(), name
    assert (np.abs(sym[..., 0] - o['sym'][..., 0])[act] <= f4(np.maximum(np.abs(o['sym'][..., 0]), 1e-3))[act]).all(), name
    assert (np.abs(cost[:, 0] - o['cost'][:, 0]) <= f4(o['cost'][:, 0])).all(), name
    cmp = compared(name) if name in CASES else (o['cond'] <= so.COND_MAX)
    if cmp.any():
        xyz = got['xyzw'][..., :3].double().numpy()
        with np.errstate(invalid='ignore'):
            err = np.abs(xyz - o['xyz']).max(-1)
        tol = 1e-4 + 2 * ulp32(np.abs(o['xyz']).max(-1))
        m = free & cmp[:, None]
        share = (err / tol)[m].max()
        e1 = np.abs(resid[..., 1] - o['resid'][..., 1]) / (f4(o['resid'][..., 1]) + 1e-6 + o['resid_shift'])
        ma = act & cmp[:, None]
        es = np.abs(sym[..., 1] - o['sym'][..., 1]) / (f4(np.maximum(np.abs(o['sym'][..., 1]), 1e-3)) + o['sym_shift'])
        ec = np.abs(cost[:, 1] - o['cost'][:, 1]) / (f4(o['cost'][:, 1]) + o['cost_shift'])
        text = '%d of %d samples compared, |xyz - oracle| %.3g mm = %.3g of its bound; resid %.3g, sym %.3g, cost %.3g of theirs; cond max %.3g; status %s' % (
            cmp.sum(), cmp.size, err[m].max(), share, e1[m].max(), es[ma].max() if ma.any() else 0.0, ec[cmp].max(),
            o['cond'][cmp].max(), np.bincount(st.ravel(), minlength=3).tolist())
        print(name + ': ' + text)
        if name in CASES:
            note(name, text)
        assert (err[m] <= tol[m]).all(), (name, share)
        assert (e1[m] <= 1).all() and (es[ma] <= 1).all() and (ec[cmp] <= 1).all(), (name, e1[m].max(), ec[cmp].max())
    check_cost(c, got, name=name)
    return c, o, got


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize('name', DECOUPLED)
def test_without_coupling_it_is_the_per_joint_refinement(name):
    c, o, got = check_vs_oracle(name)
    want = ro.refine(c['points'], c['P'], c['init'], c['views'], c['weighted'], c['huber'])
    assert not want['passed'].any() and (want['cond'] <= ro.COND_MAX).all()
    xyz = got['xyzw'][..., :3].double().numpy()
    err, tol = np.abs(xyz - want['xyz']).max(-1), 1e-4 + 2 * ulp32(np.abs(want['xyz']).max(-1))
    print('%s: |xyz - per-joint oracle| %.3g of the bound' % (name, (err / tol).max()))
    assert (err <= tol).all(), (err / tol).max()
    rtol = lambda a: 4 * ulp32(a) + 1e-6
    resid = got['resid'].double().numpy()
    assert (np.abs(resid[..., 0] - want['resid'][..., 0]) <= rtol(want['resid'][..., 0])).all()
    assert (np.abs(resid[..., 1] - want['resid'][..., 1]) <= rtol(want['resid'][..., 1]) + want['resid_shift']).all()
    if c['limbs']:                                                    # sym is still measured, it just does not pull
        assert torch.isfinite(got['sym']).all()
    else:
        assert got['sym'].shape == (2, 0, 2)


@pytest.mark.parametrize('name', COUPLED)
def test_coupled_minimum_is_the_oracles(name):
    c, o = case(name)
    if 'robust' in name:                                              # start and masks from the device's own robust solver
        from xas_amd import ops_eval
        r = ops_eval.triangulate_robust(torch.from_numpy(c['points']).cuda(), torch.from_numpy(c['P']).cuda(), threshold_px=THR)
        init, views = r['xyzw'].cpu().numpy(), r['inliers'].cpu().numpy()
        assert np.array_equal(views, c['robust']['mask'])
        c = dict(c, init=init, views=views)
        o = so.refine(c['points'], c['P'], init, **_kw(c))
        c, o, got = check_vs_oracle(name, got=run(c), o=o, c=c)
    else:
        c, o, got = check_vs_oracle(name)
    assert o['free'].all() and o['active'].all() and compared(name).mean() >= 0.9
    if 'clean' in name:
        assert (got['status'] == 0).all()
        assert np.abs(got['xyzw'][..., :3].numpy() - c['world']).max() < 1e-2         # the planted skeleton is the minimum
        assert got['sym'].abs().max() < 1e-2
    if 'noisy' in name and c['sym_w'] == 10.0:                        # the pull does something: limbs end more alike than they start
        assert (got['sym'][..., 1].abs().mean() < 0.5 * got['sym'][..., 0].abs().mean())


def test_fixed_joints_pass_through_and_switch_their_pairs_off():
    c, o, got = check_vs_oracle('fixed')
    for b, joints in FIXED_JOINTS.items():
        assert tuple(np.flatnonzero(~o['free'][b])) == joints
        assert tuple(np.flatnonzero(got['status'][b].numpy() == 2)) == joints
    # sample 0: joints 2, 6, 12, 15 touch all four pairs; sample 1 has no free joint at all; sample 2 is whole
    assert not o['active'][0].any() and not o['active'][1].any() and o['active'][2].all()
    assert torch.equal(bits(got['xyzw'][1]), bits(torch.from_numpy(c['init'][1]))) and (got['cost'][1] == 0).all()
    assert compared('fixed')[[0, 2]].all()
    used = [int(sum(1 << v for v in ro.views_used(c['points'][0, :, 7 + k], 0))) for k in range(5)]
    assert used == [0b111100, 0b111001, 0b110011, 0b100111, 0b001111]
    c, o, got = check_vs_oracle('behind')
    assert tuple(np.flatnonzero(~o['free'][0])) == (3, 16) and o['free'][1].all()
    assert o['active'].tolist() == [[False, True, False, True], [True] * 4]
    assert compared('behind').all()


def test_zero_length_limb_at_init_is_harmless():
    c, o, got = check_vs_oracle('flat')
    lb = np.linalg.norm(c['init'][0, 13, :3].astype(np.float64) - c['init'][0, 12, :3])
    assert abs(float(got['sym'][0, 0, 0]) + lb) <= ulp32(lb)                           # |a| = 0: the residual is -|b|
    assert torch.isfinite(got['xyzw']).all() and torch.isfinite(got['sym']).all() and (got['cost'][:, 1] <= got['cost'][:, 0]).all()


def test_unconverged_runs_only_lower_the_cost():
    c, o, got = check_vs_oracle('one_trial')
    assert (got['status'] == 1).all() and (got['cost'][:, 1] < got['cost'][:, 0]).all()
    c, o, got = check_vs_oracle('illcond')
    assert (o['cond'] > so.COND_MAX).all() and torch.isfinite(got['xyzw']).all()
    assert (got['cost'][:, 1] <= got['cost'][:, 0]).all()


def test_two_runs_and_missing_outputs_change_nothing():
    from xas_amd import _lib
    c, _ = case('w10_noisy_b3v6k24l16')
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pts, P, init = d(c['points']), d(c['P']), d(c['init'])
    B, V, K, _ = c['points'].shape
    L = len(c['limbs'])
    import ctypes
    table = (ctypes.c_int * (4 * L))(*[j for row in c['limbs'] for j in row])
    runs = []
    for fill in (float('nan'), 7.0):                                  # poisoned buffers: nothing is read before it is written
        out = dict(xyzw=torch.full((B, K, 4), fill).cuda(), resid=torch.full((B, K, 2), fill).cuda(), sym=torch.full((B, L, 2), fill).cuda(),
                   cost=torch.full((B, 2), fill).cuda(), status=torch.full((B, K), 9, dtype=torch.uint8).cuda())
        _lib.call('xas_triangulate_skeleton', _lib.ptr(pts), _lib.ptr(P), _lib.ptr(init), None, table, B, V, K, L, 0, 0.0, 10.0, 20,
                  *[_lib.ptr(out[k]) for k in ('xyzw', 'resid', 'sym', 'cost', 'status')])
        runs.append({k: v.cpu() for k, v in out.items()})
    for k in runs[0]:
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), k
    bare = run(c, want=())
    assert set(bare) == {'xyzw'} and torch.equal(bits(bare['xyzw']), bits(runs[0]['xyzw']))
    some = run(c, want=('sym',))
    assert set(some) == {'xyzw', 'sym'} and torch.equal(bits(some['sym']), bits(runs[0]['sym']))


def test_refusals_name_the_limit():
    from xas_amd import ops_eval
    t = lambda *s: torch.ones(*s).cuda()
    args = lambda V=3, K=4: (t(1, V, K, 3), t(1, V, 3, 4), t(1, K, 4))
    with pytest.raises(RuntimeError, match=r'K=25 joints \(needs 3 <= K <= XAS_SKEL_MAX_JOINTS = 24\)'):
        ops_eval.triangulate_skeleton(*args(K=25), limbs=())
    with pytest.raises(RuntimeError, match=r'V=7 views'):
        ops_eval.triangulate_skeleton(*args(V=7), limbs=())
    with pytest.raises(RuntimeError, match=r'limbs\[0\]\[3\] = 4 is no joint'):
        ops_eval.triangulate_skeleton(*args(), limbs=((1, 0, 3, 4),))
    with pytest.raises(RuntimeError, match=r'sym_w'):
        ops_eval.triangulate_skeleton(*args(), limbs=(), sym_w=-1.0)
    with pytest.raises(RuntimeError, match='every limb pair is'):
        ops_eval.triangulate_skeleton(*args(), limbs=((1, 0, 3),))


# ------------------------------------------------------------------------------------------------ Eval
def _eval_setup():
    from test_gpu_tri_robust import PlantedDetector, eval_case
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
    from test_gpu_tri_robust import _cfg
    cfg = _cfg(cams)
    cfg['model_params'].update(keys)
    return cfg


@pytest.mark.parametrize('tri', ['dlt', 'robust'])
def test_eval_batch_couples_only_when_asked(tmp_path, tri):
    import eval as xeval
    from modules import util as mu
    from xas_amd import ops_eval
    cams, xd, det = _eval_setup()
    mk = lambda **keys: xeval.Eval(_cfg_with(cams, **keys), det, [], str(tmp_path), tri=tri)
    today, lm = mk().eval_batch(xd, 'best'), mk(tri_refine='lm').eval_batch(xd, 'best')
    sk = mk(tri_refine='skeleton', tri_sym=10.0).eval_batch(xd, 'best')
    assert set(sk) == set(lm) | {'tri_sym_mm'} == set(today) | {'tri_refine_px', 'tri_refine_gain_px', 'tri_sym_mm'}
    assert sk['tri_sym_mm'].shape == (2,) and sk['tri_sym_mm'].is_cuda and torch.isfinite(sk['tri_sym_mm']).all()
    assert float(sk['tri_refine_px']) >= 0
    sel = {'cam_%d' % c: ops_eval.eval_select(det.kps[i], xd['cam_%d_joints' % c], mode='best')['sel3d'] for i, c in enumerate(cams)}
    px = THR if tri == 'robust' else None
    direct, r = mu.triangulation_skeleton(sel, xd, cams, robust_px=px, sym_w=10.0, want=('sym',))
    assert torch.equal(sk['world_tri'], direct) and not torch.equal(sk['world_tri'], lm['world_tri'])
    assert torch.equal(sk['tri_sym_mm'], r['sym'].abs().reshape(-1, 2).nanmean(dim=0))
    # lm is what it was: the per-joint call, bit for bit
    direct_lm, _ = mu.triangulation_refined(sel, xd, cams, robust_px=px)
    assert torch.equal(bits(lm['world_tri']), bits(direct_lm))
    for k in today:                                                   # nothing but the triangulated pose moves
        if 'tri' not in k:
            assert torch.equal(sk[k], today[k]), k
    assert mk(tri_refine='skeleton').tri_sym == ops_eval.TRI_SYM_W == 0.1


def test_result_file_gains_one_line_with_skeleton_only(tmp_path):
    import eval as xeval
    cams, xd, det = _eval_setup()
    texts = {}
    for tag, keys in (('today', {}), ('lm', dict(tri_refine='lm')), ('skeleton', dict(tri_refine='skeleton', tri_sym=2.0))):
        e = xeval.Eval(_cfg_with(cams, **keys), det, [dict(xd), dict(xd)], str(tmp_path / tag))
        lines = e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt').read().strip().split('\n')
    assert len(texts['lm']) == len(texts['today']) + 1 and texts['lm'][-1].startswith('TRI refine lm (huber 0.0): ')
    assert not any('skeleton' in l for l in texts['lm'])
    new = texts['skeleton']
    tri = texts['today'].index('---Tri3D-----')                       # only the triangulated pose's own figures move
    assert len(new) == len(texts['today']) + 1 and new[:tri + 1] == texts['today'][:tri + 1] == texts['lm'][:tri + 1]
    assert new[-1].startswith('TRI refine skeleton (huber 0.0, sym 2.0): reprojection RMS ')
    assert ' px, gained ' in new[-1] and ' px, limb asymmetry ' in new[-1] and new[-1].endswith(' mm')
    with pytest.raises(ValueError, match="tri_refine='skeleton' refines over at most 6 cameras; cam_id_list has 7"):
        xeval.Eval(_cfg_with(list(range(7)), tri_refine='skeleton'), det, [], str(tmp_path))
    det.num_kp = 25
    with pytest.raises(ValueError, match="tri_refine='skeleton' couples at most 24 joints; the detector has 25"):
        xeval.Eval(_cfg_with(cams, tri_refine='skeleton'), det, [], str(tmp_path))
