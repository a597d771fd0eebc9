"""xas_calibrate_linearise / xas_calibrate_bundle on the device against the float64 oracle (tests/_calib_oracle.py) on the
decidable cases of tests/_calib_inputs.py (test_calib_abi checks on the CPU that they are).
Tolerances.  tol = max(16 x the distance the oracle shows between its own two formulations on that case, 64 ulps of double),
relative to the scale of the quantity: the largest |entry| of S (of b); 1 rad for omega; the largest |coordinate| of the points
for tau and the points.  The margin covers another order of summation and FMA contraction.  `out` is fp32: two doubles that close
may round to neighbouring floats, so one fp32 ulp of the value is added there."""
import numpy as np
import pytest
import torch

import _calib_inputs as ci
import _calib_oracle as co
from test_calib_abi import CASE_LIST, formulation_distance

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
DEV = 'cuda'


def dev(case):
    t = lambda a, dt=None: None if a is None else torch.as_tensor(a, dtype=dt).to(DEV)
    return dict(points=t(case['points']), pmat=t(case['P']), init=t(case['init']), rig=t(case['rig'], torch.int64),
                views=t(case['views']))


def kwargs(case, **over):
    k = dict(free=case['free_mask'], weighted=case['weighted'], huber_px=case['huber'], prior_rot=case['prior_rot'],
             prior_trans=case['prior_trans'], num_rigs=case['R'])
    k.update(over)
    return k


_oracle = {}


def oracle(name, variant):
    """Computed once per case and shared: the case, both schedules' results per rig, and their distance."""
    key = (name, variant)
    if key not in _oracle:
        c = ci.planted() if name == 'planted' else ci.make(name, variant)
        rigs = [co.make_rig(c, r) for r in range(c['R'])]
        a = [g.lm(g.step_dense, c['max_iter']) for g in rigs]
        b = [g.lm(g.step_schur, c['max_iter']) for g in rigs]
        _oracle[key] = (c, rigs, a, b)
    return _oracle[key]


@pytest.mark.parametrize('name,variant', CASE_LIST)
def test_linearise_matches_the_oracle(name, variant):
    from xas_amd import ops_calib
    c, rigs, _, _ = oracle(name, variant)
    d = dev(c)
    for lam in (0.0, 1e-3):
        got = ops_calib.calibrate_linearise(lam=lam, **d, **kwargs(c))
        for r, g in enumerate(rigs):
            S1, b1 = g.schur_of_dense(g.delta0, g.X0, lam)
            S2, b2, _ = g.schur_system(g.delta0, g.X0, lam)
            C, _, _ = g.cost(g.delta0, g.X0)
            S, b = got['S'][r].cpu(), got['b'][r].cpu()
            sS, sb = float(S2.abs().max()), float(b2.abs().max())
            tS = max(16 * float((S1 - S2).abs().max()) / sS, 64 * EPS)
            tb = max(16 * float((b1 - b2).abs().max()) / sb, 64 * EPS)
            rS, rb = float((S - S2).abs().max()) / sS, float((b - b2).abs().max()) / sb
            print('linearise %s %s rig %d lambda %g: S %.2e (bound %.2e)  b %.2e (bound %.2e)' % (name, variant, r, lam, rS, tS, rb, tb))
            assert rS <= tS and rb <= tb
            assert abs(float(got['C'][r]) - C) <= 64 * EPS * abs(C)
            assert torch.equal(S, S.T)


def _compare(c, rigs, a, b, got):
    order = np.argsort(c['rig'], kind='stable')
    out = got['xyzw'].cpu().numpy()
    for r, g in enumerate(rigs):
        m = c['rig'] == r
        tol = max(16 * formulation_distance(a[r], b[r]), 64 * EPS)
        scale = max(1.0, float(np.abs(b[r]['X']).max())) if g.M else 1.0
        delta = got['delta'][r].cpu().numpy()
        assert int(got['status'][r]) == b[r]['status']
        assert got['trials'][r].tolist() == [b[r]['trials'], b[r]['accepted']]
        dw, dt = np.abs(delta[:, :3] - b[r]['delta'][:, :3]).max(), np.abs(delta[:, 3:] - b[r]['delta'][:, 3:]).max()
        o, ref = out[m], b[r]['out']
        fixed = ~g.free
        assert np.array_equal(o[fixed].view(np.uint32), c['init'][m][fixed].view(np.uint32))          # bit for bit, NaN included
        assert np.array_equal(o[..., 3].view(np.uint32), c['init'][m][..., 3].view(np.uint32))
        dx = np.abs(o[g.free][:, :3].astype(np.float64) - b[r]['X'])
        ulp = np.spacing(np.abs(ref[g.free][:, :3])).astype(np.float64)
        print('bundle %s rig %d: omega %.2e tau %.2e out %.2e (tol %.2e, scale %.0f)' % (
            c['name'], r, dw, dt / scale, float((dx / scale).max()) if g.M else 0.0, tol, scale))
        assert dw <= tol and dt <= tol * scale
        assert (dx <= tol * scale + ulp).all()
        for v in range(c['V']):
            if v not in g.slot:
                assert (delta[v] == 0).all()
        cost = got['cost'][r].tolist()
        assert cost[1] <= cost[0]
        assert abs(cost[0] - b[r]['cost'][0]) <= 1e-12 * abs(cost[0]) and abs(cost[1] - b[r]['cost'][1]) <= 1e-9 * abs(cost[1])
        if g.M:
            assert np.allclose(got['rms'][r].tolist(), b[r]['rms'], rtol=1e-9)
    return order


@pytest.mark.parametrize('name,variant', CASE_LIST)
def test_bundle_matches_the_oracle(name, variant):
    from xas_amd import ops_calib
    c, rigs, a, b = oracle(name, variant)
    d = dev(c)
    got = ops_calib.calibrate_bundle(max_iter=c['max_iter'], **d, **kwargs(c))
    _compare(c, rigs, a, b, got)
    again = ops_calib.calibrate_bundle(max_iter=c['max_iter'], **d, **kwargs(c))
    for k in got:                                                       # the same bits in every output
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), k
    few = ops_calib.calibrate_bundle(max_iter=c['max_iter'], want=(), **d, **kwargs(c))
    assert set(few) == {'delta', 'xyzw'}                                # optional outputs as NULL change nothing in the others
    for k in few:
        assert torch.equal(got[k].view(torch.uint8), few[k].view(torch.uint8)), k
    cov = got['cam_cov']
    V = c['V']
    for r, g in enumerate(rigs):
        for v in range(V):
            if v not in g.slot:
                assert (cov[r, 6 * v:6 * v + 6] == 0).all() and (cov[r, :, 6 * v:6 * v + 6] == 0).all()
        if g.M and g.nc:
            S, _, _ = g.schur_system(torch.as_tensor(b[r]['delta']), torch.as_tensor(b[r]['X']), 0.0)
            rows = [6 * v + i for v in g.free_cams for i in range(6)]
            sub = cov[r].cpu()[rows][:, rows]
            resid = (sub @ S - torch.eye(len(rows), dtype=torch.float64)).abs().max()
            cond = float(torch.linalg.cond(S))
            print('cam_cov %s rig %d: |cov S - I| %.2e cond %.2e' % (name, r, float(resid), cond))
            assert float(resid) <= 64 * EPS * cond * len(rows)          # an inverse carries the condition number


def gpu_decisions(d, kw, max_iter):
    """What the device decided, trial by trial and per rig, read off the trials output of calls with 1, 2, .. max_iter trials
    (a call is a pure function of its inputs, so each is a prefix of the next)."""
    from xas_amd import ops_calib
    R = kw['num_rigs']
    dec, last = [[] for _ in range(R)], [0] * R
    for m in range(1, max_iter + 1):
        t = ops_calib.calibrate_bundle(max_iter=m, want=('trials',), **d, **kw)['trials'].tolist()
        for r in range(R):
            if t[r][0] == m:
                dec[r].append(t[r][1] > last[r])
                last[r] = t[r][1]
    return dec


def test_long_schedules_follow_the_oracle_through_ties():
    """30 trials on cameras bumped by 3 degrees and 100 mm, six seeds, plain and Huber: the rigs converge after a handful of
    trials, and from there every trial changes the cost by less than TIE_MARGIN of itself, where no two orders of summation need
    agree.  The oracle is made to take the device's decision at those trials (and must agree by itself at every other), and
    status, trial counts, delta and out are compared as in the short cases.  Between them the rigs must contain the step-rule
    stop, rejected trials and the stop at lambda > 1e12."""
    from xas_amd import ops_calib
    seen = set()
    for seed in range(1, 7):
        for variant in ('plain', 'huber'):
            c = ci.make('typical', variant, seed=seed, deg=3.0, mm=100.0)
            c['max_iter'] = 30
            d, kw = dev(c), kwargs(c)
            dec = gpu_decisions(d, kw, c['max_iter'])
            rigs = [co.make_rig(c, r) for r in range(c['R'])]
            pairs = [co.follow(g, dec[r], c['max_iter']) for r, g in enumerate(rigs)]
            got = ops_calib.calibrate_bundle(max_iter=c['max_iter'], **d, **kw)
            print('followed seed %d %s: decisions %s, status %s, trials %s' % (
                seed, variant, [''.join('AR'[not x] for x in q) for q in dec], got['status'].tolist(), got['trials'].tolist()))
            _compare(c, rigs, [p[0] for p in pairs], [p[1] for p in pairs], got)
            seen |= {'rejected' for q in dec if not all(q)} | {'status %d' % v for v in got['status'].tolist()}
            seen |= {'lambda stop' for t, v in zip(got['trials'].tolist(), got['status'].tolist()) if v == 1 and t[0] < 30}
    print('followed schedules saw:', sorted(seen))
    assert {'rejected', 'status 0', 'lambda stop'} <= seen


def test_nonzero_start_and_camera_0_free():
    from xas_amd import ops_calib
    c = ci.make('typical')
    rng = np.random.default_rng(5)
    c['delta0'] = rng.normal(size=(c['R'], c['V'], 6)) * np.array([2e-3] * 3 + [3.0] * 3)
    c['free_mask'] = 0b011                                              # camera 0 free, camera 2 fixed
    rigs = [co.make_rig(c, r) for r in range(c['R'])]
    a = [g.lm(g.step_dense, c['max_iter']) for g in rigs]
    b = [g.lm(g.step_schur, c['max_iter']) for g in rigs]
    assert all(x['decisions'] == y['decisions'] and min(y['margins']) > 1e-9 for x, y in zip(a, b))
    got = ops_calib.calibrate_bundle(max_iter=c['max_iter'], delta=torch.as_tensor(c['delta0']), **dev(c), **kwargs(c))
    _compare(c, rigs, a, b, got)


def test_no_free_camera_is_the_per_point_refinement():
    """free_mask = 0: the points alone are solved, under one lambda and one stop per rig.  Both solvers run until their steps
    are under 1e-5 mm (or their trials out, which is later); Gauss-Newton steps that small leave each within 1e-5 mm of the
    minimum, so the two are within 2e-5 mm plus the rounding of `out` to fp32 (one ulp of the value)."""
    from xas_amd import ops_calib, ops_eval
    c, _, _, _ = oracle('widest', 'plain')
    d = dev(c)
    got = ops_calib.calibrate_bundle(max_iter=64, **d, **kwargs(c, free=0))
    ref = ops_eval.triangulate_refine(d['points'], d['pmat'], d['init'], views=d['views'], max_iter=64, want=('status',))
    assert (got['delta'] == 0).all() and (got['status'] != 2).all() and (got['cam_cov'] == 0).all()
    fixed = ref['status'] == 2
    assert int(fixed.sum()) >= 3 and torch.equal(got['xyzw'][fixed].view(torch.int32), d['init'][fixed].view(torch.int32))
    a, b = got['xyzw'][~fixed][:, :3].double(), ref['xyzw'][~fixed][:, :3].double()
    ulp = torch.as_tensor(np.spacing(b.abs().float().cpu().numpy())).to(DEV).double()
    print('free_mask 0 against triangulate_refine: largest distance %.3e mm' % float((a - b).abs().max()))
    assert ((a - b).abs() <= 2e-5 + ulp).all()
    assert (got['cost'][:, 1] <= got['cost'][:, 0]).all()


def test_rigs_are_independent_bit_for_bit():
    from xas_amd import ops_calib
    c, _, _, _ = oracle('widest', 'plain')
    d = dev(c)
    whole = ops_calib.calibrate_bundle(max_iter=3, **d, **kwargs(c))
    for r in range(c['R']):
        m = d['rig'] == r
        sub = {k: (None if v is None else v[m]) for k, v in d.items()}
        sub['rig'] = torch.zeros(int(m.sum()), dtype=torch.int64, device=DEV)
        alone = ops_calib.calibrate_bundle(max_iter=3, **sub, **kwargs(c, num_rigs=1))
        spread = dict(sub, rig=sub['rig'] + 1)                          # the same samples as rig 1 of 3, rigs 0 and 2 empty
        padded = ops_calib.calibrate_bundle(max_iter=3, **spread, **kwargs(c, num_rigs=3))
        for k in ('delta', 'cost', 'rms', 'cam_cov', 'status', 'trials'):
            assert torch.equal(whole[k][r].view(torch.uint8), alone[k][0].view(torch.uint8)), k
            assert torch.equal(padded[k][1].view(torch.uint8), alone[k][0].view(torch.uint8)), k
        assert torch.equal(whole['xyzw'][m].view(torch.int32), alone['xyzw'].view(torch.int32))
        assert torch.equal(padded['xyzw'].view(torch.int32), alone['xyzw'].view(torch.int32))
        assert (padded['status'][[0, 2]].cpu() == 2).all()


def test_planted_cameras_are_recovered():
    from xas_amd import ops_calib
    c, rigs, _, b = oracle('planted', 'plain')
    got = ops_calib.calibrate_bundle(max_iter=c['max_iter'], **dev(c), **kwargs(c))
    out = got['xyzw'].cpu().numpy()
    for r, g in enumerate(rigs):
        rms = got['rms'][r].tolist()
        print('planted rig %d: rms %.3e -> %.3e px (oracle %.3e -> %.3e), status %d' % (
            r, rms[0], rms[1], b[r]['rms'][0], b[r]['rms'][1], int(got['status'][r])))
        assert int(got['status'][r]) == b[r]['status'] == 0              # the step rule stopped it, as it stopped the oracle
        assert rms[1] <= 16 * max(b[r]['rms'][1], 1e-4)                 # 1e-4 px: what fp32 detections of ~1e3 px resolve
        m = c['rig'] == r
        truth = c['truth'][m][g.free]
        aligned = co.similarity_align(out[m][g.free][:, :3].astype(np.float64), truth)
        assert np.abs(aligned - truth).max() < 0.05


def test_sentinels_round_every_output_stay_intact():
    import ctypes
    from xas_amd._lib import call, ptr, query
    c, _, _, _ = oracle('typical', 'plain')
    order = np.argsort(c['rig'], kind='stable')
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a[order])).to(DEV)
    N, V, K, R = c['N'], c['V'], c['K'], c['R']
    start = np.concatenate([[0], np.cumsum(np.bincount(c['rig'], minlength=R))]).astype(int)
    table = (ctypes.c_int * (R + 1))(*start.tolist())
    pad = 64

    def guarded(n, dtype, fill):
        buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
        return buf, buf[pad:pad + n]
    bufs = {'delta': guarded(R * V * 6, torch.float64, 0.0), 'out': guarded(N * K * 4, torch.float32, -7.0),
            'cost': guarded(R * 2, torch.float64, -7.0), 'rms': guarded(R * 2, torch.float64, -7.0),
            'cam_cov': guarded(R * 36 * V * V, torch.float64, -7.0), 'status': guarded(R, torch.uint8, 77),
            'trials': guarded(R * 2, torch.int32, -7)}
    nbytes = query('xas_calibrate_workspace_bytes', N, V, K, R)
    ws_buf =torch.full((nbytes + 2 * pad + 16,), 99, dtype=torch.uint8, device=DEV)
    off = (-ws_buf.data_ptr() - pad) % 16 + pad
    ws = ws_buf[off:off + nbytes]
    pts, P, init, views = t(c['points']), t(c['P']), t(c['init']), t(c['views'])
    call('xas_calibrate_bundle', ptr(pts), ptr(P), ptr(init), ptr(views), table, N, V, K, R, c['free_mask'], 0, 0.0,
         c['prior_rot'], c['prior_trans'], 3, *(ptr(bufs[k][1]) for k in ('delta', 'out', 'cost', 'rms', 'cam_cov', 'status', 'trials')),
         ptr(ws))
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        fill = {'delta': 0.0, 'status': 77}.get(k, -7)
        assert (buf[:pad] == fill).all() and (buf[pad + view.numel():] == fill).all(), k
    assert (ws_buf[:off] == 99).all() and (ws_buf[off + nbytes:] == 99).all()
    assert (bufs['status'][1] == 1).all() and (bufs['out'][1] != -7.0).all()
