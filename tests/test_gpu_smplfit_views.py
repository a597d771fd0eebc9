"""xas_smpl_fit_views / xas_smpl_fit_views_linearise on the GPU against tests/_smplfit_views_oracle.py (float64 torch) on the
cases of tests/_smplfit_views_cases.py.

Bounds.  Both sides are double arithmetic on the same fp32 inputs and differ by rounding and by the order of their sums.  The
oracle forms every quantity twice (stacked rows with an autograd Jacobian; joint blocks by hand); the distance of its two answers
is its own SPREAD.  A device-to-oracle distance, relative to the largest |entry|, is held to test_gpu_smplfit_tracks.bound:
16 x that spread with a floor of 64 ulps of double.  A run of this file with -s prints every figure;
profiles/smpl_fit_views_check.txt keeps them."""
import numpy as np
import pytest
import torch

import _smplfit_views_cases as vc
import _smplfit_views_oracle as vo
from test_gpu_smplfit_tracks import bound, join, split

pytestmark = pytest.mark.gpu

_cache = {}


def layer_of(V, reg='dense', center=0):
    key = (V, reg, center)
    if key not in _cache:
        from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer
        a, _ = vc.model(V, reg)
        _cache[key] = (SMPL_Layer.from_arrays(a, center_idx=None if center < 0 else center).cuda(), torch.as_tensor(a['h36m_regressor']).cuda())
    return _cache[key]


def device(c, fn='fit', rows=None, **kw):
    """The case (or its rows) through ops_smplfit on the GPU -> the op's dict on the CPU."""
    from xas_amd import ops_smplfit
    layer, hreg = layer_of(c['V'], c['reg'], c['center'])
    rows = np.arange(len(c['x0'])) if rows is None else np.asarray(rows)
    g = lambda k: None if c[k] is None else torch.as_tensor(c[k][rows]).cuda()
    op = ops_smplfit.fit_smpl_views if fn == 'fit' else ops_smplfit.linearise_smpl_views
    out = op(g('points'), g('P'), layer, hreg, split(c['x0'][rows]), views=g('views'), anchor=g('anchor'), info=g('info'),
             weighted=c['weighted'], huber=c['huber'], anchor_huber=c['anchor_huber'], pose_prior=vc.WP, shape_prior=vc.WS, **kw)
    return {k: v.cpu() for k, v in out.items()}


def fit_of(name):
    if ('fit', name) not in _cache:
        _cache[('fit', name)] = device(vc.build(name), iters=vc.FIT_ITERS)
    return _cache[('fit', name)]


@pytest.mark.parametrize('name', sorted(vc.CASES))
def test_linearise_against_the_oracle(name):
    c = vc.build(name)
    out = device(c, 'lin')
    for b, s in enumerate(vc.oracle_samples(name)):
        assert out['used'][b].tolist() == s.used.tolist()
        if not torch.isfinite(s.x0).all():
            continue                                                                 # a start that is not finite: NaN, nothing to compare
        H, g = s.normal_rows(s.x0)
        Hb, gb = s.normal_blocks(s.x0)
        C, _ = s.cost(s.x0)
        Cb = float(s.blocks(s.x0)[2].sum()) + float((s.wp * s.x0[6:75] ** 2).sum() + (s.ws * s.x0[75:] ** 2).sum())
        jb, jb2 = s.joint_blocks(s.x0), s.blocks_autograd(s.x0)
        sH, sg, sC, sj = vo.rel(Hb, H), vo.rel(gb, g), abs(Cb - C) / C, vo.rel(jb2, jb)
        dH, dg, dC, dj = vo.rel(out['H'][b], H), vo.rel(out['g'][b], g), abs(float(out['cost'][b]) - C) / C, vo.rel(out['joint_blocks'][b], jb)
        print('views linearise %s sample %d: H %.2e (spread %.2e, bound %.2e)  g %.2e (spread %.2e, bound %.2e)  C %.2e (spread %.2e, bound %.2e)  '
              'joint blocks %.2e (spread %.2e, bound %.2e)' % (name, b, dH, sH, bound(sH), dg, sg, bound(sg), dC, sC, bound(sC), dj, sj, bound(sj)))
        assert dH <= bound(sH) and dg <= bound(sg) and dC <= bound(sC) and dj <= bound(sj)
        assert torch.equal(out['H'][b], out['H'][b].T) and torch.isfinite(out['H'][b]).all()
        assert not out['joint_blocks'][b][torch.as_tensor(s.used == 0)].any()        # a joint not used: zeros


@pytest.mark.parametrize('name', sorted(vc.CASES))
def test_fit_follows_the_oracles_lm(name):
    c, out = vc.build(name), fit_of(name)
    x = join(out)
    for b, s in enumerate(vc.oracle_samples(name)):
        assert out['used'][b].tolist() == s.used.tolist()
        if s.passed():
            assert int(out['status'][b]) == 2 and int(out['iters'][b]) == 0
            continue
        r = s.lm(vc.FIT_ITERS)
        assert r['margin'] >= 1e-9                                                   # comparable decisions
        assert int(out['status'][b]) == r['status'] == 1 and int(out['iters'][b]) == r['iters']
        gx = vo.rel(x[b], r['x'])
        gc = abs(float(out['cost'][b, 1]) - r['cost'][1]) / r['cost'][1]
        print('views fit %s sample %d: %d trials (accepted %s), cost %.3f -> %.6f (oracle %.6f, gap %.2e), parameters %.2e (oracle spread %.2e, '
              'bound %.2e)' % (name, b, r['iters'], ''.join('y' if a else 'n' for a in r['accepts']), float(out['cost'][b, 0]),
                               float(out['cost'][b, 1]), r['cost'][1], gc, gx, r['spread'], bound(r['spread'])))
        assert gx <= bound(r['spread']) and gc <= bound(r['spread'])
        assert float(out['cost'][b, 1]) <= float(out['cost'][b, 0])
        assert vo.rel(out['joints'][b], s.joints(r['x']).detach()) <= bound(r['spread'])


def test_pass_through_is_the_init_bit_for_bit():
    c, out = vc.build('passed_V70'), fit_of('passed_V70')
    x0 = torch.as_tensor(c['x0']).float().double()
    assert out['status'].tolist() == [2, 2, 1] and out['iters'].tolist()[:2] == [0, 0]
    assert torch.equal(join(out)[0], x0[0])
    assert torch.equal(join(out)[1].nan_to_num(nan=7.0), x0[1].nan_to_num(nan=7.0))  # NaN stays NaN, the rest its bits
    assert torch.equal(out['cost'][0, 0], out['cost'][0, 1]) and torch.isfinite(out['cost'][0]).all()
    assert not torch.isfinite(out['cost'][1]).any()
    zero = device(c, iters=0)
    assert zero['status'].tolist() == [2, 2, 1] and zero['iters'].tolist() == [0, 0, 0]
    assert torch.equal(join(zero)[2], x0[2]) and torch.equal(zero['cost'][2, 0], zero['cost'][2, 1])
    # nothing to do
    from xas_amd import ops_smplfit
    layer, hreg = layer_of(70)
    e = lambda *s: torch.zeros(*s, device='cuda')
    none = ops_smplfit.fit_smpl_views(e(0, 2, 18, 3), e(0, 2, 3, 4), layer, hreg, {'pose': e(0, 72), 'betas': e(0, 10), 'trans': e(0, 3)})
    assert none['pose'].shape == (0, 72) and none['used'].shape == (0, 18)


def test_runs_are_bit_identical_and_samples_independent():
    from xas_amd import ops_smplfit
    for name in ('one_camera_ray_V70', 'four_cameras_full_V513'):
        c = vc.build(name)
        B = len(c['x0'])
        nbytes = ops_smplfit.views_workspace_bytes(B, c['V'])
        runs = [fit_of(name)]
        for fill in (0xFF, 0x55):
            runs.append(device(c, iters=vc.FIT_ITERS, workspace=torch.full((nbytes,), fill, dtype=torch.uint8, device='cuda')))
        lins = [device(c, 'lin', workspace=torch.full((nbytes,), fill, dtype=torch.uint8, device='cuda')) for fill in (0xFF, 0x55)]
        for r in runs[1:]:
            for key in runs[0]:
                assert torch.equal(r[key], runs[0][key]), key
        for key in lins[0]:
            assert torch.equal(lins[1][key], lins[0][key]), key
        alone = device(c, rows=[B - 1], iters=vc.FIT_ITERS)                          # the last sample without the others
        swapped = device(c, rows=np.arange(B)[::-1].copy(), iters=vc.FIT_ITERS)
        for key in runs[0]:
            assert torch.equal(alone[key][0], runs[0][key][B - 1]), key
            assert torch.equal(swapped[key], runs[0][key].flip(0)), key


def test_cost_never_rises():
    for name in sorted(vc.CASES):
        out = fit_of(name)
        fin = torch.isfinite(out['cost'][:, 0])
        assert (out['cost'][fin, 1] <= out['cost'][fin, 0]).all(), name
    long = device(vc.build('six_cameras_behind_V70'), iters=30)
    assert (long['cost'][:, 1] <= long['cost'][:, 0]).all() and (long['cost'][:, 1] <= fit_of('six_cameras_behind_V70')['cost'][:, 1]).all()


def test_where_the_problems_coincide():
    """No valid view, anchors = targets, info = w_k I, anchor_huber = 0: xas_smpl_fit's problem on those targets and weights."""
    from xas_amd import ops_smplfit
    import _smplfit_tracks_cases as tc
    t = tc.build('mixed_V70', extras=True)                                          # joint 3 has weight 0 and a NaN target
    rows = np.nonzero((t['w'] > 0).sum(1) >= 6)[0][:3]
    tgt, w, x0 = t['tgt'][rows], t['w'][rows] * np.linspace(0.5, 2.0, 18, dtype=np.float32), t['x0'][rows]
    layer, hreg = layer_of(70)
    B = len(rows)
    info = np.zeros((B, 18, 6), np.float32)
    info[..., 0] = info[..., 3] = info[..., 5] = w
    points = np.zeros((B, 1, 18, 3), np.float32)
    P = np.tile(vc.look_at(np.array([0.0, 0.0, -4000.0]), np.zeros(3)).astype(np.float32), (B, 1, 1, 1))
    cuda = lambda a: torch.as_tensor(a).cuda()
    kw = dict(pose_prior=tc.WP, shape_prior=tc.WS)
    lin = ops_smplfit.linearise_smpl_views(cuda(points), cuda(P), layer, hreg, split(x0), anchor=cuda(tgt), info=cuda(info), anchor_huber=0.0, **kw)
    r, J = ops_smplfit.linearise_smpl(cuda(tgt), cuda(w), layer, hreg, split(x0), **kw)
    H, g, C = (J.transpose(1, 2) @ J).cpu(), (J.transpose(1, 2) @ r.unsqueeze(-1))[..., 0].cpu(), (r * r).sum(1).cpu()
    m = vc.model(70)[1]
    spreads = []
    for b in range(B):
        s = vo.Sample(m, x0[b], points[b], P[b], None, tgt[b], info[b], False, 0.0, 0.0, tc.WP, tc.WS, 0)
        assert s.used.tolist() == lin['used'][b].tolist() == [0x80 if w[b, k] > 0 else 0 for k in range(18)]
        Ha, ga = s.normal_rows(s.x0)
        Hb, gb = s.normal_blocks(s.x0)
        spreads.append((vo.rel(Hb, Ha), vo.rel(gb, ga)))
        dH, dg, dC = vo.rel(lin['H'][b].cpu(), H[b]), vo.rel(lin['g'][b].cpu(), g[b]), abs(float(lin['cost'][b]) - float(C[b])) / float(C[b])
        print('views = joints, sample %d: H %.2e (bound %.2e)  g %.2e (bound %.2e)  C %.2e' % (b, dH, bound(spreads[-1][0]), dg, bound(spreads[-1][1]), dC))
        assert dH <= bound(spreads[-1][0]) and dg <= bound(spreads[-1][1]) and dC <= bound(0.0)
    a = ops_smplfit.fit_smpl_views(cuda(points), cuda(P), layer, hreg, split(x0), anchor=cuda(tgt), info=cuda(info), anchor_huber=0.0,
                                   iters=vc.FIT_ITERS, **kw)
    o = ops_smplfit.fit_smpl(cuda(tgt), cuda(w), layer, hreg, init=split(x0), iters=vc.FIT_ITERS, **kw)
    a, o = {k: v.cpu() for k, v in a.items()}, {k: v.cpu() for k, v in o.items()}
    assert torch.equal(a['iters'], o['iters']) and torch.equal(a['status'], o['status'])
    for b in range(B):
        s = vo.Sample(m, x0[b], points[b], P[b], None, tgt[b], info[b], False, 0.0, 0.0, tc.WP, tc.WS, 0)
        spread = s.lm(vc.FIT_ITERS)['spread']
        gap = vo.rel(join(a)[b], join(o)[b])
        print('views = joints, sample %d after %d trials: parameters %.2e (oracle spread %.2e, bound %.2e)' % (b, vc.FIT_ITERS, gap, spread, bound(spread)))
        assert gap <= bound(spread)


@pytest.mark.parametrize('ncam', (1, 4))
def test_eval_writes_the_pixel_fit(tmp_path, ncam):
    """eval.py's Eval through the synthetic loader of tests/test_eval_fit_cli.py with fit_data reproj, one camera and four."""
    import eval as xeval
    from test_eval_fit_cli import _cfg, _setup
    cams, xd, det, model, smpl = _setup(tmp_path)
    cams = cams[:ncam]
    banks, texts = {}, {}
    for tag, keys in (('joints', {}), ('reproj', dict(fit_data='reproj'))):
        banks[tag] = str(tmp_path / tag / 'bank.npz')
        e = xeval.Eval(_cfg(cams, fit_smpl=banks[tag], smpl_model=model, fit_iters=8, **keys), det, [dict(xd)], str(tmp_path / tag))
        e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt').read().strip().split('\n')
        with np.load(banks[tag]) as z:
            banks[tag] = {k: z[k] for k in z.files}
    old, new = banks['joints'], banks['reproj']
    B = xd['cam_0_joints'].shape[0]
    assert sorted(new) == sorted(list(old) + ['fit_data', 'reproj_rms_px', 'pose_joints', 'betas_joints', 'trans_joints'])
    assert str(new['fit_data']) == 'reproj' and new['reproj_rms_px'].shape == (B, 2) and new['pose'].shape == (B, 72)
    for k in ('pose', 'betas', 'trans'):
        assert np.array_equal(new[k + '_joints'], old[k])                          # the warm start is the joint fit
    fitted = new['status'] != 2
    assert fitted.any() and (new['reproj_rms_px'][fitted, 1] <= new['reproj_rms_px'][fitted, 0]).all()
    assert (new['cost'][fitted, 1] <= new['cost'][fitted, 0]).all()
    assert texts['reproj'][:-1] == texts['joints'][:-1] and texts['reproj'][-1].startswith('FIT smpl reproj (8 trials')
    assert 'reprojection RMS ' in texts['reproj'][-1] and ' px' in texts['reproj'][-1]
    print('eval --fit-data reproj, %d camera(s): %s' % (ncam, texts['reproj'][-1]))


def test_eval_hands_over_inliers_and_fused_anchors(tmp_path, monkeypatch):
    """--tri robust and --tri-volume with --fit-data reproj, on the planted four-camera batch and detector of
    tests/test_gpu_eval_all_options.py: the inlier bytes arrive as `views`, the fused points as anchors with the inverse of their
    covariance (NaN where the volume passed a joint through), and the file is written as in the plain runs."""
    import eval as xeval
    import _smplfit_inputs as si
    import _volume_inputs as vi
    from test_eval_calib_cli import _setup
    from test_eval_fit_cli import _cfg
    from test_gpu_eval_all_options import D, PlantedAllDetector
    from xas_amd import ops_smplfit, ops_track
    cams, xd, planted = _setup()
    det = PlantedAllDetector()
    det.kps, det.cubes = planted.kps, {}
    B, K = xd['cam_0_joints'].shape[0], det.num_kp
    rng = np.random.Generator(np.random.PCG64(5))
    for i in range(len(cams)):
        centre = det.kps[i][:, 0].double().cpu().numpy()
        L = np.zeros((B, D, D, K * D), np.float32)
        for b in range(B):
            for k in range(K):
                L[b, :, :, k * D:(k + 1) * D] = vi.log_gaussian((centre[b, k] + 1.0) / 2.0 * D, D, 1.0) + 0.02 * rng.normal(size=(D, D, D))
        det.cubes[i] = torch.from_numpy(L).cuda().permute(0, 3, 1, 2)
    model = str(tmp_path / 'smpl.npz')
    np.savez(model, **{k: np.asarray(v) for k, v in si.arrays(70).items()})
    seen, real = [], ops_smplfit.fit_smpl_views

    def spy(points, P, *args, **kw):
        seen.append(dict(kw, points=points, P=P))
        return real(points, P, *args, **kw)
    monkeypatch.setattr(ops_smplfit, 'fit_smpl_views', spy)
    bank = str(tmp_path / 'out' / 'bank.npz')
    keys = dict(tri_weight='spread', tri_volume=True, tri_vol_side=2000.0, tri_vol_grid=8, tri_vol_levels=2, tri_huber=2.5, fit_smpl=bank,
                smpl_model=model, fit_iters=8, fit_data='reproj')
    e = xeval.Eval(_cfg(cams, **keys), det, [dict(xd)], str(tmp_path), tri='robust')
    e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
    assert len(seen) == 1
    kw = seen[0]
    assert kw['views'].dtype == torch.uint8 and tuple(kw['views'].shape) == (B, K) and kw['weighted'] is True and kw['huber'] == 2.5
    assert tuple(kw['points'].shape) == (B, len(cams), K, 3) and tuple(kw['anchor'].shape) == (B, K, 3) and tuple(kw['info'].shape) == (B, K, 6)
    fused = torch.isfinite(kw['anchor']).all(-1)
    assert fused.any() and torch.isfinite(kw['info'][fused]).all()
    with np.load(bank) as z:
        cols = {k: z[k] for k in z.files}
    assert str(cols['fit_data']) == 'reproj' and cols['reproj_rms_px'].shape == (B, 2)
    fitted = cols['status'] != 2
    assert fitted.any() and (cols['cost'][fitted, 1] <= cols['cost'][fitted, 0]).all()
    # the same call, made directly: `used` shows the anchors and no view outside the inliers
    r = real(kw['points'], kw['P'], e.smpl_layer, e.h36m_regressor, {k: torch.as_tensor(cols[k + '_joints']).cuda() for k in ('pose', 'betas', 'trans')},
             views=kw['views'], anchor=kw['anchor'], info=kw['info'], weighted=True, huber=2.5, iters=8, pose_prior=kw['pose_prior'],
             shape_prior=kw['shape_prior'])
    used, views = r['used'].cpu(), kw['views'].cpu()
    usable = fused.cpu() & torch.isfinite(kw['info']).all(-1).cpu()
    assert torch.equal((used & 0x80) != 0, usable)
    given = views != 0
    assert not ((used & 0x3f)[given] & ~views[given]).any()
    assert np.array_equal(r['pose'].float().cpu().numpy(), cols['pose'])


def test_planted_monocular_sequence_is_the_oracles():
    """tests/golden/smplfit_views_planted.npz (the oracle alone, on the CPU): 12 samples, one camera, 2 px of pixel noise, 30 mm of
    depth noise, a tenth of the joints on a decoy 250 to 600 mm down the ray.  The device reproduces the oracle's joint fit on the
    single-view world points and its pixel fit with ray anchors (default weights, 30 trials), and so its two figures: the mean
    distance to the noise-free joints, 63.124 mm against 39.518 mm."""
    from xas_amd import ops_smplfit
    z, p = vc.load_planted(), vc.PLANTED
    layer, hreg = layer_of(p['V'])
    cuda = lambda a: torch.as_tensor(a).cuda()
    N = p['N']
    per = ops_smplfit.fit_smpl(cuda(z['anchor']), torch.ones(N, 18, device='cuda'), layer, hreg, init=split(z['x0']), iters=p['iters'])
    pix = ops_smplfit.fit_smpl_views(cuda(z['points']), cuda(z['P']), layer, hreg, split(z['warm']), anchor=cuda(z['anchor']), info=cuda(z['info']),
                                     iters=p['iters'])
    per, pix = {k: v.cpu() for k, v in per.items()}, {k: v.cpu() for k, v in pix.items()}
    assert (ops_smplfit.POSE_PRIOR, ops_smplfit.SHAPE_PRIOR) == p['joints_priors'] and float(z['margin'].min()) >= 1e-9 and float(z['joints_margin'].min()) >= 1e-9
    assert per['iters'].tolist() == z['joints_iters'].tolist() and per['status'].tolist() == z['joints_status'].tolist()
    assert pix['iters'].tolist() == z['views_iters'].tolist() and pix['status'].tolist() == z['views_status'].tolist()
    assert pix['used'].tolist() == z['used'].tolist()
    # per sample, each fit against its oracle under the bound of that oracle's own spread (the joint fit's: its two assemblies'
    # steps and the distance of tests/_smplfit_oracle.lm's result from the pixel oracle's where the problems coincide)
    xj, xv, worst = join(per), join(pix), [0.0, 0.0]
    for b in range(N):
        gj, gv = vo.rel(xj[b], z['joints_x'][b]), vo.rel(xv[b], z['views_x'][b])
        yj, yv = vo.rel(per['joints'][b], z['joints_joints'][b]), vo.rel(pix['joints'][b], z['views_joints'][b])
        sj, sv = float(z['joints_spread'][b]), float(z['spread'][b])
        print('planted monocular sample %d: joint fit parameters %.2e joints %.2e (oracle spread %.2e, bound %.2e); pixel fit parameters %.2e '
              'joints %.2e (oracle spread %.2e, bound %.2e)' % (b, gj, yj, sj, bound(sj), gv, yv, sv, bound(sv)))
        assert gj <= bound(sj) and yj <= bound(sj) and gv <= bound(sv) and yv <= bound(sv)
        worst = [max(worst[0], bound(sj)), max(worst[1], bound(sv))]
    fig = vc.planted_figures(per['joints'].numpy(), pix['joints'].numpy(), z['clean'])
    ofig = tuple(float(f) for f in z['figures'])
    print('planted monocular, the device: mean distance to the noise-free joints %.3f mm (joint fit) vs %.3f mm (pixel fit with ray anchors)' % fig)
    print('planted monocular, the oracle: %.3f vs %.3f mm' % ofig)
    # the figures are means of distances between joints that agree within those bounds (a distance moves by at most sqrt(3) of it)
    top = float(np.abs(z['views_joints']).max())
    assert abs(fig[0] - ofig[0]) <= 2 * worst[0] * top and abs(fig[1] - ofig[1]) <= 2 * worst[1] * top
    assert ofig[1] < ofig[0] and fig[1] < fig[0]
