"""xas_smpl_fit_tracks_smooth / _linearise on the GPU against tests/_smplfit_smooth_oracle.py (float64 torch: the full Jacobian of
a track with the acceleration prior's rows by autograd, the damped normal equations solved densely and by a block recurrence
with border, the header's LM step for step), on the interleaved tracks of tests/_smplfit_smooth_cases.py.

Bounds.  Those of tests/test_gpu_smplfit_tracks.py, for its reason (another summation order): a device-to-oracle distance,
relative to the largest |entry|, is held to 16 x the oracle's own SPREAD (the distance of its two solves, or of two orders of a
sum), with a floor of 64 ulps of double.  A run with -s prints every figure; profiles/smpl_fit_smooth_check.txt keeps them."""
import numpy as np
import pytest
import torch

import _smplfit_smooth_cases as sc
import _smplfit_smooth_oracle as sm
import _smplfit_tracks_oracle as to
from test_gpu_smplfit_tracks import bound, join, layer_of, split

pytestmark = pytest.mark.gpu

_cache = {}
NY = 75


def device(c, fn='fit', rows=None, smooth=True, rot_w=None, trans_w=None, **kw):
    """The case (or its rows) through ops_smplfit on the GPU -> the op's dict on the CPU."""
    from xas_amd import ops_smplfit
    layer, hreg, _ = layer_of(c['V'])
    rows = np.arange(len(c['track'])) if rows is None else np.asarray(rows)
    if smooth:
        op = ops_smplfit.fit_smpl_tracks_smooth if fn == 'fit' else ops_smplfit.linearise_smpl_tracks_smooth
        kw.update(rot_w=c['rot_w'] if rot_w is None else rot_w, trans_w=c['trans_w'] if trans_w is None else trans_w)
    else:
        op = ops_smplfit.fit_smpl_tracks if fn == 'fit' else ops_smplfit.linearise_smpl_tracks
    out = op(torch.as_tensor(c['tgt'][rows]).cuda(), torch.as_tensor(c['w'][rows]).cuda(), c['track'][rows], c['frame'][rows], layer, hreg,
             init=split(c['x0'][rows]), pose_prior=sc.WP, shape_prior=sc.WS, **kw)
    return {k: v.cpu() for k, v in out.items()}


def fit_of(name):
    if name not in _cache:
        _cache[name] = device(sc.build(name), iters=sc.FIT_ITERS)
    return _cache[name]


def damped(H, lam):
    return H + lam * torch.diag(torch.diagonal(H))


@pytest.mark.parametrize('lam', (1e-3, 10.0))
@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_linearise_against_the_oracle(name, lam):
    c = sc.build(name)
    out = device(c, 'lin', lam=lam)
    tracks = sc.tracks_of_case(c)
    assert out['track_ids'].tolist() == [s for s, _, _ in tracks]
    for k, (s, rows, trk) in enumerate(tracks):
        off = [i for i, u in enumerate(trk.usable) if not u]
        for key in ('d_y', 'g_y', 'hdiag', 'hoff', 'border'):                        # passed through: zeros
            assert not out[key][rows[off]].any(), key
        if trk.T == 0:
            assert not out['corner'][k].any() and not out['g_beta'][k].any() and not out['d_beta'][k].any() and float(out['cost'][k]) == 0
            continue
        T, n, use = trk.T, NY * trk.T, rows[trk.rows]
        H, g = trk.normal(trk.y0, trk.beta0)
        A = damped(H, lam)
        Hrev, grev = (lambda J, r: (J.flip(0).T @ J.flip(0), J.flip(0).T @ r.flip(0)))(*_full_jacobian(trk))
        sH, sg = to.rel(damped(Hrev, lam), A), to.rel(grev, g)                       # the same sums in the opposite order
        body = torch.zeros(n, n, dtype=torch.float64)
        W = torch.diag(trk.wvec)
        for i in range(T):
            body[NY * i:NY * (i + 1), NY * i:NY * (i + 1)] = out['hdiag'][use[i]]
            if i >= 1:
                body[NY * i:NY * (i + 1), NY * (i - 1):NY * i] = out['hoff'][use[i], 0] * W
                body[NY * (i - 1):NY * i, NY * i:NY * (i + 1)] = out['hoff'][use[i], 0] * W
            if i >= 2:
                body[NY * i:NY * (i + 1), NY * (i - 2):NY * (i - 1)] = out['hoff'][use[i], 1] * W
                body[NY * (i - 2):NY * (i - 1), NY * i:NY * (i + 1)] = out['hoff'][use[i], 1] * W
        border = torch.cat([out['border'][use[i]] for i in range(T)], 1)             # [10, 75 T]
        g_dev = torch.cat([out['g_y'][use].reshape(-1), out['g_beta'][k]])
        big = float(A.abs().max())
        gB = float((body - A[:n, :n]).abs().max()) / big
        gb = float((border - A[n:, :n]).abs().max()) / big
        gc = float((out['corner'][k] - A[n:, n:]).abs().max()) / big
        gg = to.rel(g_dev, g)
        C = trk.total(trk.y0, trk.beta0)
        Crev = float(sum(reversed(trk.frame_costs(trk.y0, trk.beta0)))) + trk.prior_cost(trk.y0)
        sC, gC = abs(C - Crev) / C, abs(float(out['cost'][k]) - C) / C
        dense, blk = to.solve_dense(H, g, lam), sm.solve_block(H, g, lam, T)
        d_dev = torch.cat([out['d_y'][use].reshape(-1), out['d_beta'][k]])
        r_own = max(to.residual_of(H, g, lam, dense), to.residual_of(H, g, lam, blk))
        r_dev = to.residual_of(H, g, lam, d_dev)
        print('smooth linearise %s track %d (T = %d) lambda %g: body %.2e border %.2e corner %.2e (spread %.2e, bound %.2e)  rhs %.2e '
              '(spread %.2e, bound %.2e)  C %.2e (spread %.2e, bound %.2e)  residual of d %.2e (the oracle\'s own %.2e, bound %.2e)  '
              'step gap %.2e (spread %.2e)' % (name, s, T, lam, gB, gb, gc, sH, bound(sH), gg, sg, bound(sg), gC, sC, bound(sC), r_dev,
                                              r_own, bound(r_own), to.rel(d_dev, dense), to.rel(blk, dense)))
        assert max(gB, gb, gc) <= bound(sH) and gg <= bound(sg) and gC <= bound(sC)
        assert r_dev <= bound(r_own)
        assert torch.isfinite(out['corner'][k]).all() and torch.equal(out['corner'][k], out['corner'][k].T)
        assert torch.isfinite(d_dev).all() and d_dev.abs().max() > 0


def _full_jacobian(trk):
    """The track's whole residual and Jacobian, data rows then the prior's: (J [R, 75 T + 10], r [R])."""
    r, J = trk.jacobian(trk.y0, trk.beta0)
    if trk.temporal:
        Jp = torch.autograd.functional.jacobian(lambda v: trk.prior_residual(v.view(trk.T, NY)), trk.y0.reshape(-1))
        J = torch.cat([J, torch.cat([Jp, torch.zeros(len(Jp), 10, dtype=torch.float64)], 1)])
        r = torch.cat([r, trk.prior_residual(trk.y0)])
    return J, r


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_fit_follows_the_oracles_lm(name):
    out = fit_of(name)
    x = join(out)
    for k, (s, rows, trk, r) in enumerate(sc.oracle_fit(name)):
        assert out['status'][rows].tolist() == [0 if u else 2 for u in trk.usable]
        assert int(out['track_status'][k]) == r['status'] and int(out['track_trials'][k]) == r['trials']
        if trk.T == 0:
            continue
        assert r['margin'] >= 1e-9                                                  # comparable decisions (tests/test_smplfit_smooth_abi.py)
        use = rows[trk.rows]
        xo = torch.cat([r['y'], r['beta'].expand(trk.T, 10)], 1)
        gx, gb = to.rel(x[use], xo), to.rel(out['track_betas'][k], r['beta'])
        gc = abs(float(out['track_cost'][k, 1]) - r['cost'][1]) / r['cost'][1]
        gf = to.rel(out['cost'][use], torch.as_tensor(r['frame_cost']))
        print('smooth fit %s track %d (T = %d): %d trials, cost %.3f -> %.6f (oracle %.6f, gap %.2e), parameters %.2e, betas %.2e, frame '
              'costs %.2e (oracle spread %.2e, bound %.2e)' % (name, s, trk.T, r['trials'], float(out['track_cost'][k, 0]),
                                                             float(out['track_cost'][k, 1]), r['cost'][1], gc, gx, gb, gf, r['spread'],
                                                             bound(r['spread'])))
        assert gx <= bound(r['spread']) and gb <= bound(r['spread'])
        assert float(out['track_cost'][k, 1]) <= float(out['track_cost'][k, 0])
        assert torch.equal(out['betas'][use], out['track_betas'][k].expand(len(use), 10))
    passed = np.nonzero(out['status'].numpy() == 2)[0]
    c = sc.build(name)
    assert torch.equal(join(out)[passed], torch.as_tensor(c['x0']).float().double()[passed])   # the init, bit for bit


def test_agrees_with_the_track_fit_where_the_problems_coincide():
    """Both weights 0 (every track), and tracks of fewer than three frames at any weights: xas_smpl_fit_tracks' problem."""
    for name, pick in (('zero_V70', lambda T: True), ('mixed_V70', lambda T: 0 < T < 3)):
        c = sc.build(name)
        if name == 'mixed_V70':                                                     # without the repeated frame: the track fit keeps it
            keep = np.nonzero(~((c['track'] == 2) & (c['w'].sum(1) > 6) & _repeats(c)))[0]
            c = {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        for lam in (1e-3, 10.0):
            new, old = device(c, 'lin', lam=lam), device(c, 'lin', smooth=False, lam=lam)
            for k, (s, rows, trk) in enumerate(sc.tracks_of_case(c)):
                if not pick(trk.T):
                    continue
                use, n = rows[trk.rows], NY * trk.T
                H, g = trk.normal(trk.y0, trk.beta0)
                dense, blk, sch = to.solve_dense(H, g, lam), sm.solve_block(H, g, lam, trk.T), to.solve_schur(H, g, lam, trk.T)
                spread = max(to.rel(blk, dense), to.rel(sch['d'], dense))
                d_new = torch.cat([new['d_y'][use].reshape(-1), new['d_beta'][k]])
                d_old = torch.cat([old['d_y'][use].reshape(-1), old['d_beta'][k]])
                # the reduced system of the new exports: corner - sum_i B_i Hd_i^-1 B_i^T
                red = new['corner'][k].clone()
                rhs = -new['g_beta'][k].clone()
                for f in use:
                    X = torch.linalg.solve(new['hdiag'][f], torch.cat([new['border'][f].T, -new['g_y'][f].unsqueeze(1)], 1))
                    red, rhs = red - new['border'][f] @ X[:, :10], rhs - new['border'][f] @ X[:, 10]
                Alu, blu = to.reduced_by_lu(H, g, lam, trk.T)
                sA, sb = to.rel(Alu, sch['reduced']), to.rel(blu, sch['rhs'])
                gd, gA, gb = to.rel(d_new, d_old), to.rel(red, old['reduced'][k]), to.rel(rhs, old['rhs'][k])
                print('smooth vs track fit %s track %d (T = %d) lambda %g: step %.2e (spread %.2e, bound %.2e)  reduced %.2e (spread %.2e, '
                      'bound %.2e)  rhs %.2e (spread %.2e, bound %.2e)' % (name, s, trk.T, lam, gd, spread, bound(spread), gA, sA, bound(sA),
                                                                          gb, sb, bound(sb)))
                assert gd <= bound(spread) and gA <= bound(sA) and gb <= bound(sb)
                assert float(new['cost'][k]) == pytest.approx(float(old['cost'][k]), rel=64 * to.EPS)


def _repeats(c):
    """[N] bool: the sample repeats the frame number of an earlier sample of its track."""
    out = np.zeros(len(c['track']), bool)
    for s in set(c['track'].tolist()):
        rows = np.nonzero(c['track'] == s)[0]
        rows = rows[np.argsort(c['frame'][rows], kind='stable')]
        for a, b in zip(rows, rows[1:]):
            out[b] = c['frame'][a] == c['frame'][b]
    return out


def test_runs_are_bit_identical():
    from xas_amd import ops_smplfit
    c = sc.build('mixed_V70')
    N, S = len(c['track']), len(set(c['track'].tolist()))
    nbytes = ops_smplfit.tracks_smooth_workspace_bytes(N, c['V'], S)
    runs = [fit_of('mixed_V70')]
    for fill in (0xFF, 0x55):
        runs.append(device(c, iters=sc.FIT_ITERS, workspace=torch.full((nbytes,), fill, dtype=torch.uint8, device='cuda')))
    for r in runs[1:]:
        for key in runs[0]:
            assert torch.equal(r[key], runs[0][key]), key
    perm = np.random.Generator(np.random.PCG64(9)).permutation(N)
    moved = device(c, rows=perm, iters=sc.FIT_ITERS)
    for key in ('pose', 'trans', 'joints', 'cost', 'status', 'betas', 'track'):
        assert torch.equal(moved[key], runs[0][key][perm]), key
    for key in ('track_betas', 'track_cost', 'track_trials', 'track_status', 'track_ids'):
        assert torch.equal(moved[key], runs[0][key]), key
    lin = [device(c, 'lin', lam=1e-3, workspace=torch.full((nbytes,), 0xFF, dtype=torch.uint8, device='cuda')),
           device(c, 'lin', lam=1e-3, workspace=torch.full((nbytes,), 0x55, dtype=torch.uint8, device='cuda')),
           device(c, 'lin', rows=perm, lam=1e-3)]
    for key in ('hdiag', 'hoff', 'border', 'g_y', 'd_y'):
        assert torch.equal(lin[1][key], lin[0][key]) and torch.equal(lin[2][key], lin[0][key][perm]), key
    for key in ('corner', 'g_beta', 'd_beta', 'cost'):
        assert torch.equal(lin[1][key], lin[0][key]) and torch.equal(lin[2][key], lin[0][key]), key


def test_unwrapped_start_and_edges():
    c = sc.build('wrap_V70')
    zero = device(c, iters=0)
    for k, (s, rows, trk) in enumerate(sc.tracks_of_case(c)):
        use = rows[trk.rows]
        y = join(zero)[use, :NY]
        assert torch.equal(y[:, 3:], trk.y0[:, 3:]) and torch.equal(y[0], trk.y0[0])  # all but the unwrapped vectors: the init's bits
        assert to.rel(y[:, :3], trk.y0[:, :3]) <= bound(0.0)                        # those: the oracle's within the floor of 64 ulps
        assert int(zero['track_trials'][k]) == 0 and torch.equal(zero['track_cost'][k, 0], zero['track_cost'][k, 1])
    assert float((sc.tracks_of_case(c)[0][2].raw_y0 - sc.tracks_of_case(c)[0][2].y0).abs().max()) > 3.0
    # tracks without a sample, through the C entry point with no model arrays at all
    from xas_amd import _lib, ops_smplfit
    S = 2
    ws = torch.empty(ops_smplfit.tracks_smooth_workspace_bytes(0, 70, S), dtype=torch.uint8, device='cuda')
    tb, tcst = torch.full((S, 10), 7.0, dtype=torch.float64, device='cuda'), torch.full((S, 2), 7.0, dtype=torch.float64, device='cuda')
    tt, tst = torch.full((S,), 7, dtype=torch.int32, device='cuda'), torch.full((S,), 7, dtype=torch.uint8, device='cuda')
    _lib.call('xas_smpl_fit_tracks_smooth', *([None] * 16), 1.0, 1.0, 1e4, 1.0, 0, 70, S, 0, 5, None, None, None, None, None, _lib.ptr(tb),
              _lib.ptr(tcst), _lib.ptr(tt), _lib.ptr(tst), _lib.ptr(ws))
    assert not tb.any() and not tcst.any() and tt.tolist() == [0, 0] and tst.tolist() == [2, 2]


def test_eval_writes_the_smoothed_file(tmp_path):
    """eval.py's Eval through the synthetic loader of tests/test_eval_fit_cli.py with fit_shape track, with and without fit_smooth."""
    import re
    import eval as xeval
    from test_eval_fit_cli import _cfg, _setup
    cams, xd, det, model, smpl = _setup(tmp_path)
    B = xd['cam_0_joints'].shape[0]
    paths = [['seq0/img_%06d.jpg' % (b * B + i) for i in range(B)] for b in range(2)]       # one sequence: a track of 2 B frames
    batches = [dict(xd, cam_0_img_path=paths[b]) for b in range(2)]
    banks, texts = {}, {}
    for tag, keys in (('track', {}), ('again', {}), ('smooth', dict(fit_smooth=1e4, fit_smooth_trans=0.5))):
        banks[tag] = str(tmp_path / tag / 'bank.npz')
        e = xeval.Eval(_cfg(cams, fit_smpl=banks[tag], smpl_model=model, fit_iters=8, fit_shape='track', **keys), det,
                       [dict(b) for b in batches], str(tmp_path / tag))
        e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt').read().strip().split('\n')
        with np.load(banks[tag]) as z:
            banks[tag] = {k: z[k] for k in z.files}
    old, new = banks['track'], banks['smooth']
    assert sorted(banks['again']) == sorted(old) and all(np.array_equal(old[k], banks['again'][k], equal_nan=True) for k in old)
    assert texts['again'] == texts['track'] and 'smoothed over frames' not in texts['track'][-1]
    assert sorted(new) == sorted(list(old) + ['fit_smooth', 'joint_accel_mm'])
    assert new['fit_smooth'].tolist() == [1e4, 0.5] and new['joint_accel_mm'].shape == (2 * B, 3)
    assert np.isnan(new['joint_accel_mm'][:, 1]).all()                               # no unsmoothed track fit was run
    inner = np.isfinite(new['joint_accel_mm'][:, 2])
    assert np.array_equal(inner, np.isfinite(new['joint_accel_mm'][:, 0]))
    for s in np.unique(new['track']):
        rows = np.nonzero((new['track'] == s) & (new['status'] != 2))[0]
        assert inner[rows].sum() == max(len(rows) - 2, 0)                            # NaN at the two ends of a track
    m = re.search(r'smoothed over frames \(weights 10000\.0 0\.5\): joint acceleration (\S+) -> (\S+) mm / frame\^2, joint RMS (\S+) -> (\S+) mm$',
                  texts['smooth'][-1])
    assert m and texts['smooth'][-1].startswith(texts['track'][-1].split(': joint RMS')[0])
    assert float(m.group(2)) == pytest.approx(float(np.nanmean(new['joint_accel_mm'][:, 2])), rel=1e-6)
    print('eval --fit-smooth: ' + m.group(0))


def test_planted_sequence_is_the_oracles():
    p, z = sc.planted_inputs(), sc.load_planted()
    T = sc.PLANTED['T']
    c = dict(V=sc.PLANTED['V'], x0=p['x0'], tgt=p['tgt'], w=np.ones((T, 18), np.float32), track=np.zeros(T, np.int64), frame=p['frames'],
             rot_w=sc.PLANTED['rot_w'], trans_w=sc.PLANTED['trans_w'])
    new, old = device(c, iters=sc.PLANTED['iters']), device(c, smooth=False, iters=sc.PLANTED['iters'])
    assert float(z['margin']) >= 1e-9 and float(z['track_margin']) >= 1e-9
    assert int(new['track_trials'][0]) == int(z['trials']) and int(new['track_status'][0]) == int(z['status'])
    gap, gap0 = to.rel(join(new), torch.as_tensor(z['x'])), to.rel(join(old), torch.as_tensor(z['track_x']))
    fig = sc.planted_figures(new['joints'].numpy(), old['joints'].numpy(), p)
    ofig = sc.planted_figures(z['joints'], z['track_joints'], p)
    print('planted on the device: joints from the noise-free joints %.3f mm (smoothed) vs %.3f mm (track fit); mean joint acceleration '
          '%.3f vs %.3f mm / frame^2' % fig)
    print('planted, the oracle:   %.3f vs %.3f mm; %.3f vs %.3f mm / frame^2; parameter gap %.2e (smoothed; spread %.2e, bound %.2e), %.2e '
          '(track fit; spread %.2e, bound %.2e)' % (*ofig, gap, float(z['spread']), bound(float(z['spread'])), gap0, float(z['track_spread']),
                                                    bound(float(z['track_spread']))))
    assert gap <= bound(float(z['spread'])) and gap0 <= bound(float(z['track_spread']))
    # the figures are means over the joints: the joints themselves within the bound
    assert to.rel(new['joints'], torch.as_tensor(z['joints'])) <= bound(float(z['spread']))
    assert to.rel(old['joints'], torch.as_tensor(z['track_joints'])) <= bound(float(z['track_spread']))
    assert fig[0] < fig[1] and fig[2] < fig[3]
