"""xas_smpl_fit_tracks / xas_smpl_fit_tracks_linearise on the GPU against tests/_smplfit_tracks_oracle.py (float64 torch: the
full Jacobian of a track from autograd, the damped normal equations solved densely, the header's LM step for step), on the
synthetic bodies of tests/_smplfit_inputs.py and the interleaved tracks of tests/_smplfit_tracks_cases.py.

Bounds.  Both sides are double arithmetic on the same fp32 inputs and differ by rounding and by the order of their sums.  The
oracle solves every system twice, densely and by eliminating the frames by hand; the distance of its two answers is its own
SPREAD.  A device-to-oracle distance (relative to the largest |entry|) is held to 16 x that spread, the margin of
profiles/track_skeleton_check.txt for the same reason (another summation order), with a floor of 64 ulps of double where the
spread happens to be next to nothing.  A run of this file with -s prints every figure; profiles/smpl_fit_tracks_check.txt keeps
them."""
import numpy as np
import pytest
import torch

import _smplfit_oracle as so
import _smplfit_tracks_cases as tc
import _smplfit_tracks_oracle as to

pytestmark = pytest.mark.gpu

EPS = to.EPS
_cache = {}


PER_FRAME_BOUND = 16 * 9.969e-14     # tests/test_gpu_smplfit.py's PARAM_BOUND (profiles/smpl_fit_check.txt)


def bound(spread):
    return max(16 * spread, 64 * EPS)


def layer_of(V):
    if V not in _cache:
        from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer
        a, m = tc.model(V)
        _cache[V] = (SMPL_Layer.from_arrays(a, center_idx=0).cuda(), torch.as_tensor(a['h36m_regressor']).cuda(), m)
    return _cache[V]


def split(x):
    x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
    return {'pose': torch.cat([x[:, :3], x[:, 6:75]], 1).cuda(), 'trans': x[:, 3:6].contiguous().cuda(), 'betas': x[:, 75:].contiguous().cuda()}


def join(out):
    p = out['pose'].cpu()
    return torch.cat([p[:, :3], out['trans'].cpu(), p[:, 3:], out['betas'].cpu()], 1)


def device(c, fn='fit', rows=None, **kw):
    """The case (or its rows) through ops_smplfit on the GPU -> the op's dict on the CPU."""
    from xas_amd import ops_smplfit
    layer, hreg, _ = layer_of(c['V'])
    rows = np.arange(len(c['track'])) if rows is None else np.asarray(rows)
    op = ops_smplfit.fit_smpl_tracks if fn == 'fit' else ops_smplfit.linearise_smpl_tracks
    out = op(torch.as_tensor(c['tgt'][rows]).cuda(), torch.as_tensor(c['w'][rows]).cuda(), c['track'][rows], c['frame'][rows], layer, hreg,
             init=split(c['x0'][rows]), pose_prior=tc.WP, shape_prior=tc.WS, **kw)
    return {k: v.cpu() for k, v in out.items()}


def fit_of(name):
    if ('fit', name) not in _cache:
        _cache[('fit', name)] = device(tc.build(name), iters=tc.FIT_ITERS)
    return _cache[('fit', name)]


@pytest.mark.parametrize('lam', (1e-3, 10.0))
@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_linearise_against_the_oracle(name, lam):
    c = tc.build(name, extras=True)
    out = device(c, 'lin', lam=lam)
    tracks = tc.tracks_of_case(c)
    assert out['track_ids'].tolist() == [s for s, _, _ in tracks]
    for k, (s, rows, trk) in enumerate(tracks):
        dy = out['d_y'][rows]
        assert not dy[[i for i, u in enumerate(trk.usable) if not u]].any()          # passed through: no step
        if trk.T == 0:
            assert not out['reduced'][k].any() and not out['rhs'][k].any() and not out['d_beta'][k].any()
            continue
        H, g = trk.normal(trk.y0, trk.beta0)
        sch, dense = to.solve_schur(H, g, lam, trk.T), to.solve_dense(H, g, lam)
        Alu, blu = to.reduced_by_lu(H, g, lam, trk.T)
        costs = trk.frame_costs(trk.y0, trk.beta0)
        C, Crev = trk.cost(trk.y0, trk.beta0), float(sum(reversed(costs)))
        sA, sb, sC = to.rel(Alu, sch['reduced']), to.rel(blu, sch['rhs']), abs(C - Crev) / C
        gA, gb, gC = to.rel(out['reduced'][k], sch['reduced']), to.rel(out['rhs'][k], sch['rhs']), abs(float(out['cost'][k]) - C) / C
        d_dev = torch.cat([dy[trk.rows].reshape(-1), out['d_beta'][k]])
        r_own = max(to.residual_of(H, g, lam, dense), to.residual_of(H, g, lam, sch['d']))
        r_dev = to.residual_of(H, g, lam, d_dev)
        print('tracks linearise %s track %d (T = %d) lambda %g: reduced %.2e (spread %.2e, bound %.2e)  rhs %.2e (spread %.2e, bound %.2e)  '
              'C %.2e (spread %.2e, bound %.2e)  residual of d %.2e (the oracle\'s own %.2e, bound %.2e)  step gap %.2e (spread %.2e)'
              % (name, s, trk.T, lam, gA, sA, bound(sA), gb, sb, bound(sb), gC, sC, bound(sC), r_dev, r_own, bound(r_own),
                 to.rel(d_dev, dense), to.rel(sch['d'], dense)))
        assert gA <= bound(sA) and gb <= bound(sb) and gC <= bound(sC)
        assert r_dev <= bound(r_own)
        assert torch.isfinite(out['reduced'][k]).all() and torch.equal(out['reduced'][k], out['reduced'][k].T)


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_fit_follows_the_oracles_lm(name):
    c, out = tc.build(name), fit_of(name)
    x = join(out)
    for k, (s, rows, trk, r) in enumerate(tc.oracle_fit(name)):
        assert r['margin'] >= 1e-9                                                  # comparable decisions (tests/test_smplfit_tracks_abi.py)
        assert int(out['track_status'][k]) == r['status'] == 1 and int(out['track_trials'][k]) == r['trials']
        assert out['status'][rows].tolist() == [0 if u else 2 for u in trk.usable]
        xo = torch.cat([r['y'], r['beta'].expand(trk.T, 10)], 1)
        gx, gb = to.rel(x[rows], xo), to.rel(out['track_betas'][k], r['beta'])
        gc = abs(float(out['track_cost'][k, 1]) - r['cost'][1]) / r['cost'][1]
        print('tracks fit %s track %d (T = %d): %d trials, cost %.3f -> %.6f (oracle %.6f, gap %.2e), parameters %.2e, betas %.2e '
              '(oracle spread %.2e, bound %.2e)' % (name, s, trk.T, r['trials'], float(out['track_cost'][k, 0]), float(out['track_cost'][k, 1]),
                                                  r['cost'][1], gc, gx, gb, r['spread'], bound(r['spread'])))
        assert gx <= bound(r['spread']) and gb <= bound(r['spread'])
        assert float(out['track_cost'][k, 1]) <= float(out['track_cost'][k, 0])
        assert torch.equal(out['betas'][rows], out['track_betas'][k].expand(len(rows), 10))
        assert abs(float(out['cost'][rows, 1].sum()) - float(out['track_cost'][k, 1])) <= 1e-12 * r['cost'][1]


def test_tracks_of_one_frame_are_the_per_sample_fit():
    from xas_amd import ops_smplfit
    c, out = tc.build('singles_V70'), fit_of('singles_V70')
    layer, hreg, _ = layer_of(c['V'])
    one = ops_smplfit.fit_smpl(torch.as_tensor(c['tgt']).cuda(), torch.as_tensor(c['w']).cuda(), layer, hreg, init=split(c['x0']),
                               iters=tc.FIT_ITERS, pose_prior=tc.WP, shape_prior=tc.WS)
    one = {k: v.cpu() for k, v in one.items()}
    k = out['track'].long()                                                         # sample -> its track's row
    gap = to.rel(join(out), join(one))
    print('tracks of one frame vs xas_smpl_fit: parameter gap %.2e, costs identical: %s' % (gap, torch.equal(out['cost'], one['cost'])))
    assert torch.equal(out['cost'], one['cost']) and torch.equal(out['track_cost'][k], one['cost'])
    assert torch.equal(out['track_trials'][k], one['iters']) and torch.equal(out['track_status'][k], one['status'])
    assert gap <= max(bound(r['spread']) for _, _, _, r in tc.oracle_fit('singles_V70'))


def test_pass_through_and_edges():
    from xas_amd import ops_smplfit
    c = tc.build('mixed_V70', extras=True)
    full = device(c, iters=tc.FIT_ITERS)
    passed = np.nonzero(full['status'].numpy() == 2)[0]
    assert len(passed) == 3
    x0 = torch.as_tensor(c['x0']).float().double()
    assert torch.equal(join(full)[passed], x0[passed])                             # the init, bit for bit
    assert torch.equal(full['cost'][passed, 0], full['cost'][passed, 1])
    keep = np.setdiff1d(np.arange(len(c['track'])), passed)
    less = device(c, rows=keep, iters=tc.FIT_ITERS)
    for key in ('pose', 'trans', 'joints', 'cost', 'status', 'betas'):
        assert torch.equal(full[key][keep], less[key]), key
    for key in ('track_betas', 'track_cost', 'track_trials', 'track_status'):       # the last track exists in `full` alone
        assert torch.equal(full[key][:3], less[key]), key
    assert int(full['track_status'][3]) == 2 and int(full['track_trials'][3]) == 0
    rows3 = np.nonzero(c['track'] == 3)[0]
    rows3 = rows3[np.argsort(c['frame'][rows3])]
    mean = (x0[rows3[0], 75:] + x0[rows3[1], 75:]) / 2
    assert torch.equal(full['track_betas'][3], mean)
    assert (full['track_cost'][:, 1] <= full['track_cost'][:, 0]).all()
    # no trial: the start, status trial limit
    zero = device(c, iters=0)
    fitted = zero['status'].numpy() == 0
    assert zero['track_status'].tolist() == [1, 1, 1, 2] and zero['track_trials'].tolist() == [0, 0, 0, 0]
    assert torch.equal(join(zero)[:, :75], x0[:, :75]) and torch.equal(zero['track_cost'][:, 0], zero['track_cost'][:, 1])
    for k, (s, rows, trk) in enumerate(tc.tracks_of_case(c)):
        if trk.T:
            assert torch.equal(zero['track_betas'][k], trk.beta0)
            assert torch.equal(zero['betas'][rows[trk.rows]], trk.beta0.expand(trk.T, 10))
    assert fitted.sum() == len(keep)
    # nothing to do
    layer, hreg, _ = layer_of(70)
    e = lambda *s: torch.zeros(*s, device='cuda')
    none = ops_smplfit.fit_smpl_tracks(e(0, 18, 3), e(0, 18), np.zeros(0, np.int64), np.zeros(0, np.int64), layer, hreg,
                                       init={'pose': e(0, 72), 'betas': e(0, 10), 'trans': e(0, 3)})
    assert none['pose'].shape == (0, 72) and none['track_betas'].shape == (0, 10)
    # tracks without a sample, through the C entry point with no model arrays at all: nothing of them is read
    from xas_amd import _lib
    S = 2
    ws = torch.empty(ops_smplfit.tracks_workspace_bytes(0, 70, S), dtype=torch.uint8, device='cuda')
    tb, tcst = torch.full((S, 10), 7.0, dtype=torch.float64, device='cuda'), torch.full((S, 2), 7.0, dtype=torch.float64, device='cuda')
    tt, tst = torch.full((S,), 7, dtype=torch.int32, device='cuda'), torch.full((S,), 7, dtype=torch.uint8, device='cuda')
    _lib.call('xas_smpl_fit_tracks', *([None] * 16), 1.0, 1.0, 0, 70, S, 0, 5, None, None, None, None, None, _lib.ptr(tb), _lib.ptr(tcst),
              _lib.ptr(tt), _lib.ptr(tst), _lib.ptr(ws))
    assert not tb.any() and not tcst.any() and tt.tolist() == [0, 0] and tst.tolist() == [2, 2]


def test_runs_are_bit_identical():
    from xas_amd import ops_smplfit
    c, first = tc.build('mixed_V70', extras=True), None
    N, S = len(c['track']), 4
    nbytes = ops_smplfit.tracks_workspace_bytes(N, c['V'], S)
    runs = [device(c, iters=tc.FIT_ITERS), device(c, iters=tc.FIT_ITERS)]
    for fill in (0xFF, 0x55):
        runs.append(device(c, iters=tc.FIT_ITERS, workspace=torch.full((nbytes,), fill, dtype=torch.uint8, device='cuda')))
    for r in runs[1:]:
        for key in runs[0]:
            assert torch.equal(r[key], runs[0][key]), key
    perm = np.random.Generator(np.random.PCG64(9)).permutation(N)
    moved = device(c, rows=perm, iters=tc.FIT_ITERS)
    for key in ('pose', 'trans', 'joints', 'cost', 'status', 'betas', 'track'):
        assert torch.equal(moved[key], runs[0][key][perm]), key
    for key in ('track_betas', 'track_cost', 'track_trials', 'track_status', 'track_ids'):
        assert torch.equal(moved[key], runs[0][key]), key
    lin = [device(c, 'lin', lam=1e-3), device(c, 'lin', rows=perm, lam=1e-3)]
    assert torch.equal(lin[1]['d_y'], lin[0]['d_y'][perm])
    for key in ('reduced', 'rhs', 'd_beta', 'cost'):
        assert torch.equal(lin[1][key], lin[0][key]), key


def test_planted_sequence_is_the_oracles():
    from xas_amd import ops_smplfit
    p, z = tc.planted_inputs(), tc.load_planted()
    T, iters = tc.PLANTED['T'], tc.PLANTED['iters']
    layer, hreg, _ = layer_of(tc.PLANTED['V'])
    tg, w = torch.as_tensor(p['tgt']).cuda(), torch.ones(T, 18, device='cuda')
    trk = ops_smplfit.fit_smpl_tracks(tg, w, np.zeros(T, np.int64), np.arange(T), layer, hreg, init=split(p['x0']), iters=iters,
                                      pose_prior=tc.WP, shape_prior=tc.WS)
    per = ops_smplfit.fit_smpl(tg, w, layer, hreg, init=split(p['x0']), iters=iters, pose_prior=tc.WP, shape_prior=tc.WS)
    trk, per = {k: v.cpu() for k, v in trk.items()}, {k: v.cpu() for k, v in per.items()}
    assert float(z['margin']) >= 1e-9
    assert int(trk['track_trials'][0]) == int(z['trials']) and int(trk['track_status'][0]) == int(z['status'])
    gap, gap_f = to.rel(join(trk), torch.as_tensor(z['x'])), to.rel(join(per), torch.as_tensor(z['frames_x']))
    fig = tc.planted_figures(trk['track_betas'][0].numpy(), trk['joints'].numpy(), per['betas'].numpy(), per['joints'].numpy(), p)
    ofig = tc.planted_figures(z['x'][0, 75:], z['joints'], z['frames_x'][:, 75:], z['frames_joints'], p)
    print('planted on the device: |beta - truth| %.4f (track) vs %.4f (per frame); joints from the noise-free joints %.3f vs %.3f mm'
          % fig)
    print('planted, the oracle:   |beta - truth| %.4f (track) vs %.4f (per frame); joints %.3f vs %.3f mm; parameter gap %.2e '
          '(track; spread %.2e, bound %.2e), %.2e (per frame)' % (*ofig, gap, float(z['spread']), bound(float(z['spread'])), gap_f))
    assert gap <= bound(float(z['spread']))
    # the per-frame half of the comparison: xas_smpl_fit against its oracle, by the bound of its own tests
    assert gap_f <= PER_FRAME_BOUND
    assert fig[0] < fig[1] and fig[2] <= fig[3]
    assert ofig[0] < ofig[1] and ofig[2] <= ofig[3]
