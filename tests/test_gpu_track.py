"""xas_track_linearise / xas_track_smooth on the device against the float64 oracle (tests/_track_oracle.py) on the cases of
tests/_track_inputs.py.
Tolerances: the rule of test_gpu_calib.py.  tol = max(16 x the distance the oracle shows between its own two formulations on
that (track, joint), 64 ulps of double), relative to the scale of the quantity: the largest |entry| of the band (of g), the
largest |coordinate| of the points.  `out` is fp32: two doubles that close may round to neighbouring floats, so one fp32 ulp of
the value is added there.  C is one sum of n non-negative terms in another order: n ulps of double bound that.
The oracle follows the device's accept / reject sequence, read off `trials` and `cost` of calls with 1, 2, .. max_iter trials (a
call is a pure function of its inputs, so each is a prefix of the next); it raises if the device decided otherwise than the
oracle at a trial that is no tie."""
import numpy as np
import pytest
import torch

import _track_inputs as ti
import _track_oracle as tk

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
DEV = 'cuda'


def dev(c, rows=None):
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    t = lambda a, dt=None: None if a is None else torch.as_tensor(np.ascontiguousarray(pick(a)), dtype=dt).to(DEV)
    return dict(points=t(c['points']), pmat=t(c['P']), init=t(c['init']), track=t(c['track'], torch.int64),
                frame=t(c['frame'], torch.int64), views=t(c['views']))


def kwargs(c, **over):
    k = dict(weighted=c['weighted'], huber_px=c['huber'], acc_w=c['acc_w'])
    k.update(over)
    return k


def gpu_decisions(d, kw, max_iter):
    """-> decisions [S][K]: per (track, joint) the list of accepted? per trial the device made."""
    from xas_amd import ops_track
    dec, last = None, None
    for m in range(1, max_iter + 1):
        r = ops_track.track_smooth(max_iter=m, want=('trials', 'cost'), **d, **kw)
        trials, cost = r['trials'].cpu().numpy(), r['cost'].cpu().numpy()
        if dec is None:
            dec = [[[] for _ in range(trials.shape[1])] for _ in range(trials.shape[0])]
            last = cost[..., 0].copy()
        for s, k in zip(*np.nonzero(trials == m)):
            dec[s][k].append(bool(cost[s, k, 1] < last[s, k]))
        last = cost[..., 1].copy()
    return dec


def compare(c, got, dec, joints=None, label=''):
    """Every (track, joint) of the case against the oracle made to follow `dec`."""
    out, status, resid = got['xyzw'].cpu().numpy(), got['status'].cpu().numpy(), got['resid'].cpu().numpy()
    ts, cost, trials = got['track_status'].cpu().numpy(), got['cost'].cpu().numpy(), got['trials'].cpu().numpy()
    worst = 0.0
    for s in range(c['S']):
        for k in (range(c['K']) if joints is None else joints):
            trk, rows = tk.make_track(c, s, k)
            a, b = tk.follow(trk, dec[s][k], c['max_iter'])
            dist, scale = tk.distance(a, b)
            tol = max(16 * dist, 64 * EPS)
            assert int(ts[s, k]) == b['status'] and int(trials[s, k]) == b['trials'], (s, k, ts[s, k], trials[s, k], b['status'], b['trials'])
            assert np.array_equal(status[rows, k], b['frame_status'])
            assert np.array_equal(out[rows, k, 3].view(np.uint32), c['init'][rows, k, 3].view(np.uint32))
            assert cost[s, k, 1] <= cost[s, k, 0]
            if trk.passed:
                assert np.array_equal(out[rows, k].view(np.uint32), c['init'][rows, k].view(np.uint32))      # bit for bit, NaN included
                assert np.isnan(resid[rows, k]).all() and cost[s, k].tolist() == [0.0, 0.0]
                continue
            dx = np.abs(out[rows, k, :3].astype(np.float64) - b['X'])
            ulp = np.spacing(np.abs(b['out'][:, :3])).astype(np.float64)
            worst = max(worst, float((dx / (tol * scale + ulp)).max()))
            assert (dx <= tol * scale + ulp).all(), (s, k, float((dx / scale).max()), tol)
            assert np.isfinite(out[rows, k, :3]).all()
            assert abs(cost[s, k, 0] - b['cost'][0]) <= 1e-12 * abs(b['cost'][0]) and abs(cost[s, k, 1] - b['cost'][1]) <= 1e-9 * abs(b['cost'][1])
            assert np.allclose(resid[rows, k], b['resid'], rtol=1e-5, equal_nan=True)
    print('smooth %s%s: largest distance / (tolerance + one fp32 ulp) %.3f' % (c['name'], label, worst))


@pytest.mark.parametrize('name', list(ti.LINEARISE))
def test_linearise_matches_the_oracle(name):
    from xas_amd import ops_track
    c = ti.make(ti.LINEARISE, name)
    d = dev(c)
    for lam in (0.0, 1e-3):
        got = ops_track.track_linearise(lam=lam, **d, **kwargs(c))
        band, g, C = got['band'].cpu().numpy(), got['g'].cpu().numpy(), got['C'].cpu().numpy()
        for k in sorted({0, c['K'] // 2, c['K'] - 1}):
            trk, rows = tk.make_track(c, 0, k)
            H, g1 = trk.dense_system(trk.X0, lam)
            b1, (b2, g2) = tk.Track.band_of(H.numpy()), trk.band_system(trk.X0, lam)
            sb, sg = np.abs(b2).max(), np.abs(g2).max()
            tb, tg = max(16 * np.abs(b1 - b2).max() / sb, 64 * EPS), max(16 * np.abs(g1.numpy() - g2).max() / sg, 64 * EPS)
            rb = np.abs(band[rows, k].reshape(-1, 9) - b2).max() / sb
            rg = np.abs(g[rows, k].reshape(-1) - g2).max() / sg
            Cor = trk.cost(trk.X0)[0]
            n = len(trk.ot) + len(trk.sten)
            print('linearise %s joint %d lambda %g: band %.2e (bound %.2e)  g %.2e (bound %.2e)  C %.2e (bound %.2e)' % (
                name, k, lam, rb, tb, rg, tg, abs(C[0, k] - Cor) / Cor, n * EPS))
            assert rb <= tb and rg <= tg
            assert abs(C[0, k] - Cor) <= n * EPS * Cor


_runs = {}


def run(name):
    """A smoothing case, its result on the device and the device's decisions: computed once and shared."""
    from xas_amd import ops_track
    if name not in _runs:
        c = ti.planted() if name == 'planted' else ti.make(ti.SMOOTH, name)
        d, kw = dev(c), kwargs(c)
        _runs[name] = (c, d, kw, ops_track.track_smooth(max_iter=c['max_iter'], **d, **kw))
    return _runs[name]


@pytest.mark.parametrize('name', [n for n in ti.SMOOTH if n != 'acc_w_0'])
def test_smooth_matches_the_oracle(name):
    from xas_amd import ops_track
    c, d, kw, got = run(name)
    dec = gpu_decisions(d, kw, c['max_iter'])
    compare(c, got, dec)
    status = got['status'].cpu().numpy()
    if name == 'several':                                             # what the case was built to contain
        assert {0, 1, 2} <= set(status.reshape(-1).tolist()) and set(got['track_status'].reshape(-1).tolist()) >= {0, 2}
    if name in ('T1', 'one_data_frame'):
        assert (status == 2).all() and (got['trials'] == 0).all()


@pytest.mark.parametrize('name', list(ti.SMOOTH))
def test_runs_are_bit_identical_whatever_the_workspace_held(name):
    from xas_amd import ops_track
    from xas_amd._lib import query
    c, d, kw, got = run(name)
    again = ops_track.track_smooth(max_iter=c['max_iter'], **d, **kw)
    nbytes, pad = query('xas_track_smooth_workspace_bytes', c['N'], c['K']), 256
    buf = torch.full((nbytes + 2 * pad + 16,), 0xFF, dtype=torch.uint8, device=DEV)          # NaN in every double and float
    off = (-buf.data_ptr() - pad) % 16 + pad
    dirty = ops_track.track_smooth(max_iter=c['max_iter'], workspace=buf[off:off + nbytes], **d, **kw)
    assert (buf[:off] == 0xFF).all() and (buf[off + nbytes:] == 0xFF).all()                   # nothing written outside it
    few = ops_track.track_smooth(max_iter=c['max_iter'], want=(), **d, **kw)
    assert set(few) == {'xyzw', 'tracks'}
    for k in got:
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), k
        assert torch.equal(got[k].view(torch.uint8), dirty[k].view(torch.uint8)), k
    assert torch.equal(got['xyzw'].view(torch.int32), few['xyzw'].view(torch.int32))
    assert (got['cost'][..., 1] <= got['cost'][..., 0]).all()


def test_shuffled_samples_give_the_same_bits():
    from xas_amd import ops_track
    c, d, kw, got = run('several')
    perm = torch.as_tensor(np.random.default_rng(3).permutation(c['N'])).to(DEV)
    sh = {k: (None if v is None else v[perm].contiguous()) for k, v in d.items()}
    mixed = ops_track.track_smooth(max_iter=c['max_iter'], **sh, **kw)
    for k in ('xyzw', 'status', 'resid'):
        assert torch.equal(mixed[k].view(torch.uint8), got[k][perm].contiguous().view(torch.uint8)), k
    for k in ('track_status', 'cost', 'trials', 'tracks'):
        assert torch.equal(mixed[k].view(torch.uint8), got[k].view(torch.uint8)), k
    twice = dict(sh, frame=sh['frame'].clone())
    twice['frame'][1] = twice['frame'][0]
    twice['track'] = torch.zeros_like(twice['track'])
    with pytest.raises(RuntimeError, match='twice'):
        ops_track.track_smooth(**twice, **kw)


def test_without_the_prior_every_frame_is_the_per_frame_refinement():
    """acc_w = 0 and no gap frame: the frames are independent problems under one lambda and one stop per track.  The data
    frames must end where xas_triangulate_refine's cost is no higher than at its own result: both costs in float64 at the fp32
    outputs (_refine_oracle.cost_at), each with the slack that rounding its point to fp32 can add, plus the tolerance floor of
    this file relative to the cost."""
    import _refine_oracle as ro
    from xas_amd import ops_eval
    c, d, kw, got = run('acc_w_0')
    ref = ops_eval.triangulate_refine(d['points'], d['pmat'], d['init'], max_iter=c['max_iter'], want=('status',))
    assert (got['status'] == 0).all() and (ref['status'] != 2).all()
    Cs, ss = ro.cost_at(c['points'], c['P'], got['xyzw'][..., :3].cpu().numpy())
    Cr, sr = ro.cost_at(c['points'], c['P'], ref['xyzw'][..., :3].cpu().numpy())
    print('acc_w 0: largest (C smooth - C refine) / C refine %.3e' % float(((Cs - Cr) / Cr).max()))
    assert (Cs <= Cr + ss + sr + 64 * EPS * Cr).all()
    assert (got['cost'][..., 1] <= got['cost'][..., 0]).all()


def test_planted_noise_is_smoothed_and_the_gap_filled():
    """130 frames, V = 4, K = 18, detections with 2 px of noise, three frames of joint 5 without data: the smoothed track lies
    strictly closer to the true trajectory than xas_triangulate_refine's per-frame points on the data frames (the oracle alone
    shows the same in test_track_abi), and the filled frames are the oracle's fill within the tolerance."""
    from xas_amd import ops_eval
    c, d, kw, got = run('planted')
    k = 5
    ref = ops_eval.triangulate_refine(d['points'], d['pmat'], d['init'], max_iter=30, want=('status',))
    status = got['status'].cpu().numpy()
    data = status == 0
    assert (status[[60, 61, 62], k] == 1).all() and int((status == 1).sum()) == 3 and not (status == 2).any()
    truth = c['truth'].astype(np.float64)
    smooth_mm = np.linalg.norm(got['xyzw'][..., :3].cpu().numpy().astype(np.float64) - truth, axis=-1)
    frame_mm = np.linalg.norm(ref['xyzw'][..., :3].cpu().numpy().astype(np.float64) - truth, axis=-1)
    print('planted: per-frame %.3f mm, smoothed %.3f mm on the data frames; the three filled frames %.3f mm' % (
        frame_mm[data].mean(), smooth_mm[data].mean(), smooth_mm[~data].mean()))
    assert smooth_mm[data].mean() < frame_mm[data].mean()
    assert np.isfinite(smooth_mm[~data]).all()
    dec = gpu_decisions(d, kw, c['max_iter'])
    compare(c, got, dec, joints=[k], label=' joint 5')
