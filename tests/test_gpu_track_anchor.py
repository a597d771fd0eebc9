"""xas_track_anchor_linearise / xas_track_anchor_smooth on the device against the float64 oracle
(tests/_track_anchor_oracle.py) on the cases of tests/_track_anchor_inputs.py, and against xas_track_smooth / xas_track_linearise
bit for bit where no anchors are given.
Tolerances: the rule of test_gpu_track.py.  tol = max(16 x the distance the oracle shows between its own two formulations on
that (track, joint), 64 ulps of double), relative to the scale of the quantity: the largest |entry| of the band (of g), the
largest |coordinate| of the points.  `out` is fp32, so one fp32 ulp of the value is added there.  C is one sum of n non-negative
terms in another order: n ulps of double bound that.
The oracle follows the device's accept / reject sequence, read off `trials` and `cost` of calls with 1, 2, .. max_iter trials;
it raises if the device decided otherwise than the oracle at a trial that is no tie."""
import numpy as np
import pytest
import torch

import _track_anchor_inputs as ai
import _track_anchor_oracle as ao
import _track_inputs as ti
import _track_oracle as tk

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
DEV = 'cuda'


def dev(c):
    t = lambda a, dt=None: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    return dict(points=t(c['points']), pmat=t(c['P']), init=t(c['init']), track=t(c['track'], torch.int64),
                frame=t(c['frame'], torch.int64), views=t(c['views']), anchor=t(c.get('anchor')), info=t(c.get('info')))


def kwargs(c):
    return dict(weighted=c['weighted'], huber_px=c['huber'], acc_w=c['acc_w'], anchor_huber=c.get('anchor_huber', 0.0))


def joints_of(c):
    """Every joint of a small K; of K = 18 both ends, the middle and the joints the case planted something in."""
    if c['K'] <= 3:
        return list(range(c['K']))
    spec = ai.CASES.get(c['name'], {})
    planted = {k for key in ('nan', 'zero_trace', 'anchor_nan', 'decoy', 'behind', 'gaps') for _, _, k in spec.get(key, ())}
    return sorted({0, c['K'] // 2, c['K'] - 1} | planted)


def gpu_decisions(d, kw, max_iter):
    """-> decisions [S][K]: per (track, joint) the list of accepted? per trial the device made."""
    from xas_amd import ops_track
    dec, last = None, None
    for m in range(1, max_iter + 1):
        r = ops_track.track_anchor_smooth(max_iter=m, want=('trials', 'cost'), **d, **kw)
        trials, cost = r['trials'].cpu().numpy(), r['cost'].cpu().numpy()
        if dec is None:
            dec = [[[] for _ in range(trials.shape[1])] for _ in range(trials.shape[0])]
            last = cost[..., 0].copy()
        for s, k in zip(*np.nonzero(trials == m)):
            dec[s][k].append(bool(cost[s, k, 1] < last[s, k]))
        last = cost[..., 1].copy()
    return dec


def compare(c, got, dec, joints, label=''):
    """The (track, joint)s of the case against the oracle made to follow `dec`."""
    out, status, resid = got['xyzw'].cpu().numpy(), got['status'].cpu().numpy(), got['resid'].cpu().numpy()
    ts, cost, trials = got['track_status'].cpu().numpy(), got['cost'].cpu().numpy(), got['trials'].cpu().numpy()
    worst = 0.0
    for s in range(c['S']):
        for k in joints:
            trk, rows = ao.make_track(c, s, k)
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
            n = len(trk.ot) + len(trk.sten) + len(trk.at)
            assert abs(cost[s, k, 0] - b['cost'][0]) <= max(1e-12 * abs(b['cost'][0]), n * EPS * abs(b['cost'][0]))
            assert abs(cost[s, k, 1] - b['cost'][1]) <= 1e-9 * abs(b['cost'][1])
            assert np.allclose(resid[rows, k], b['resid'], rtol=1e-5, equal_nan=True)
    print('anchor smooth %s%s: largest distance / (tolerance + one fp32 ulp) %.3f' % (c['name'], label, worst))


_runs = {}


def run(name):
    """A case, its result on the device: computed once and shared."""
    from xas_amd import ops_track
    if name not in _runs:
        c = ai.planted() if name == 'planted' else ai.make(name)
        d, kw = dev(c), kwargs(c)
        _runs[name] = (c, d, kw, ops_track.track_anchor_smooth(max_iter=c['max_iter'], **d, **kw))
    return _runs[name]


@pytest.mark.parametrize('name', [n for n in ai.CASES if n != 'T1_V1'])
def test_linearise_matches_the_oracle(name):
    from xas_amd import ops_track
    c, d, kw, _ = run(name)
    for lam in (0.0, 1e-3):
        got = ops_track.track_anchor_linearise(lam=lam, **d, **kw)
        band, g, C = got['band'].cpu().numpy(), got['g'].cpu().numpy(), got['C'].cpu().numpy()
        for s in range(c['S']):
            for k in joints_of(c):
                trk, rows = ao.make_track(c, s, k)
                if trk.passed:
                    assert not band[rows, k].any() and not g[rows, k].any() and C[s, k] == 0.0
                    continue
                H, g1 = trk.dense_system(trk.X0, lam)
                b1, (b2, g2) = tk.Track.band_of(H.numpy()), trk.band_system(trk.X0, lam)
                sb, sg = np.abs(b2).max(), np.abs(g2).max()
                tb, tg = max(16 * np.abs(b1 - b2).max() / sb, 64 * EPS), max(16 * np.abs(g1.numpy() - g2).max() / sg, 64 * EPS)
                rb = np.abs(band[rows, k].reshape(-1, 9) - b2).max() / sb
                rg = np.abs(g[rows, k].reshape(-1) - g2).max() / sg
                Cor = trk.cost(trk.X0)[0]
                n = len(trk.ot) + len(trk.sten) + len(trk.at)
                print('anchor linearise %s track %d joint %d lambda %g: band %.2e (bound %.2e)  g %.2e (bound %.2e)  C %.2e (bound %.2e)' % (
                    name, s, k, lam, rb, tb, rg, tg, abs(C[s, k] - Cor) / Cor, n * EPS))
                assert rb <= tb and rg <= tg
                assert abs(C[s, k] - Cor) <= n * EPS * Cor


@pytest.mark.parametrize('name', list(ai.CASES))
def test_smooth_matches_the_oracle(name):
    c, d, kw, got = run(name)
    assert c['max_iter'] <= 12
    compare(c, got, gpu_decisions(d, kw, c['max_iter']), joints_of(c))
    status = got['status'].cpu().numpy()
    assert (got['cost'][..., 1] <= got['cost'][..., 0]).all()
    if name == 'T1_V1':
        assert (status == 2).all() and (got['trials'] == 0).all()
    if name == 'several_V1':                                          # what the case was built to contain
        assert {0, 1, 2} <= set(status.reshape(-1).tolist()) and 2 in set(got['track_status'].reshape(-1).tolist())
    if name == 'T64_V4_anchors_only':                                 # F is empty everywhere: no pixel residual to report
        assert torch.isnan(got['resid']).all() and (status[:, 0] == np.r_[1, 1, np.zeros(62, np.uint8)]).all()


@pytest.mark.parametrize('table,name', [('SMOOTH', n) for n in ti.SMOOTH] + [('LINEARISE', n) for n in ti.LINEARISE])
def test_without_anchors_it_is_track_smooth_bit_for_bit(table, name):
    """NULL anchors and V >= 2: every output of both entry points is xas_track_smooth's / xas_track_linearise's."""
    from xas_amd import ops_track
    c = ti.make(getattr(ti, table), name)
    d = {k: v for k, v in dev(c).items() if k not in ('anchor', 'info')}
    kw = dict(weighted=c['weighted'], huber_px=c['huber'], acc_w=c['acc_w'])
    pairs = [(ops_track.track_smooth(max_iter=c['max_iter'], **d, **kw),
              ops_track.track_anchor_smooth(max_iter=c['max_iter'], anchor_huber=3.0, **d, **kw))]
    pairs += [(ops_track.track_linearise(lam=lam, **d, **kw), ops_track.track_anchor_linearise(lam=lam, **d, **kw)) for lam in (0.0, 1e-3)]
    for want, got in pairs:
        assert set(want) == set(got)
        for k in want:
            assert torch.equal(want[k].view(torch.uint8), got[k].view(torch.uint8)), k


@pytest.mark.parametrize('name', list(ai.CASES))
def test_runs_are_bit_identical_whatever_the_workspace_held(name):
    from xas_amd import ops_track
    from xas_amd._lib import query
    c, d, kw, got = run(name)
    again = ops_track.track_anchor_smooth(max_iter=c['max_iter'], **d, **kw)
    nbytes, pad = query('xas_track_anchor_workspace_bytes', c['N'], c['K']), 256
    buf = torch.full((nbytes + 2 * pad + 16,), 0xFF, dtype=torch.uint8, device=DEV)          # NaN in every double and float
    off = (-buf.data_ptr() - pad) % 16 + pad
    dirty = ops_track.track_anchor_smooth(max_iter=c['max_iter'], workspace=buf[off:off + nbytes], **d, **kw)
    assert (buf[:off] == 0xFF).all() and (buf[off + nbytes:] == 0xFF).all()                   # nothing written outside it
    few = ops_track.track_anchor_smooth(max_iter=c['max_iter'], want=(), **d, **kw)
    assert set(few) == {'xyzw', 'tracks'}
    for k in got:
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), k
        assert torch.equal(got[k].view(torch.uint8), dirty[k].view(torch.uint8)), k
    assert torch.equal(got['xyzw'].view(torch.int32), few['xyzw'].view(torch.int32))
    assert (got['cost'][..., 1] <= got['cost'][..., 0]).all()


def test_planted_monocular_track_is_the_oracles():
    """The planted case of test_track_anchor_abi on the device: closer to the truth than the anchors, and the oracle's result
    within the tolerance on a joint with decoys and on one without."""
    c, d, kw, got = run('planted')
    truth = c['truth'].astype(np.float64)
    smooth_mm = np.linalg.norm(got['xyzw'][..., :3].cpu().numpy().astype(np.float64) - truth, axis=-1)
    anchor_mm = np.linalg.norm(c['anchor'].astype(np.float64) - truth, axis=-1)
    print('planted, one camera, on the device: anchors %.2f mm, smoothed %.2f mm' % (anchor_mm.mean(), smooth_mm.mean()))
    assert (got['status'] == 0).all() and smooth_mm.mean() < anchor_mm.mean()
    compare(c, got, gpu_decisions(d, kw, c['max_iter']), [0, 1], label=' joints 0 (decoys) and 1')
