"""xas_track_skeleton_linearise / xas_track_skeleton_smooth on the device against the float64 oracle
(tests/_track_skeleton_oracle.py) on the cases of tests/_track_skeleton_inputs.py.
Tolerances: the rule of test_gpu_track.py and test_gpu_track_anchor.py.  tol = max(16 x the distance the oracle shows between
its own two formulations on that track, 64 ulps of double), relative to the scale of the quantity: the largest |entry| of the
blocks (of g), the largest |coordinate| of the points.  `out` is fp32, so one fp32 ulp of the value is added there.  C is one
sum of n non-negative terms in another order: n ulps of double bound that.  The trial step d is held to its residual: the
largest |(H + lambda diag H) d + g| of the oracle's by-hand system over the largest |g|, at most 16 x what the oracle's own two
solves leave (or 64 ulps).
The oracle follows the device's accept / reject sequence, read off `trials` and `cost` of calls with 1, 2, .. max_iter trials;
it raises if the device decided otherwise than the oracle at a trial that is no tie.
Measured on an MI355X: profiles/track_skeleton_check.txt."""
import numpy as np
import pytest
import torch

import _track_anchor_oracle as ao
import _track_oracle as tk
import _track_skeleton_inputs as si
import _track_skeleton_oracle as so

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
DEV = 'cuda'


def dev(c):
    t = lambda a, dt=None: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    return dict(points=t(c['points']), pmat=t(c['P']), init=t(c['init']), track=t(c['track'], torch.int64),
                frame=t(c['frame'], torch.int64), views=t(c['views']), anchor=t(c.get('anchor')), info=t(c.get('info')),
                bones=c['bones'], length=t(c['length']))


def kwargs(c):
    return dict(weighted=c['weighted'], huber_px=c['huber'], acc_w=c['acc_w'], anchor_huber=c.get('anchor_huber', 0.0), bone_w=c['bone_w'])


def gpu_decisions(d, kw, max_iter):
    """-> decisions [S]: per track the list of accepted? per trial the device made."""
    from xas_amd import ops_track
    dec, last = None, None
    for m in range(1, max_iter + 1):
        r = ops_track.track_skeleton_smooth(max_iter=m, want=('trials', 'cost'), **d, **kw)
        trials, cost = r['trials'].cpu().numpy(), r['cost'].cpu().numpy()
        if dec is None:
            dec, last = [[] for _ in range(len(trials))], cost[:, 0].copy()
        for s in np.nonzero(trials == m)[0]:
            dec[s].append(bool(cost[s, 1] < last[s]))
        last = cost[:, 1].copy()
    return dec


_runs, _oracle = {}, {}


def case_of(name):
    return si.planted() if name == 'planted' else si.monocular() if name == 'monocular' else si.make(name)


def run(name):
    """A case, its result on the device: computed once and shared."""
    from xas_amd import ops_track
    if name not in _runs:
        c = case_of(name)
        d, kw = dev(c), kwargs(c)
        _runs[name] = (c, d, kw, ops_track.track_skeleton_smooth(max_iter=c['max_iter'], **d, **kw))
    return _runs[name]


def oracle(name):
    """Per track the oracle's two results along the device's decisions: computed once and shared."""
    if name not in _oracle:
        c, d, kw, _ = run(name)
        dec = gpu_decisions(d, kw, c['max_iter'])
        _oracle[name] = []
        for s in range(c['S']):
            trk = so.SkeletonTrack(c, s)
            _oracle[name].append((trk,) + tuple(so.follow(trk, dec[s], c['max_iter'])))
    return _oracle[name]


def compare(name):
    c, _, _, got = run(name)
    out, status, resid, bone = (got[k].cpu().numpy() for k in ('xyzw', 'status', 'resid', 'bone'))
    ts, cost, trials = got['track_status'].cpu().numpy(), got['cost'].cpu().numpy(), got['trials'].cpu().numpy()
    assert np.array_equal(got['length'].cpu().numpy().view(np.uint32), c['length'].view(np.uint32))
    for s, (trk, a, b) in enumerate(oracle(name)):
        rows = trk.rows
        dist, scale = tk.distance(a, b)
        tol = max(16 * dist, 64 * EPS)
        assert not a['ties'] and not b['ties'], (s, a['ties'], b['ties'])      # no trial whose decision the oracle cannot make
        assert int(ts[s]) == b['status'] and int(trials[s]) == b['trials'], (s, ts[s], trials[s], b['status'], b['trials'])
        assert np.array_equal(status[rows], b['frame_status'])
        assert np.array_equal(out[rows][..., 3].view(np.uint32), c['init'][rows][..., 3].view(np.uint32))
        fixed = ~trk.free
        assert np.array_equal(out[rows][:, fixed].view(np.uint32), c['init'][rows][:, fixed].view(np.uint32))     # bit for bit
        assert np.isnan(resid[rows][:, fixed]).all() and cost[s, 1] <= cost[s, 0]
        assert np.array_equal(np.isnan(bone[rows]), np.isnan(b['bone']))
        if not trk.free.any():
            assert cost[s].tolist() == [0.0, 0.0] and trials[s] == 0 and np.isnan(bone[rows]).all()
            continue
        dx = np.abs(out[rows][:, trk.free, :3].astype(np.float64) - b['X'][:, trk.free])
        ulp = np.spacing(np.abs(b['out'][:, trk.free, :3])).astype(np.float64)
        worst = float((dx / (tol * scale + ulp)).max())
        print('skeleton smooth %s track %d: oracle-vs-oracle %.2e, device-vs-oracle %.2e (relative), distance / (tolerance + one fp32 ulp) %.3f'
              % (name, s, dist, float((dx / scale).max()), worst))
        assert (dx <= tol * scale + ulp).all() and np.isfinite(out[rows][:, trk.free, :3]).all()
        assert abs(cost[s, 0] - b['cost'][0]) <= max(1e-12, trk.terms * EPS) * abs(b['cost'][0])
        assert abs(cost[s, 1] - b['cost'][1]) <= 1e-9 * abs(b['cost'][1])
        assert np.allclose(resid[rows], b['resid'], rtol=1e-5, equal_nan=True)
        act = trk.act
        db = np.abs(bone[rows][:, act].astype(np.float64) - b['bone'][:, act])
        assert (db <= 2 * tol * scale + np.spacing(np.abs(b['bone'][:, act]).astype(np.float32))).all()     # two points, one fp32 ulp
    return got


@pytest.mark.parametrize('name', list(si.CASES))
def test_linearise_matches_the_oracle(name):
    from xas_amd import ops_track
    c, d, kw, _ = run(name)
    for lam in (0.0, 1e-3):
        got = ops_track.track_skeleton_linearise(lam=lam, **d, **kw)
        g, hdiag, hoff, dd, C = (got[k].cpu().numpy() for k in ('g', 'hdiag', 'hoff', 'd', 'C'))
        for s in range(c['S']):
            trk = so.SkeletonTrack(c, s)
            rows, T, n = trk.rows, trk.T, trk.n
            Hd, off, g2 = trk.block_system(trk.X0, lam)
            assert np.array_equal(hoff[rows], off) or np.abs(hoff[rows] - off).max() <= 64 * EPS * np.abs(off).max()
            if not trk.free.any():
                assert not g[rows].any() and not hdiag[rows].any() and not dd[rows].any() and C[s] == 0.0
                continue
            ab, g1 = trk.dense_system(trk.X0, lam)
            H1 = np.stack([so.SkeletonTrack.full(ab[:n, t * n:(t + 1) * n]) for t in range(T)])       # the diagonal blocks
            fix = np.repeat(~trk.free, 3)
            Hd[:, fix] = 0.0; Hd[:, :, fix] = 0.0; H1[:, fix] = 0.0; H1[:, :, fix] = 0.0
            sh, sg = np.abs(Hd).max(), np.abs(g2).max()
            th, tg = max(16 * np.abs(H1 - Hd).max() / sh, 64 * EPS), max(16 * np.abs(g1 - g2.reshape(-1)).max() / sg, 64 * EPS)
            rh, rg = np.abs(hdiag[rows] - Hd).max() / sh, np.abs(g[rows].reshape(T, n) - g2).max() / sg
            Cor = trk.cost(trk.X0)[0]
            d_dense, d_block = trk.step_dense(trk.X0, lam), trk.step_block(trk.X0, lam)
            assert d_dense is not None and d_block is not None and np.isfinite(dd[rows]).all()
            r_own = max(trk.residual_of(d_dense.numpy(), lam), trk.residual_of(d_block.numpy(), lam))
            r_dev, bound = trk.residual_of(dd[rows], lam), max(16 * r_own, 64 * EPS)
            print('skeleton linearise %s track %d lambda %g: hdiag %.2e (bound %.2e)  g %.2e (bound %.2e)  C %.2e (bound %.2e)  '
                  'residual of d %.2e (the oracle\'s own %.2e, bound %.2e)' % (name, s, lam, rh, th, rg, tg, abs(C[s] - Cor) / Cor,
                                                                              trk.terms * EPS, r_dev, r_own, bound))
            assert rh <= th and rg <= tg and abs(C[s] - Cor) <= trk.terms * EPS * Cor
            assert r_dev <= bound and not dd[rows][:, ~trk.free].any()


@pytest.mark.parametrize('name', list(si.CASES))
def test_smooth_matches_the_oracle(name):
    c, _, _, got = run(name)
    assert c['max_iter'] <= 8
    compare(name)
    status, ts = got['status'].cpu().numpy(), got['track_status'].cpu().numpy()
    if name == 'T5_K1_no_bones':                                      # n = 3 and Bn = 0 through the whole solver
        assert (status == 0).all() and got['trials'].tolist() == [2] and got['bone'].shape == (5, 0, 2)
        assert float(got['cost'][0, 1]) < float(got['cost'][0, 0])
    if name == 'T1_K1_nothing_free':
        assert (status == 2).all() and ts.tolist() == [2]
    if name == 'several_V4':
        assert ts[0] == 2 and set(ts[1:].tolist()) <= {0, 1} and {0, 1, 2} <= set(status.reshape(-1).tolist())
    if name == 'T65_K18_V1':                                          # what the case was built to contain
        bone = got['bone'].cpu().numpy()
        off = [b for b, (i, j) in enumerate(c['bones']) if 9 in (i, j)] + [2, 4]
        assert (status[:, 9] == 2).all() and np.isnan(bone[:, off]).all() and np.isfinite(np.delete(bone, off, 1)).all()
        assert status[[0, 1, 30, 31, 32, 64], 10].tolist() == [1] * 6 and np.isnan(c['init'][0, 9, :3]).any()


@pytest.mark.parametrize('name', ['T5_K24', 'T65_K18_V1', 'several_V4'])
def test_runs_are_bit_identical_whatever_the_workspace_held(name):
    from xas_amd import ops_track
    from xas_amd._lib import query
    c, d, kw, got = run(name)
    nbytes, pad = query('xas_track_skeleton_workspace_bytes', c['N'], c['K']), 256
    assert nbytes > 0 and nbytes % 16 == 0
    for fill in (0xFF, 0x55):                                         # NaN in every double and float; a finite pattern
        buf = torch.full((nbytes + 2 * pad + 16,), fill, dtype=torch.uint8, device=DEV)
        off = (-buf.data_ptr() - pad) % 16 + pad
        dirty = ops_track.track_skeleton_smooth(max_iter=c['max_iter'], workspace=buf[off:off + nbytes], **d, **kw)
        assert (buf[:off] == fill).all() and (buf[off + nbytes:] == fill).all()                    # nothing written outside it
        for k in got:
            assert torch.equal(got[k].view(torch.uint8), dirty[k].view(torch.uint8)), k
    few = ops_track.track_skeleton_smooth(max_iter=c['max_iter'], want=(), **d, **kw)
    assert set(few) == {'xyzw', 'tracks', 'length'} and torch.equal(got['xyzw'].view(torch.int32), few['xyzw'].view(torch.int32))


def test_planted_rigid_track_is_the_oracles():
    """T = 130, K = 18, V = 4, rigid bones, 2 px of noise, the wrist unseen for three frames: the device gives the oracle's
    result, and the forearm over the filled frames stays within what the oracle leaves of its length error."""
    c, _, _, got = run('planted')
    compare('planted')
    trk, a, b = oracle('planted')[0]
    X = got['xyzw'][..., :3].cpu().numpy().astype(np.float64)
    fore = int(np.nonzero((c['bones'] == (si.WRIST, si.ELBOW)).all(1))[0][0])
    err = lambda Y: np.abs(np.linalg.norm(Y[c['gap'], si.WRIST] - Y[c['gap'], si.ELBOW], axis=-1) - c['true_length'][fore]).max()
    bone = got['bone'].cpu().numpy().astype(np.float64)
    rms = np.sqrt(np.nanmean(bone ** 2, axis=(0, 1)))
    mm = np.linalg.norm(X - c['truth'].astype(np.float64), axis=-1).mean()
    print('planted on the device: bone-length RMS %.3f -> %.3f mm, %.3f mm from the truth, forearm error over the filled frames %.3f mm '
          '(the oracle: %.3f mm)' % (rms[0], rms[1], mm, err(X), err(b['X'])))
    assert rms[1] < rms[0]
    assert err(X) <= err(b['X']) + 16 * max(tk.distance(a, b)[0], 4 * EPS) * tk.distance(a, b)[1] + 2 * np.spacing(np.float32(np.abs(X).max()))


def test_monocular_track_is_the_oracles():
    """One camera, K = 18, ray anchors, a tenth of the frames of every third joint on a decoy down the ray."""
    compare('monocular')
