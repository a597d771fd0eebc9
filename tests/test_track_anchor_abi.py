"""xas_track_anchor_* without a GPU: the three symbols are exported, declared and bound with matching argument lists; every
argument rule answers 1 with its message before any launch; the workspace query; ops_track.ray_information and
covariance_information against numpy; and the oracle (tests/_track_anchor_oracle.py): its two formulations give the same band,
gradient and schedule on every case, its anchor blocks are half its autograd Hessian, and the planted monocular effect holds
for the oracle alone."""
import ctypes

import numpy as np
import pytest
import torch

import _track_anchor_inputs as ai
import _track_anchor_oracle as ao
import _track_oracle as tk

NAMES = {'xas_track_anchor_workspace_bytes': ('ii', 'z'),
         'xas_track_anchor_linearise': ('pppppppp' 'iiiii' 'f' 'ddd' 'ppp' 'pp', 'i'),
         'xas_track_anchor_smooth': ('pppppppp' 'iiiii' 'f' 'dd' 'i' 'pppppp' 'pp', 'i')}


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in NAMES.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
    assert len(_lib.fn('xas_track_anchor_smooth').argtypes) == 25 and len(_lib.fn('xas_track_anchor_linearise').argtypes) == 22
    assert lib.xas_abi_version() == 3


def test_workspace_size_is_monotone_and_aligned():
    from xas_amd import _lib
    ws = _lib.fn('xas_track_anchor_workspace_bytes')
    sizes = [ws(N, 18) for N in (1, 2, 15, 64, 4096)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 and s > 0 for s in sizes)
    assert ws(64, 1) < ws(64, 18)
    assert ws(64, 18) == _lib.fn('xas_track_smooth_workspace_bytes')(64, 18)          # the record is the shared one
    for bad in ((0, 18), (4, 0), (-1, 3), (1 << 20, 1 << 12)):
        assert ws(*bad) == 0, bad


def test_argument_errors_return_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    smooth, lin = _lib.fn('xas_track_anchor_smooth'), _lib.fn('xas_track_anchor_linearise')
    one, far = ctypes.c_void_p(64), ctypes.c_void_p(1 << 30)     # aligned non-null pointers: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()

    def call(f=smooth, N=4, V=1, K=5, S=2, start=(0, 3, 4), flags=0, ah=3.0, acc=0.05, iters=5, lam=0.0, outs=None, init=one,
             workspace=one, anchor=one, info=one, **null):
        table = (ctypes.c_int * len(start))(*start)
        head = [None if n in null else (init if n == 'init' else one) for n in ('points', 'P', 'init', 'views')]
        head += [anchor, info, None if 'table' in null else table, None if 'frame' in null else one, N, V, K, S, flags, 0.0, ah, acc]
        if f is smooth:
            return f(*head, iters, *(outs or [far] * 6), workspace, None)
        return f(*head, lam, *(outs or [far] * 3), workspace, None)
    for f in (smooth, lin):
        who = 'track_anchor_smooth' if f is smooth else 'track_anchor_linearise'
        for n in ('points', 'P', 'init', 'table', 'frame'):
            assert call(f, **{n: None}) == 1 and 'null buffer' in err() and who in err(), n
        assert call(f, workspace=None) == 1 and 'null buffer' in err()
        assert call(f, V=0) == 1 and 'V=0' in err()
        assert call(f, V=7) == 1 and 'V=7' in err()
        assert call(f, anchor=None) == 1 and 'anchor and info come together' in err()
        assert call(f, info=None) == 1 and 'anchor and info come together' in err()
        assert call(f, ah=-1.0) == 1 and 'anchor_huber' in err()
        assert call(f, ah=float('nan')) == 1 and 'anchor_huber' in err()
        assert call(f, ah=float('inf')) == 1 and 'anchor_huber' in err()
        assert call(f, N=0, start=(0, 0, 0)) == 1 and 'bad shape' in err()
        assert call(f, K=0) == 1 and 'bad shape' in err()
        assert call(f, S=0, start=(0,)) == 1 and 'S=0' in err()
        assert call(f, S=5, start=(0, 1, 2, 3, 4, 4)) == 1 and 'S=5' in err()
        assert call(f, start=(1, 3, 4)) == 1 and 'start runs' in err()
        assert call(f, start=(0, 3, 5)) == 1 and 'start runs' in err()
        assert call(f, S=3, start=(0, 3, 2, 4)) == 1 and 'increasing' in err()
        assert call(f, S=3, start=(0, 2, 2, 4)) == 1 and 'increasing' in err()          # an empty track
        assert call(f, flags=2) == 1 and 'unknown flag bits' in err()
        assert call(f, acc=-1.0) == 1 and 'acc_w' in err()
        assert call(f, acc=float('nan')) == 1 and 'acc_w' in err()
        assert call(f, acc=float('inf')) == 1 and 'acc_w' in err()
        assert call(f, workspace=ctypes.c_void_p(72)) == 1 and 'aligned' in err()
    assert call(iters=0) == 1 and 'max_iter=0' in err()
    assert call(iters=65) == 1 and 'max_iter=65' in err()
    assert call(outs=[None] + [far] * 5) == 1 and 'null buffer' in err()         # out is required, the other five are optional
    assert call(init=far) == 1 and 'overlap' in err()
    for i in range(3):
        assert call(lin, outs=[None if k == i else far for k in range(3)]) == 1 and 'null buffer' in err()
    assert call(lin, lam=-1.0) == 1 and 'lambda' in err()


def test_information_matrices_match_numpy():
    from xas_amd import ops_track
    assert ops_track.TRACK_DEPTH_W == 4e-4 and ops_track.TRACK_ANCHOR_HUBER == 3.0
    c = ai.make('T4_V1_gaps')
    got = ops_track.ray_information(torch.as_tensor(c['P'][:, 0]), torch.as_tensor(c['anchor']), 4e-4).numpy()
    want = ai.ray_info(c['P'][:, 0], c['anchor'], 4e-4)
    bad = ~np.isfinite(c['anchor']).all(-1)
    assert got.shape == (4, 3, 6) and got.dtype == np.float32 and bad.any()
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()
    assert np.allclose(got[~bad], want[~bad], rtol=1e-6, atol=0)
    W = ao.sym(got[~bad].astype(np.float64))
    assert np.allclose(np.trace(W, axis1=-2, axis2=-1), 4e-4, rtol=1e-6)                         # depth_w |r|^2
    assert np.abs(np.linalg.eigvalsh(W)[:, :2]).max() < 1e-10                                   # rank one
    rng = np.random.default_rng(5)
    Q = np.linalg.qr(rng.normal(size=(6, 2, 3, 3)))[0]
    cov = np.einsum('nkij,nkj,nklj->nkil', Q, rng.uniform(25.0, 900.0, (6, 2, 3)), Q).astype(np.float32)
    cov[0, 0, 1, 1] = np.nan
    cov[1, 1] = -cov[1, 1]                                                                       # not positive definite
    cov[2, 0] = 0.0
    info = ops_track.covariance_information(torch.as_tensor(cov)).numpy()
    ok = np.ones((6, 2), bool)
    ok[0, 0] = ok[1, 1] = ok[2, 0] = False
    assert info.shape == (6, 2, 6) and np.isnan(info[~ok]).all()
    inv = np.linalg.inv(cov[ok].astype(np.float64))
    assert np.allclose(info[ok], inv[:, ai.TRI[0], ai.TRI[1]], rtol=1e-5, atol=0)


@pytest.mark.parametrize('name', list(ai.CASES))
def test_oracle_band_is_its_autograd_matrix(name):
    c = ai.make(name)
    for s in range(c['S']):
        for k in sorted({0, c['K'] - 1}):
            trk, _ = ao.make_track(c, s, k)
            if trk.passed:
                continue
            for lam in (0.0, 1e-3):
                H, g1 = trk.dense_system(trk.X0, lam)
                band, g2 = trk.band_system(trk.X0, lam)
                dense = tk.Track.band_of(H.numpy())
                assert np.abs(np.tril(H.numpy(), -tk.BW - 1)).max() == 0
                assert np.abs(dense - band).max() / np.abs(band).max() < 1e-12
                assert np.abs(g1.numpy() - g2).max() <= 1e-10 * max(np.abs(g2).max(), 1e-300)


@pytest.mark.parametrize('name', ['T2_V2', 'T63_V1_decoys', 'T64_V4_anchors_only'])
def test_anchor_blocks_are_half_the_autograd_hessian(name):
    """Huber inactive on the anchor term (delta 0): the by-hand blocks psi W are half the Hessian of the anchor cost itself."""
    c = ai.make(name)
    trk, _ = ao.make_track(c, 0, 0, anchor_huber=0.0)
    X = trk.X0 + 3.0                                            # away from the anchors: e is not 0
    n = 3 * trk.T
    Ha = 0.5 * torch.autograd.functional.hessian(trk.anchor_cost, X).reshape(n, n).numpy()
    with_a, _ = trk.band_system(X, 0.0)
    trk.at = trk.at[:0]; trk.A = trk.A[:0]; trk.W = trk.W[:0]     # the same track without its anchor term
    without, _ = trk.band_system(X, 0.0)
    assert np.abs(Ha).max() > 0
    assert np.abs(tk.Track.band_of(Ha) - (with_a - without)).max() <= 1e-12 * np.abs(Ha).max()


@pytest.mark.parametrize('name', list(ai.CASES))
def test_oracle_formulations_agree(name):
    c = ai.make(name)
    seen = set()
    for s in range(c['S']):
        for k in sorted({0, 1, 2, c['K'] // 2, c['K'] - 1} & set(range(c['K']))):
            trk, rows = ao.make_track(c, s, k)
            a, b = trk.lm(trk.step_dense, c['max_iter']), trk.lm(trk.step_band, c['max_iter'])
            seen.add(a['status'])
            if trk.passed:
                assert a['status'] == b['status'] == 2 and a['trials'] == b['trials'] == 0
                assert np.array_equal(b['out'].view(np.uint32), c['init'][rows][:, k].view(np.uint32))
                continue
            assert b['cost'][1] <= b['cost'][0] and a['cost'][1] <= a['cost'][0]
            ties = a['ties'] + b['ties']                              # from the first tie on the two may part: the GPU tests follow
            upto = min(ties) if ties else min(len(a['decisions']), len(b['decisions']))
            assert a['decisions'][:upto] == b['decisions'][:upto]
            if not ties:
                assert a['status'] == b['status'] and a['trials'] == b['trials'] and tk.distance(a, b)[0] < 1e-9
            else:
                assert abs(a['cost'][1] - b['cost'][1]) <= 1e-8 * abs(b['cost'][1])
    if name == 'T1_V1':
        assert seen == {2}
    if name == 'several_V1':
        assert 2 in seen and len(seen) > 1


def test_cases_contain_what_they_were_built_for():
    """The frame rules of the header, read off the oracle's classification."""
    trk, _ = ao.make_track(ai.make('T65_V1_K18'), 0, 4)
    assert trk.data.all() and np.isnan(trk.init[[0, 33], :3]).all() and np.isfinite(trk.X0.numpy()).all()   # init NaN: starts at the anchor
    trk, _ = ao.make_track(ai.make('T65_V1_K18'), 0, 9)
    assert not trk.data[[10, 11, 64]].any() and trk.data.sum() == 62                   # zero trace: not usable, one view: a gap
    c = ai.make('T130_V2_1e4')
    trk, _ = ao.make_track(c, 0, 1)
    assert trk.data[50] and trk.nused[50] == 0 and trk.nused[49] == 2                  # behind a view: the anchor term alone
    trk, _ = ao.make_track(c, 0, 2)
    assert trk.data[70] and not trk.usable[70] and not trk.data[90]                    # data by its views; neither: a gap
    assert np.abs(c['anchor'][np.isfinite(c['anchor'])]).min() > 8e3
    trk, _ = ao.make_track(ai.make('T64_V4_anchors_only'), 0, 2)
    assert trk.nused.sum() == 0 and list(np.nonzero(~trk.data)[0]) == [20, 21, 40]
    c = ai.make('T63_V1_decoys')
    trk, _ = ao.make_track(c, 0, 0)
    _, psi, _ = trk._anchor(torch.as_tensor(c['truth'][:, 0].astype(np.float64)))
    assert trk.ah == 3.0 and (trk.nused == 1).all() and len(trk.at) == 63
    assert list(np.nonzero(psi.numpy() < 1)[0]) == [5, 30, 31, 62]                       # Huber active on the decoys alone


def test_planted_monocular_effect_holds_for_the_oracle_alone():
    """130 frames, K = 18, one camera, 2 px and 30 mm of noise, a tenth of the frames of every third joint on a decoy 250-600 mm
    along the ray: the smoothed tracks lie closer to the truth than the anchors, and closer with anchor_huber = 3 than with 0."""
    c = ai.planted()
    truth = c['truth'].astype(np.float64)
    mm = {}
    for ah in (3.0, 0.0):
        X = np.stack([(lambda t: t.lm(t.step_band, 30)['X'])(ao.make_track(c, 0, k, anchor_huber=ah)[0]) for k in range(c['K'])], 1)
        mm[ah] = np.linalg.norm(X - truth, axis=-1)
    anchors = np.linalg.norm(c['anchor'].astype(np.float64) - truth, axis=-1)
    dj = c['decoys'].any(0)
    print('planted, one camera: anchors %.2f mm, smoothed %.2f mm with anchor_huber 3, %.2f mm with 0; joints with decoys alone: '
          '%.2f, %.2f, %.2f mm' % (anchors.mean(), mm[3.0].mean(), mm[0.0].mean(), anchors[:, dj].mean(), mm[3.0][:, dj].mean(),
                                   mm[0.0][:, dj].mean()))
    assert c['decoys'].sum() == 6 * 13
    assert mm[3.0].mean() < anchors.mean() and mm[0.0].mean() < anchors.mean()
    assert mm[3.0].mean() < mm[0.0].mean()
