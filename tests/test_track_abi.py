"""xas_track_* without a GPU: the three symbols are exported, declared and bound with matching argument lists; every argument
rule answers 1 with its message before any launch; the workspace grows with N and K; ops_track.tracks_of; and the oracle
(tests/_track_oracle.py): its two formulations (dense with an autograd Jacobian; banded by hand) give the same band and gradient
and the same schedule on every case, and the planted effect holds for the oracle alone."""
import ctypes

import numpy as np
import pytest

import _track_inputs as ti
import _track_oracle as tk

NAMES = {'xas_track_smooth_workspace_bytes': ('ii', 'z'),
         'xas_track_linearise': ('pppppp' 'iiiii' 'f' 'dd' 'ppp' 'pp', 'i'),
         'xas_track_smooth': ('pppppp' 'iiiii' 'f' 'd' 'i' 'pppppp' 'pp', 'i')}


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in NAMES.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
    assert len(_lib.fn('xas_track_smooth').argtypes) == 22 and len(_lib.fn('xas_track_linearise').argtypes) == 19
    assert lib.xas_abi_version() == 3


def test_workspace_size_is_monotone_and_aligned():
    from xas_amd import _lib
    ws = _lib.fn('xas_track_smooth_workspace_bytes')
    sizes = [ws(N, 18) for N in (1, 2, 15, 64, 4096)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 and s > 0 for s in sizes)
    assert ws(64, 1) < ws(64, 18)
    for bad in ((0, 18), (4, 0), (-1, 3), (1 << 20, 1 << 12)):
        assert ws(*bad) == 0, bad


def test_argument_errors_return_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    smooth, lin = _lib.fn('xas_track_smooth'), _lib.fn('xas_track_linearise')
    one, far = ctypes.c_void_p(64), ctypes.c_void_p(1 << 30)     # aligned non-null pointers: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()

    def call(f=smooth, N=4, V=3, K=5, S=2, start=(0, 3, 4), flags=0, acc=0.05, iters=5, lam=0.0, outs=None, init=one,
             workspace=one, **null):
        table = (ctypes.c_int * len(start))(*start)
        head = [None if n in null else (init if n == 'init' else one) for n in ('points', 'P', 'init', 'views')]
        head += [None if 'table' in null else table, None if 'frame' in null else one, N, V, K, S, flags, 0.0, acc]
        if f is smooth:
            return f(*head, iters, *(outs or [far] * 6), workspace, None)
        return f(*head, lam, *(outs or [far] * 3), workspace, None)
    for f in (smooth, lin):
        for n in ('points', 'P', 'init', 'table', 'frame'):
            assert call(f, **{n: None}) == 1 and 'null buffer' in err(), n
        assert call(f, workspace=None) == 1 and 'null buffer' in err()
        assert call(f, V=1) == 1 and 'V=1' in err()
        assert call(f, V=7) == 1 and 'V=7' in err()
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
    assert call(init=ctypes.c_void_p((1 << 30) + 16)) == 1 and 'overlap' in err()
    for i in range(3):
        assert call(lin, outs=[None if k == i else far for k in range(3)]) == 1 and 'null buffer' in err()
    assert call(lin, lam=-1.0) == 1 and 'lambda' in err()


def test_tracks_of():
    from xas_amd import ops_track
    h36m = ['images/s_09_act_02_subact_01_ca_01/s_09_act_02_subact_01_ca_01_%06d.jpg' % f for f in (5, 1, 2, 3, 20, 21, 29, 38)]
    other = ['images/s_11_act_02_subact_01_ca_01/s_11_act_02_subact_01_ca_01_%06d.jpg' % f for f in (2, 1)]
    track, frame = ops_track.tracks_of(h36m + other, max_gap=8)
    assert frame.tolist() == [5, 1, 2, 3, 20, 21, 29, 38, 2, 1]
    assert track.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 3, 3]               # 5 -> 20 and 29 -> 38 are more than 8 apart; 21 -> 29 is not
    assert ops_track.tracks_of(h36m, max_gap=100)[0].tolist() == [0] * 8
    track, frame = ops_track.tracks_of(None, count=5)
    assert track.tolist() == [0] * 5 and frame.tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(RuntimeError, match='twice'):
        ops_track.tracks_of(['a/seq_a_000001.jpg', 'a/seq_a_000002.jpg', 'a/seq_a_000001.jpg'])
    with pytest.raises(RuntimeError, match='no frame number'):
        ops_track.tracks_of(['a/image.jpg'])
    assert ops_track.tracks_of(['x/seq_a_000001.jpg', 'x/seq_b_000001.jpg'])[0].tolist() == [0, 1]
    assert ops_track.TRACK_ACC_W == 0.05 and ops_track.TRACK_MAX_GAP == 8 and len(ops_track.STATUS_NAMES) == 3


def formulations(c, s, k):
    trk, rows = tk.make_track(c, s, k)
    return trk, rows, trk.lm(trk.step_dense, c['max_iter']), trk.lm(trk.step_band, c['max_iter'])


@pytest.mark.parametrize('name', list(ti.LINEARISE))
def test_oracle_band_is_its_autograd_matrix(name):
    c = ti.make(ti.LINEARISE, name)
    for k in (0, c['K'] - 1):
        trk, _ = tk.make_track(c, 0, k)
        assert not trk.passed
        for lam in (0.0, 1e-3):
            H, g1 = trk.dense_system(trk.X0, lam)
            band, g2 = trk.band_system(trk.X0, lam)
            dense = tk.Track.band_of(H.numpy())
            assert np.abs(np.tril(H.numpy(), -tk.BW - 1)).max() == 0                 # nothing of H lies outside the band
            assert np.abs(dense - band).max() / np.abs(band).max() < 1e-12
            assert np.abs(g1.numpy() - g2).max() / np.abs(g2).max() < 1e-10
        # the prior's part: half the autograd Hessian of acc_w X^T (A x I3) X is acc_w (A x I3)
        import torch
        prior = lambda x: c['acc_w'] * (trk._accel(x)[1] * (trk._accel(x)[0] ** 2).sum(-1)).sum()
        Hp = 0.5 * torch.autograd.functional.hessian(prior, trk.X0).reshape(3 * trk.T, 3 * trk.T).numpy()
        A = trk.prior_matrix()
        for t in range(trk.T):
            for o in range(3):
                if t - o >= 0:
                    assert abs(Hp[3 * t, 3 * (t - o)] - c['acc_w'] * A[t, o]) <= 1e-12 * max(1.0, abs(Hp).max())


@pytest.mark.parametrize('name', list(ti.SMOOTH))
def test_oracle_formulations_agree(name):
    c = ti.make(ti.SMOOTH, name)
    seen = set()
    for s in range(c['S']):
        for k in range(min(c['K'], 3)):
            trk, rows, a, b = formulations(c, s, k)
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
            else:                                                     # a tie is a cost change below 1e-9 of the cost: both are at the minimum
                assert abs(a['cost'][1] - b['cost'][1]) <= 1e-8 * abs(b['cost'][1])
    if name in ('T1', 'one_data_frame'):
        assert seen == {2}
    if name == 'several':
        assert 2 in seen and len(seen) > 1


def test_planted_effect_holds_for_the_oracle_alone():
    """The chosen seed and acc_w: the smoothed track of the joint with the gap lies closer to the truth than the per-frame
    refinement (_refine_oracle) on its data frames, and the filled frames are near the truth."""
    import _refine_oracle as ro
    c = ti.planted()
    k = 5
    trk, rows = tk.make_track(c, 0, k)
    res = trk.lm(trk.step_band, 30)
    per_frame = ro.refine(c['points'][:, :, k:k + 1], c['P'], c['init'][:, k:k + 1])['xyz'][:, 0]
    truth = c['truth'][:, k].astype(np.float64)
    d = trk.data
    assert int((~d).sum()) == 3
    smooth_mm = np.linalg.norm(res['X'] - truth, axis=-1)
    frame_mm = np.linalg.norm(per_frame - truth, axis=-1)
    print('planted joint %d: per-frame %.3f mm, smoothed %.3f mm on the data frames; filled frames %.3f mm' % (
        k, frame_mm[d].mean(), smooth_mm[d].mean(), smooth_mm[~d].mean()))
    assert smooth_mm[d].mean() < frame_mm[d].mean()
    assert np.isfinite(res['X'][~d]).all() and smooth_mm[~d].max() < 3 * frame_mm[d].mean()
