"""xas_track_skeleton_* without a GPU: the three symbols are exported, declared and bound with matching argument lists; every
argument rule answers 1 with its message before any launch; the workspace query; ops_track.bones_of and track_bone_lengths
against numpy; and the oracle (tests/_track_skeleton_oracle.py): its two formulations give the same system and take the same
decisions, none of them a near-tie, on every case, and the planted effect holds for the oracle alone."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _track_anchor_oracle as ao
import _track_oracle as tk
import _track_skeleton_inputs as si
import _track_skeleton_oracle as so

NAMES = {'xas_track_skeleton_workspace_bytes': ('ii', 'z'),
         'xas_track_skeleton_linearise': ('pppppppppp' 'iiiiii' 'f' 'dddd' 'ppppp' 'pp', 'i'),
         'xas_track_skeleton_smooth': ('pppppppppp' 'iiiiii' 'f' 'ddd' 'i' 'ppppppp' 'pp', 'i')}


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in NAMES.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
    assert len(_lib.fn('xas_track_skeleton_smooth').argtypes) == 30 and len(_lib.fn('xas_track_skeleton_linearise').argtypes) == 28
    assert lib.xas_abi_version() == 3


def test_workspace_size_is_monotone_and_aligned():
    from xas_amd import _lib
    ws = _lib.fn('xas_track_skeleton_workspace_bytes')
    sizes = [ws(N, 18) for N in (1, 2, 15, 64, 4096)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 and s > 0 for s in sizes)
    assert ws(64, 1) < ws(64, 18) < ws(64, 24)
    per_frame = (ws(4096 + 4, 18) - ws(4096, 18)) // 4 - 4            # less the entry of `start`
    assert per_frame == 74328 == 8 * (3 * 54 * 54 + 10 * 54 + 3)      # the figure of the header and the README
    assert ws((1 << 31) // 24, 24) > 0                                # N*K just under 2^31
    for bad in ((0, 18), (4, 0), (-1, 3), (4, 25), (1 << 20, 1 << 12), ((1 << 31) // 24 + 1, 24), (1 << 27, 18)):
        assert ws(*bad) == 0, bad


def test_argument_errors_return_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    smooth, lin = _lib.fn('xas_track_skeleton_smooth'), _lib.fn('xas_track_skeleton_linearise')
    one, far = ctypes.c_void_p(64), ctypes.c_void_p(1 << 30)     # aligned non-null pointers: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()

    def call(f=smooth, N=4, V=1, K=5, S=2, start=(0, 3, 4), flags=0, ah=3.0, acc=0.05, bw=0.1, iters=5, lam=0.0, outs=None, init=one,
             workspace=one, anchor=one, info=one, bones=((1, 0), (2, 1)), Bn=None, length=one, **null):
        table = (ctypes.c_int * len(start))(*start)
        flat = [j for b in bones for j in b]
        host = None if 'host' in null else (ctypes.c_int * max(len(flat), 1))(*flat)
        head = [None if n in null else (init if n == 'init' else one) for n in ('points', 'P', 'init', 'views')]
        head += [anchor, info, host, length, None if 'table' in null else table, None if 'frame' in null else one, N, V, K, S,
                 len(bones) if Bn is None else Bn, flags, 0.0, ah, acc, bw]
        if f is smooth:
            return f(*head, iters, *(outs or [far] * 7), workspace, None)
        return f(*head, lam, *(outs or [far] * 5), workspace, None)
    for f in (smooth, lin):
        who = 'track_skeleton_smooth' if f is smooth else 'track_skeleton_linearise'
        for n in ('points', 'P', 'init', 'table', 'frame'):
            assert call(f, **{n: None}) == 1 and 'null buffer' in err() and who in err(), n
        assert call(f, workspace=None) == 1 and 'null buffer' in err()
        assert call(f, V=0) == 1 and 'V=0' in err()
        assert call(f, V=7) == 1 and 'V=7' in err()
        assert call(f, anchor=None) == 1 and 'anchor and info come together' in err()
        assert call(f, ah=-1.0) == 1 and 'anchor_huber' in err()
        assert call(f, N=0, start=(0, 0, 0)) == 1 and 'bad shape' in err()
        assert call(f, K=0) == 1 and 'K=0' in err()
        assert call(f, K=25) == 1 and 'K=25' in err() and 'XAS_SKEL_MAX_JOINTS' in err()
        assert call(f, Bn=-1) == 1 and 'Bn=-1' in err()
        assert call(f, Bn=33) == 1 and 'Bn=33' in err() and 'XAS_TRACK_MAX_BONES' in err()
        assert call(f, host=None) == 1 and 'null bones or length' in err()
        assert call(f, length=None) == 1 and 'null bones or length' in err()
        assert call(f, bones=((1, 0), (5, 1))) == 1 and 'bones[1] = (5, 1)' in err()
        assert call(f, bones=((1, 0), (2, -1))) == 1 and 'bones[1] = (2, -1)' in err()
        assert call(f, bones=((1, 0), (3, 3))) == 1 and 'joins joint 3 to itself' in err()
        for bad in (-1.0, float('nan'), float('inf')):
            assert call(f, bw=bad) == 1 and 'bone_w' in err()
            assert call(f, acc=bad) == 1 and 'acc_w' in err()
        assert call(f, S=0, start=(0,)) == 1 and 'S=0' in err()
        assert call(f, S=5, start=(0, 1, 2, 3, 4, 4)) == 1 and 'S=5' in err()
        assert call(f, start=(1, 3, 4)) == 1 and 'start runs' in err()
        assert call(f, S=3, start=(0, 2, 2, 4)) == 1 and 'increasing' in err()          # an empty track
        assert call(f, flags=2) == 1 and 'unknown flag bits' in err()
        assert call(f, workspace=ctypes.c_void_p(72)) == 1 and 'aligned' in err()
    assert call(iters=0) == 1 and 'max_iter=0' in err()
    assert call(iters=65) == 1 and 'max_iter=65' in err()
    assert call(outs=[None] + [far] * 6) == 1 and 'null buffer' in err()         # out is required, the other six are optional
    assert call(init=far) == 1 and 'overlap' in err()
    for i in range(5):
        assert call(lin, outs=[None if k == i else far for k in range(5)]) == 1 and 'null buffer' in err()
    assert call(lin, lam=-1.0) == 1 and 'lambda' in err()


def test_a_workspace_that_is_too_small_is_refused_before_the_call():
    from xas_amd import _lib, ops_track
    c = si.make('T3_K3_chain')
    t = lambda a, dt=None: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt)
    need = _lib.query('xas_track_skeleton_workspace_bytes', c['N'], c['K'])
    for f in (ops_track.track_skeleton_smooth, ops_track.track_skeleton_linearise):
        with pytest.raises(RuntimeError, match='workspace must be a contiguous uint8 tensor of at least %d bytes' % need):
            f(t(c['points']), t(c['P']), t(c['init']), t(c['track'], torch.int64), t(c['frame'], torch.int64), c['bones'],
              length=t(c['length']), workspace=torch.empty(need - 1, dtype=torch.uint8))


def test_bones_of_the_shipped_configs():
    from xas_amd import ops_track
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'configs.json')) as f:
        configs = json.load(f)
    seen = 0
    for cfg in (configs.values() if isinstance(configs, dict) else configs):
        parents = cfg['model_params']['parent_ids']
        bones = ops_track.bones_of(parents)
        assert bones.shape == (len(parents) - 1, 2) and bones.dtype == np.int32
        assert all(parents[k] == p != k for k, p in bones)
        assert np.array_equal(bones, si.bones_of(parents))
        seen += 1
    assert seen and ops_track.bones_of([-1, 0, 2]).tolist() == [[1, 0]]
    assert ops_track.TRACK_BONE_W == 0.1 and ops_track.TRACK_MAX_BONES == 32


def test_bone_lengths_are_the_numpy_median():
    from xas_amd import ops_track
    c = si.make('T65_K18_V1')
    init = c['init'].copy()
    got = ops_track.track_bone_lengths(torch.as_tensor(init), c['track'], c['frame'], c['bones'])
    want = si.median_lengths(init, c['track'], c['bones'])
    assert got.shape == (1, 17) and got.dtype == torch.float32 and np.isnan(init).any()
    assert np.allclose(got.numpy(), want, rtol=1e-6, atol=0, equal_nan=True)
    init[:, 9, 0] = np.nan                                            # no frame qualifies: NaN
    got = ops_track.track_bone_lengths(torch.as_tensor(init), c['track'], c['frame'], c['bones']).numpy()
    off = [b for b, (i, j) in enumerate(c['bones']) if 9 in (i, j)]
    assert np.isnan(got[0, off]).all() and np.isfinite(np.delete(got, off, 1)).all()
    c = si.make('several_V4')                                         # several tracks, odd and even counts, any order
    perm = np.random.default_rng(3).permutation(c['N'])
    usable = np.random.default_rng(4).random((c['N'], c['K'])) < 0.7
    got = ops_track.track_bone_lengths(torch.as_tensor(c['init'][perm]), c['track'][perm], c['frame'][perm], c['bones'],
                                       usable=torch.as_tensor(usable[perm])).numpy()
    masked = np.where(usable[..., None], c['init'][..., :3], np.nan)
    assert np.allclose(got, si.median_lengths(masked, c['track'], c['bones']), rtol=1e-6, atol=0, equal_nan=True)


@pytest.mark.parametrize('name', list(si.CASES) + ['planted', 'monocular'])
def test_oracle_formulations_agree_and_no_trial_is_a_near_tie(name):
    """What makes the cases decidable on the device: both formulations take the same decision at every trial, and every
    relative change of the cost is above tk.TIE_MARGIN.  Every case the GPU tests compare, the two large ones included."""
    c = si.planted() if name == 'planted' else si.monocular() if name == 'monocular' else si.make(name)
    for s in range(c['S']):
        trk = so.SkeletonTrack(c, s)
        if trk.free.any():
            for lam in (0.0, 1e-3):
                ab, g1 = trk.dense_system(trk.X0, lam)
                Hd, hoff, g2 = trk.block_system(trk.X0, lam)
                n, T = trk.n, trk.T
                H1 = np.stack([so.SkeletonTrack.full(ab[:n, t * n:(t + 1) * n]) for t in range(T)])
                assert np.abs(H1 - Hd).max() <= 1e-12 * np.abs(Hd).max() and np.abs(g1 - g2.reshape(-1)).max() <= 1e-10 * np.abs(g2).max()
                for o, col in ((n, 0), (2 * n, 1)):                   # the two off-diagonal blocks: a scalar on the free joints
                    if T * n > o:
                        want = np.repeat(hoff[o // n:, col], n) * np.tile(np.repeat(trk.free, 3), T - o // n)
                        assert np.abs(ab[o, :T * n - o] - want).max() <= 1e-12 * max(np.abs(hoff).max(), 1e-300)
        a, b = trk.lm(trk.step_dense, c['max_iter']), trk.lm(trk.step_block, c['max_iter'])
        assert a['decisions'] == b['decisions'] and a['status'] == b['status'] and a['trials'] == b['trials']
        assert not a['ties'] and not b['ties'] and all(m >= tk.TIE_MARGIN for m in a['margins'] + b['margins'])
        assert b['cost'][1] <= b['cost'][0] and tk.distance(a, b)[0] < 1e-9
        if not trk.free.any():
            assert a['status'] == 2 and np.array_equal(b['out'].view(np.uint32), c['init'][trk.rows].view(np.uint32))


def test_cases_contain_what_they_were_built_for():
    c = si.make('T65_K18_V1')
    trk = so.SkeletonTrack(c, 0)
    off = [b for b, (i, j) in enumerate(c['bones']) if 9 in (i, j)] + [2, 4]
    assert not trk.free[9] and trk.free.sum() == 17 and sorted(np.nonzero(~trk.act)[0]) == sorted(off)
    assert list(np.nonzero(~trk.data[:, 10])[0]) == [0, 1, 30, 31, 32, 64] and trk.data[:, 11].all()
    c = si.make('T130_K3_1e4')
    trk = so.SkeletonTrack(c, 0)
    _, ln = trk.bone_e(trk.X0)
    assert float(ln[40, 0]) == 0.0 and np.isfinite(trk.block_system(trk.X0, 0.0)[0]).all()      # coincident: a zero row, finite
    assert np.abs(c['init'][np.isfinite(c['init'])]).max() > 8e3
    c = si.make('several_V4')
    assert [so.SkeletonTrack(c, s).T for s in range(3)] == [1, 2, 130] and not so.SkeletonTrack(c, 0).free.any()
    assert len(set(np.diff(c['frame'][c['track'] == 2]))) > 1                                   # non-uniform frame numbers


def test_planted_effect_holds_for_the_oracle_alone():
    """130 frames, K = 18, V = 4, rigid bones, 2 px of noise, the wrist unseen for three frames: with the bones the bone-length
    RMS falls and the tracks lie no further from the truth than the per-joint smoother's with the same acc_w."""
    c = si.planted()
    truth = c['truth'].astype(np.float64)
    trk = so.SkeletonTrack(c, 0)
    r = trk.lm(trk.step_block, 30)
    each = np.stack([(lambda t: t.lm(t.step_band, 30)['X'])(ao.make_track(c, 0, k)[0]) for k in range(c['K'])], 1)
    rms = lambda e: float(np.sqrt(np.nanmean(e ** 2)))
    fore = int(np.nonzero((c['bones'] == (si.WRIST, si.ELBOW)).all(1))[0][0])
    arm = lambda X: np.abs(np.linalg.norm(X[c['gap'], si.WRIST] - X[c['gap'], si.ELBOW], axis=-1) - c['true_length'][fore]).max()
    mm = lambda X: float(np.linalg.norm(X - truth, axis=-1).mean())
    print('planted, oracle alone: bone-length RMS %.3f -> %.3f mm (per-joint smoother %.3f mm); from the truth: start %.3f, per-joint '
          '%.3f, with bones %.3f mm; forearm error over the filled frames: per-joint %.3f, with bones %.3f mm' % (
              rms(r['bone'][..., 0]), rms(r['bone'][..., 1]), rms(trk.bone_all(each)), mm(trk.X0.numpy()), mm(each), mm(r['X']),
              arm(each), arm(r['X'])))
    assert r['cost'][1] < r['cost'][0]
    assert rms(r['bone'][..., 1]) < rms(r['bone'][..., 0])
    assert mm(r['X']) <= mm(each)
