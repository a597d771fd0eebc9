"""xas_smpl_fit_tracks_smooth without a GPU: the three symbols are exported, declared and bound with matching argument lists and
the ABI version stays 3; the workspace is a multiple of 16 and grows with N; every argument error answers with status 1 and a
message before any launch; the oracle's dense solve and its block recurrence agree on every case; the unwrapped start is the
rotation of the raw one, and the planted start does wrap; no trial of any fit case decides on a cost change under 1e-9 relative
(the margin rule of tests/test_smplfit_tracks_abi.py: comparable accept/reject decisions); and, on the oracle alone, the committed
planted sequence is smoother and nearer the noise-free joints with the prior than without."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _smplfit_smooth_cases as sc
import _smplfit_smooth_oracle as sm
import _smplfit_tracks_oracle as to

NAMES = {'xas_smpl_fit_tracks_smooth_workspace_bytes': ('iii', 'z'),
         'xas_smpl_fit_tracks_smooth_linearise': ('p' * 16 + 'ffddiiiid' + 'p' * 11, 'i'),
         'xas_smpl_fit_tracks_smooth': ('p' * 16 + 'ffddiiiii' + 'p' * 11, 'i')}


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib, ops_smplfit
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in NAMES.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
    assert lib.xas_abi_version() == 3 == _lib.ABI_VERSION
    for f in ('fit_smpl_tracks_smooth', 'linearise_smpl_tracks_smooth', 'tracks_smooth_workspace_bytes'):
        assert callable(getattr(ops_smplfit, f))


def test_workspace_is_aligned_and_grows_with_the_frames():
    from xas_amd import _lib
    ws, old = _lib.fn('xas_smpl_fit_tracks_smooth_workspace_bytes'), _lib.fn('xas_smpl_fit_tracks_workspace_bytes')
    assert ws(-1, 10, 1) == 0 and ws(2, 0, 1) == 0 and ws(2, 10, -1) == 0
    sizes = [ws(N, 6890, 8) for N in (0, 1, 2, 100, 511, 512, 513, 2048, 100000)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(v % 16 == 0 for v in sizes)
    per_frame = (ws(100000, 6890, 8) - ws(2048, 6890, 8)) / (100000 - 2048)
    assert 160368 <= per_frame <= 160368 + 16                                       # the header's bytes per frame (and four ints)
    assert ws(2048, 6890, 8) - old(2048, 6890, 8) == 2048 * 98432                   # the factor's block rows


def test_argument_errors_return_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    fit, lin = _lib.fn('xas_smpl_fit_tracks_smooth'), _lib.fn('xas_smpl_fit_tracks_smooth_linearise')
    one = ctypes.c_void_p(64)                      # aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    names = ('pose', 'betas', 'trans', 'v_template', 'shapedirs', 'posedirs', 'j_regressor', 'weights', 'parents', 'h36m_regressor',
             'reg_verts', 'reg_count', 'targets', 'joint_w', 'track', 'frame')

    def call(f=fit, N=2, V=70, S=2, center=0, iters=5, lam=1e-3, wp=1.0, ws=1.0, rot=1e4, tr=1.0, outs=None, workspace=one, **null):
        head = [None if n in null else one for n in names]
        return f(*head, wp, ws, rot, tr, N, V, S, center, iters if f is fit else lam, *(outs or [one] * 9), workspace, None)
    for f in (fit, lin):
        for bad in (-1.0, float('nan'), float('inf')):
            assert call(f, rot=bad) == 1 and 'weights' in err()
            assert call(f, tr=bad) == 1 and 'weights' in err()
        assert call(f, N=-1) == 1 and 'B=-1' in err()
        assert call(f, S=-1) == 1 and 'S=-1' in err()
        assert call(f, wp=-1.0) == 1 and 'priors' in err()
        for n in names:
            if n not in ('reg_verts', 'reg_count'):
                assert call(f, **{n: None}) == 1 and 'null buffer' in err(), n
        assert call(f, workspace=None) == 1 and 'null buffer' in err()
        for i in range(9):
            assert call(f, outs=[None if k == i else one for k in range(9)]) == 1 and 'null output' in err()
        assert call(f, N=0, S=0, outs=[None] * 9, workspace=None, **{n: None for n in names}) == 0
    assert call(iters=-1) == 1 and 'max_iters=-1' in err()
    assert call(iters=201) == 1 and 'max_iters=201' in err()
    assert call(lin, lam=-1.0) == 1 and 'lambda' in err()


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_oracles_two_solves_agree(name):
    for s, rows, trk in sc.tracks_of_case(sc.build(name)):
        if trk.T == 0:
            continue
        H, g = trk.normal(trk.y0, trk.beta0)
        for lam in (1e-3, 10.0):
            dense, blk = to.solve_dense(H, g, lam), sm.solve_block(H, g, lam, trk.T)
            assert to.rel(blk, dense) <= 1e-10 and to.residual_of(H, g, lam, blk) <= 1e-10
        # the gradient of the whole cost is J^T r of the full Jacobian, prior included
        y, beta = trk.y0.clone().requires_grad_(True), trk.beta0.clone().requires_grad_(True)
        C = sum((to.residual(trk.point(y, beta, i), trk.m, trk.tgt[t], trk.w[t], trk.wp, trk.ws) ** 2).sum() for i, t in enumerate(trk.rows))
        if trk.temporal:
            C = C + (trk.prior_residual(y) ** 2).sum()
        C.backward()
        assert to.rel(torch.cat([y.grad.reshape(-1), beta.grad]), 2 * g) <= 1e-10


def test_cases_hold_what_they_are_for():
    mixed = sc.tracks_of_case(sc.build('mixed_V70'))
    assert [trk.T for _, _, trk in mixed] == [3, 4, 5, 7, 1, 2, 0]
    assert [trk.usable.count(False) for _, _, trk in mixed] == [0, 1, 1, 0, 0, 0, 2]
    assert mixed[1][2].usable.index(False) == 2 and mixed[2][2].usable.index(False) == 2       # in the middle of their tracks
    assert sorted(set(np.diff(mixed[3][2].f).tolist())) == [1, 2, 3]
    # both weights 0: the repeated frame stays
    assert [trk.T for _, _, trk in sc.tracks_of_case(sc.build('mixed_V70'), 0.0, 0.0)][2] == 6
    assert sc.CASES['rot_only_V70'][3:5] == (sc.ROT, 0.0) and sc.CASES['trans_only_V70'][3:5] == (0.0, sc.TRANS)
    assert sc.CASES['zero_V70'][3:5] == (0.0, 0.0) and sc.CASES['two_pass_V513'][0] == 513


def test_unwrapped_start_is_the_same_rotation_and_the_planted_start_wraps():
    trk = sc.tracks_of_case(sc.build('wrap_V70'))[0][2]
    raw, un = trk.raw_y0[:, :3], trk.y0[:, :3]
    assert float((raw[1:] - raw[:-1]).norm(dim=1).max()) > math.pi                 # two consecutive raw inits lie further apart than pi
    assert float((un[1:] - un[:-1]).norm(dim=1).max()) < 1.0 and not torch.equal(raw, un)
    for a, b in zip(raw, un):
        assert float((sm.rotation(a) - sm.rotation(b)).abs().max()) <= 1e-14
    assert torch.equal(trk.raw_y0[:, 3:], trk.y0[:, 3:])                           # the body pose is not unwrapped
    # rot_w = 0: nothing is unwrapped
    c = sc.build('wrap_V70')
    off = sc.tracks_of_case(c, 0.0, 1.0)[0][2]
    assert torch.equal(off.raw_y0, off.y0)


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_no_trial_decides_on_a_rounding_difference(name):
    for s, rows, trk, r in sc.oracle_fit(name):
        if trk.T == 0:
            assert r['status'] == 2 and r['trials'] == 0
            continue
        assert r['status'] == 1 and r['trials'] == sc.FIT_ITERS                       # stops before it converges
        assert r['margin'] >= 1e-9, 'track %d: a trial changes C by %.2e relative' % (s, r['margin'])
        assert r['cost'][1] <= r['cost'][0]


def test_committed_planted_sequence():
    z, p = sc.load_planted(), sc.planted_inputs()
    T = sc.PLANTED['T']
    assert float(z['margin']) >= 1e-9 and float(z['track_margin']) >= 1e-9 and z['x'].shape == (T, 85) == z['track_x'].shape
    assert (z['x'][:, 75:] == z['x'][0, 75:]).all()
    near, near0, acc, acc0 = sc.planted_figures(z['joints'], z['track_joints'], p)
    assert near < near0 and acc < acc0                                              # nearer the noise-free joints, and smoother
    # the stored results are points of the committed inputs: their joints are the model's
    _, m = sc.model(sc.PLANTED['V'])
    for x, J in ((z['x'], z['joints']), (z['track_x'], z['track_joints'])):
        assert float((sc.so.joints(torch.as_tensor(x[3]), m) - torch.as_tensor(J[3])).abs().max()) <= 1e-9
