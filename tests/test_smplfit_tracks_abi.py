"""xas_smpl_fit_tracks without a GPU: the three symbols are exported, declared and bound with matching argument lists and the
ABI version stays 3; the workspace grows with N while its vertex-sized part does not; every argument error answers with status 1
and a message before any launch; the oracle's two solves agree; and no trial of any GPU-test case decides on a cost change under
1e-9 relative (the condition of the skeleton smoother's tests for comparable accept/reject decisions)."""
import ctypes

import numpy as np
import pytest
import torch

import _smplfit_tracks_cases as tc
import _smplfit_tracks_oracle as to

NAMES = {'xas_smpl_fit_tracks_workspace_bytes': ('iii', 'z'),
         'xas_smpl_fit_tracks_linearise': ('p' * 16 + 'ffiiiid' + 'p' * 7, 'i'),
         'xas_smpl_fit_tracks': ('p' * 16 + 'ffiiiii' + 'p' * 11, 'i')}


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib, ops_smplfit
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in NAMES.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
    assert lib.xas_abi_version() == 3 == _lib.ABI_VERSION
    assert ops_smplfit.TRACK_STATUS_NAMES == ('converged', 'trial limit', 'no usable frame')
    assert callable(ops_smplfit.fit_smpl_tracks) and callable(ops_smplfit.linearise_smpl_tracks)


def test_workspace_grows_with_the_frames_not_with_their_vertices():
    from xas_amd import _lib
    ws = _lib.fn('xas_smpl_fit_tracks_workspace_bytes')
    assert ws(-1, 10, 1) == 0 and ws(2, 0, 1) == 0 and ws(2, 10, -1) == 0
    sizes = [ws(N, 6890, 8) for N in (0, 1, 2, 100, 511, 512, 513, 2048, 100000)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(v % 16 == 0 for v in sizes)
    assert ws(8, 70, 3) < ws(8, 70, 4) and ws(8, 70, 3) < ws(8, 300, 3)
    # the vertex-sized part belongs to the workgroups of a bounded grid: once the grid is full it does not grow with N
    part = lambda N: ws(N, 6890, 8) - ws(N, 2, 8)
    assert part(512) == part(2048) == part(100000) and part(1) * 512 == part(512)
    per_frame = (ws(100000, 6890, 8) - ws(2048, 6890, 8)) / (100000 - 2048)
    assert 61936 <= per_frame <= 61936 + 16                                         # the README's bytes per frame (and four ints)
    assert ws(2048, 6890, 8) < 2048 * 8 * (79 * 288 + 15 * 6890)                     # under what xas_smpl_fit takes for as many samples


def test_argument_errors_return_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    fit, lin = _lib.fn('xas_smpl_fit_tracks'), _lib.fn('xas_smpl_fit_tracks_linearise')
    one = ctypes.c_void_p(64)                      # aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    names = ('pose', 'betas', 'trans', 'v_template', 'shapedirs', 'posedirs', 'j_regressor', 'weights', 'parents', 'h36m_regressor',
             'reg_verts', 'reg_count', 'targets', 'joint_w', 'track', 'frame')

    def call(f=fit, N=2, V=70, S=2, center=0, iters=5, lam=1e-3, wp=1.0, ws=1.0, outs=None, workspace=one, track_ids=None, **null):
        head = [None if n in null else one for n in names]
        if track_ids is not None:
            head[14] = ctypes.cast(track_ids, ctypes.c_void_p)
        if f is fit:
            return f(*head, wp, ws, N, V, S, center, iters, *(outs or [one] * 9), workspace, None)
        return f(*head, wp, ws, N, V, S, center, lam, *(outs or [one] * 5), workspace, None)
    for f in (fit, lin):
        assert call(f, N=-1) == 1 and 'B=-1' in err()
        assert call(f, V=0) == 1 and 'V=0' in err()
        assert call(f, S=-1) == 1 and 'S=-1' in err()
        assert call(f, center=24) == 1 and 'center_idx=24' in err()
        assert call(f, wp=-1.0) == 1 and 'priors' in err()
        for n in names:
            if n not in ('reg_verts', 'reg_count'):
                assert call(f, **{n: None}) == 1 and 'null buffer' in err(), n
        assert call(f, reg_verts=None) == 1 and 'come together' in err()
        assert call(f, workspace=None) == 1 and 'null buffer' in err()
        n_out = 9 if f is fit else 5
        for i in range(n_out):
            assert call(f, outs=[None if k == i else one for k in range(n_out)]) == 1 and 'null output' in err()
        # a track id outside [0, S) in memory the host can read
        for bad in (-1, 2):
            ids = (ctypes.c_int * 2)(0, bad)
            assert call(f, track_ids=ids) == 1 and 'track[1] = %d' % bad in err()
        # nothing to do is valid and touches nothing, the null pointers included
        assert call(f, N=0, S=0, outs=[None] * n_out, workspace=None, **{n: None for n in names}) == 0
    assert call(iters=-1) == 1 and 'max_iters=-1' in err()
    assert call(iters=201) == 1 and 'max_iters=201' in err()
    assert call(lin, lam=-1.0) == 1 and 'lambda' in err()
    assert call(lin, lam=float('nan')) == 1 and 'lambda' in err()


def test_oracles_two_solves_agree():
    _, rows, trk = tc.tracks_of_case(tc.build('mixed_V70', extras=True))[0]
    assert trk.T == 3 and trk.usable.count(False) == 1
    H, g = trk.normal(trk.y0, trk.beta0)
    for lam in (0.0, 1e-3, 10.0):
        dense, sch = to.solve_dense(H, g, lam), to.solve_schur(H, g, lam, trk.T)
        A, b = to.reduced_by_lu(H, g, lam, trk.T)
        assert to.rel(sch['d'], dense) <= 1e-10 and to.rel(A, sch['reduced']) <= 1e-10 and to.rel(b, sch['rhs']) <= 1e-10
        assert to.residual_of(H, g, lam, dense) <= 1e-10
    # the gradient of the summed cost is J^T r of the full Jacobian
    y, beta = trk.y0.clone().requires_grad_(True), trk.beta0.clone().requires_grad_(True)
    C = sum((to.residual(trk.point(y, beta, i), trk.m, trk.tgt[t], trk.w[t], trk.wp, trk.ws) ** 2).sum() for i, t in enumerate(trk.rows))
    C.backward()
    grad = torch.cat([y.grad.reshape(-1), beta.grad])
    assert to.rel(grad, 2 * g) <= 1e-10


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_no_trial_decides_on_a_rounding_difference(name):
    for s, rows, trk, r in tc.oracle_fit(name):
        assert r['status'] == 1 and r['trials'] == tc.FIT_ITERS                       # stops before it converges
        assert r['margin'] >= 1e-9, 'track %d: a trial changes C by %.2e relative' % (s, r['margin'])
        assert r['cost'][1] <= r['cost'][0]


def test_committed_planted_sequence():
    z, p = tc.load_planted(), tc.planted_inputs()
    assert float(z['margin']) >= 1e-9 and z['x'].shape == (tc.PLANTED['T'], 85)
    assert (z['x'][:, 75:] == z['x'][0, 75:]).all()
    fig = tc.planted_figures(z['x'][0, 75:], z['joints'], z['frames_x'][:, 75:], z['frames_joints'], p)
    assert fig[0] < fig[1] and fig[2] <= fig[3]
    # the stored result is a point of the committed inputs: its joints are the model's
    _, m = tc.model(tc.PLANTED['V'])
    assert float((tc.so.joints(torch.as_tensor(z['x'][3]), m) - torch.as_tensor(z['joints'][3])).abs().max()) <= 1e-9
