"""xas_smpl_fit without a GPU: the three symbols are exported, declared and bound with matching argument lists; the workspace
grows with B and V; every argument error answers with status 1 and a message before any launch; B == 0 is valid.  The oracle's
own Jacobian agrees with central differences, the committed cases are what the generator says, and a fit-output file written
from the oracle's results loads as a PseudoSynth bank."""
import ctypes
import os

import numpy as np
import torch

import _smplfit_cases as sc
import _smplfit_inputs as si
import _smplfit_oracle as so

NAMES = {'xas_smpl_fit_workspace_bytes': ('ii', 'z'),
         'xas_smpl_fit_linearise': ('p' * 14 + 'ffiii' + 'pppp', 'i'),
         'xas_smpl_fit': ('p' * 14 + 'ffiiii' + 'p' * 9, 'i')}


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib, ops_smplfit
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in NAMES.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
    assert len(_lib.fn('xas_smpl_fit').argtypes) == 29 and len(_lib.fn('xas_smpl_fit_linearise').argtypes) == 23
    assert ops_smplfit.STATUS_NAMES == ('converged', 'iteration limit', 'passed through')


def test_workspace_size_is_monotone():
    from xas_amd import _lib
    ws = _lib.fn('xas_smpl_fit_workspace_bytes')
    assert ws(-1, 10) == 0 and ws(2, 0) == 0
    sizes = [[ws(B, V) for V in (1, 70, 300, 6890)] for B in (1, 3, 32)]
    assert ws(0, 70) == ws(0, 6890) < ws(1, 1)
    for row in sizes:
        assert all(a < b for a, b in zip(row, row[1:])) and all(v % 16 == 0 for v in row)
    for lo, hi in zip(sizes, sizes[1:]):
        assert all(a < b for a, b in zip(lo, hi))
    assert ws(32, 6890) >= 32 * (79 * 288 + 15 * 6890 + 3655) * 8


def test_argument_errors_return_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    fit, lin = _lib.fn('xas_smpl_fit'), _lib.fn('xas_smpl_fit_linearise')
    one = ctypes.c_void_p(64)                      # aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    names = ('pose', 'betas', 'trans', 'v_template', 'shapedirs', 'posedirs', 'j_regressor', 'weights', 'parents', 'h36m_regressor',
             'reg_verts', 'reg_count', 'targets', 'joint_w')

    def call(f=fit, B=2, V=70, center=0, iters=5, wp=1.0, ws=1.0, outs=None, workspace=one, **null):
        head = [None if n in null else one for n in names]
        if f is fit:
            return f(*head, wp, ws, B, V, center, iters, *(outs or [one] * 7), workspace, None)
        return f(*head, wp, ws, B, V, center, *(outs or [one] * 2), workspace, None)
    for f in (fit, lin):
        assert call(f, B=-1) == 1 and 'B=-1' in err()
        assert call(f, V=0) == 1 and 'V=0' in err()
        assert call(f, center=24) == 1 and 'center_idx=24' in err()
        assert call(f, center=-2) == 1 and 'center_idx=-2' in err()
        assert call(f, wp=-1.0) == 1 and 'priors' in err()
        assert call(f, ws=float('nan')) == 1 and 'priors' in err()
        for n in names:
            if n not in ('reg_verts', 'reg_count'):
                assert call(f, **{n: None}) == 1 and 'null buffer' in err(), n
        assert call(f, reg_verts=None) == 1 and 'come together' in err()
        assert call(f, reg_count=None) == 1 and 'come together' in err()
        assert call(f, workspace=None) == 1 and 'null buffer' in err()
        n_out = 7 if f is fit else 2
        for i in range(n_out):
            assert call(f, outs=[None if k == i else one for k in range(n_out)]) == 1 and 'null output' in err()
        # B == 0 is valid and touches nothing, the null pointers included
        assert call(f, B=0, outs=[None] * n_out, workspace=None, **{n: None for n in names}) == 0
    assert call(iters=-1) == 1 and 'max_iters=-1' in err()
    assert call(iters=201) == 1 and 'max_iters=201' in err()


def test_oracle_jacobian_agrees_with_central_differences():
    m = so.model_arrays(si.arrays(70))
    x = torch.as_tensor(si.random_params(1, 5)[0])
    w = torch.ones(18, dtype=torch.float64)
    w[3] = 0
    tgt = so.joints(x, m) + 5.0
    tgt[3] = float('nan')
    r, J = so.linearise(x, m, tgt, w, 100.0, 25.0)
    assert torch.isfinite(J).all() and (J[9:12] == 0).all() and (r[9:12] == 0).all()
    Jn = torch.zeros_like(J)
    for i in range(85):
        h = 1e-6 * max(1.0, abs(float(x[i])))
        e = torch.zeros(85, dtype=torch.float64)
        e[i] = h
        Jn[:, i] = (so.residual(x + e, m, tgt, w, 100.0, 25.0) - so.residual(x - e, m, tgt, w, 100.0, 25.0)) / (2 * h)
    assert float((J - Jn).abs().max()) <= 1e-8 * float(J.abs().max())
    # the root's exponential map has its derivative at omega = 0 (the generators)
    x0 = x.clone()
    x0[:3] = 0
    _, J0 = so.linearise(x0, m, tgt, w, 100.0, 25.0)
    assert float(J0[:54, :3].abs().max()) > 1.0


def test_committed_cases_are_the_generators():
    c = sc.load()
    assert len(c['index']) >= 8 and (c['gap2'] < sc.KEEP_GAP).all() and (c['iters'] <= sc.MAX_ITERS - sc.MARGIN).all()
    planted = sc.candidates()[c['index']]
    assert np.array_equal(planted, c['planted'])
    assert float(np.abs(planted[:, 6:75]).max()) <= 0.4 and float(np.abs(planted[:, 75:]).min()) > 0
    m = so.model_arrays(si.arrays(sc.V, sc.REG, sc.SEED))
    i = 0                                                                 # one case end to end; the file holds the rest
    tgt = so.joints(torch.as_tensor(planted[i]), m).float()
    assert np.array_equal(tgt.numpy(), c['targets'][i])
    w = torch.ones(18, dtype=torch.float64)
    x0 = so.kabsch_init(m, tgt.double(), w)
    assert float((x0 - torch.as_tensor(c['x0'][i])).abs().max()) <= 1e-3
    fit = so.lm(torch.as_tensor(c['x0'][i]), m, tgt.double(), w, sc.POSE_PRIOR, sc.SHAPE_PRIOR, sc.MAX_ITERS)
    assert fit['status'] == 0 and fit['iters'] == int(c['iters'][i])
    assert float((fit['x'] - torch.as_tensor(c['x'][i])).abs().max()) <= 1e-9 * float(np.abs(c['x'][i]).max())


def test_oracle_fit_file_loads_as_a_pseudo_bank(tmp_path):
    from xas_amd.pseudo import PseudoSynth
    c = sc.load()
    x = c['x'].astype(np.float32)
    path = os.path.join(str(tmp_path), 'fit.npz')
    np.savez(path, pose=np.concatenate([x[:, :3], x[:, 6:75]], 1), betas=x[:, 75:], trans=x[:, 3:6], cost=c['cost'].astype(np.float32),
             status=np.zeros(len(x), np.uint8), joint_rms_mm=np.zeros(len(x), np.float32))
    synth = PseudoSynth(path, object(), object())
    assert tuple(synth.pose.shape) == (len(x), 72) and tuple(synth.betas.shape) == (len(x), 10)
    R = synth.root
    m_R = torch.stack([so.expmap(torch.as_tensor(r[:3], dtype=torch.float64)) for r in x])
    assert float((R - m_R).abs().max()) <= 1e-12                          # the fit's omega is PseudoSynth's root rotation
