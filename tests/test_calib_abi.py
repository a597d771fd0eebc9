"""xas_calibrate_* without a GPU: the three symbols are exported, declared and bound with matching argument lists; the ABI
version stays 3; every argument rule answers 1 with its message before any launch; the workspace grows with N.  The oracle's two
formulations (dense over all unknowns, autograd Jacobian; Schur, Jacobian by hand) take the same decisions on every case with
every cost decrease far from a tie, which is what makes the inputs decidable for the GPU tests; and the planted cameras are
recovered by the oracle alone."""
import ctypes

import numpy as np
import pytest

import _calib_inputs as ci
import _calib_oracle as co

NAMES = {'xas_calibrate_workspace_bytes': ('iiii', 'z'),
         'xas_calibrate_linearise': ('ppppp' 'iiiiii' 'f' 'ddd' 'pppp' 'pp', 'i'),
         'xas_calibrate_bundle': ('ppppp' 'iiiiii' 'f' 'dd' 'i' 'ppppppp' 'pp', 'i')}
MIN_MARGIN = 1e-9        # a relative cost decrease below this is a near-tie: 1e6 x the double rounding of a sum of ~1e3 terms
CASE_LIST = [(n, v) for n in ci.CASES for v in (ci.VARIANTS if n == 'typical' else ('plain',))]


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in NAMES.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
    assert len(_lib.fn('xas_calibrate_bundle').argtypes) == 24 and len(_lib.fn('xas_calibrate_linearise').argtypes) == 21
    assert lib.xas_abi_version() == 3


def test_workspace_size_is_monotone_and_aligned():
    from xas_amd import _lib
    ws = _lib.fn('xas_calibrate_workspace_bytes')
    sizes = [ws(N, 4, 18, 2) for N in (1, 2, 15, 64, 4096)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 and s > 0 for s in sizes)
    assert ws(64, 4, 18, 1) <= ws(64, 4, 18, 16)
    for bad in ((0, 4, 18, 1), (4, 1, 18, 1), (4, 7, 18, 1), (4, 4, 0, 1), (4, 4, 18, 0), (4, 4, 18, 17), (1 << 20, 4, 1 << 12, 1)):
        assert ws(*bad) == 0, bad


def test_argument_errors_return_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    bundle, lin = _lib.fn('xas_calibrate_bundle'), _lib.fn('xas_calibrate_linearise')
    one, far = ctypes.c_void_p(64), ctypes.c_void_p(1 << 30)     # aligned non-null pointers: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()

    def call(f=bundle, N=4, V=3, K=5, R=2, start=(0, 3, 4), free=6, flags=0, pr=1.0, pt=1.0, iters=5, lam=0.0, outs=None,
             init=one, workspace=one, **null):
        table = (ctypes.c_int * len(start))(*start)
        head = [None if n in null else (init if n == 'init' else one) for n in ('points', 'P', 'init', 'views')]
        head += [None if 'rig_start' in null else table, N, V, K, R, free, flags, 0.0, pr, pt]
        if f is bundle:
            return f(*head, iters, *(outs or [far] * 7), workspace, None)
        return f(*head, lam, *(outs or [far] * 4), workspace, None)
    for f in (bundle, lin):
        for n in ('points', 'P', 'init', 'rig_start'):
            assert call(f, **{n: None}) == 1 and 'null buffer' in err(), n
        assert call(f, workspace=None) == 1 and 'null buffer' in err()
        assert call(f, V=1) == 1 and 'V=1' in err()
        assert call(f, V=7) == 1 and 'V=7' in err()
        assert call(f, N=0, start=(0, 0, 0)) == 1 and 'bad shape' in err()
        assert call(f, K=0) == 1 and 'bad shape' in err()
        assert call(f, R=0, start=(0,)) == 1 and 'R=0' in err()
        assert call(f, R=17, start=(0,) * 17 + (4,)) == 1 and 'R=17' in err()
        assert call(f, start=(1, 3, 4)) == 1 and 'rig_start runs' in err()
        assert call(f, start=(0, 3, 5)) == 1 and 'rig_start runs' in err()
        assert call(f, start=(0, 5, 4)) == 1 and 'non-decreasing' in err()
        assert call(f, flags=2) == 1 and 'unknown flag bits' in err()
        assert call(f, free=-1) == 1 and 'free_mask' in err()
        assert call(f, pr=-1.0) == 1 and 'priors' in err()
        assert call(f, pt=float('nan')) == 1 and 'priors' in err()
        assert call(f, pr=float('inf')) == 1 and 'priors' in err()
        assert call(f, workspace=ctypes.c_void_p(72)) == 1 and 'aligned' in err()
    assert call(iters=0) == 1 and 'max_iter=0' in err()
    assert call(iters=65) == 1 and 'max_iter=65' in err()
    for i in (0, 1):                                             # delta and out are required, the other five are optional
        assert call(outs=[None if k == i else far for k in range(7)]) == 1 and 'null buffer' in err()
    assert call(init=far) == 1 and 'overlap' in err()
    assert call(init=ctypes.c_void_p((1 << 30) + 16)) == 1 and 'overlap' in err()
    for i in range(4):
        assert call(lin, outs=[None if k == i else far for k in range(4)]) == 1 and 'null buffer' in err()
    assert call(lin, lam=-1.0) == 1 and 'lambda' in err()


def test_header_names_the_tolerances_the_oracle_uses():
    import os
    import re
    from test_abi import ROOT
    src = open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()
    val = lambda n: float(re.search(r'#define %s (\S+)' % n, src).group(1))
    assert val('XAS_CALIB_STEP_TOL_ROT') == co.TOL_ROT and val('XAS_CALIB_STEP_TOL_TRANS') == co.TOL_TRANS
    assert int(val('XAS_CALIB_MAX_RIGS')) == 16


@pytest.mark.parametrize('name,variant', CASE_LIST)
def test_oracle_formulations_agree_and_inputs_are_decidable(name, variant):
    c = ci.make(name, variant)
    planted_fixed = 0
    for r in range(c['R']):
        rig = co.make_rig(c, r)
        planted_fixed += rig.free.size - rig.M
        a, b = rig.lm(rig.step_dense, c['max_iter']), rig.lm(rig.step_schur, c['max_iter'])
        assert a['decisions'] == b['decisions'] and a['status'] == b['status'] == 1
        assert min(a['margins'] + b['margins']) > MIN_MARGIN, (a['margins'], b['margins'])
        assert b['cost'][1] < b['cost'][0] and b['rms'][1] < b['rms'][0]
        dist = formulation_distance(a, b)
        assert dist < 1e-9, dist
        for lam in (0.0, 1e-3):
            S1, b1 = rig.schur_of_dense(rig.delta0, rig.X0, lam)
            S2, b2, _ = rig.schur_system(rig.delta0, rig.X0, lam)
            assert float((S1 - S2).abs().max() / S2.abs().max()) < 1e-12 and float((b1 - b2).abs().max() / b2.abs().max()) < 1e-12
    if c['N'] * c['K'] >= 8:
        assert planted_fixed >= 3            # the NaN start, the joint with one valid view, the start behind a camera


def formulation_distance(a, b):
    """Largest distance between two results relative to the parameter scale: omega against 1 rad, tau and the points against
    the largest |coordinate| of the points (mm)."""
    scale = max(1.0, float(np.abs(b['X']).max())) if b['X'].size else 1.0
    d = max(np.abs(a['delta'][:, :3] - b['delta'][:, :3]).max(), np.abs(a['delta'][:, 3:] - b['delta'][:, 3:]).max() / scale)
    return max(d, np.abs(a['X'] - b['X']).max() / scale) if b['X'].size else d


def test_planted_cameras_are_recovered_by_the_oracle():
    c = ci.planted()
    rig = co.make_rig(c, 0)
    res = rig.lm(rig.step_schur, c['max_iter'])
    assert res['rms'][0] > 0.5 and res['rms'][1] < 1e-3 * res['rms'][0], res['rms']
    truth = c['truth'][c['rig'] == 0][rig.free]
    aligned = co.similarity_align(res['X'], truth)
    assert np.abs(aligned - truth).max() < 0.05, np.abs(aligned - truth).max()          # mm, in a 2 m volume
