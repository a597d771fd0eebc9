"""xas_smpl_fit_views without a GPU: the three symbols are exported, declared and bound with matching argument lists; the
workspace is xas_smpl_fit's; every argument error answers with status 1 and a message before any launch; B == 0 is valid.  The
oracle's two assemblies agree, its rules for which observations count give what the cases planted, and its LM never increases
the cost."""
import ctypes

import numpy as np
import pytest

import _smplfit_views_cases as vc
import _smplfit_views_oracle as vo

HEAD = 'p' * 17 + 'i' + 'dd' + 'ff'
NAMES = {'xas_smpl_fit_views_workspace_bytes': ('ii', 'z'),
         'xas_smpl_fit_views_linearise': (HEAD + 'iiii' + 'p' * 7, 'i'),
         'xas_smpl_fit_views': (HEAD + 'iiiii' + 'p' * 10, 'i')}


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib, ops_smplfit
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in NAMES.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
    assert len(_lib.fn('xas_smpl_fit_views').argtypes) == 37 and len(_lib.fn('xas_smpl_fit_views_linearise').argtypes) == 33
    assert ops_smplfit.VIEWS_POSE_PRIOR == 0.1 * ops_smplfit.POSE_PRIOR and ops_smplfit.VIEWS_SHAPE_PRIOR == 0.1 * ops_smplfit.SHAPE_PRIOR
    assert (vc.WP, vc.WS) == (ops_smplfit.VIEWS_POSE_PRIOR, ops_smplfit.VIEWS_SHAPE_PRIOR) and ops_smplfit.USED_ANCHOR == vo.ANCHOR_BIT


def test_workspace_is_the_joint_fits():
    from xas_amd import _lib
    ws, base = _lib.fn('xas_smpl_fit_views_workspace_bytes'), _lib.fn('xas_smpl_fit_workspace_bytes')
    assert ws(-1, 10) == 0 and ws(2, 0) == 0
    for B in (0, 1, 3, 32):
        for V in (1, 70, 513, 6890):
            assert ws(B, V) == base(B, V) and ws(B, V) % 16 == 0


def test_argument_errors_return_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    fit, lin = _lib.fn('xas_smpl_fit_views'), _lib.fn('xas_smpl_fit_views_linearise')
    one = ctypes.c_void_p(64)                      # aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    names = ('pose', 'betas', 'trans', 'v_template', 'shapedirs', 'posedirs', 'j_regressor', 'weights', 'parents', 'h36m_regressor',
             'reg_verts', 'reg_count', 'points', 'P', 'views', 'anchor', 'info')

    def call(f=fit, B=2, V=70, C=2, center=0, iters=5, flags=0, huber=0.0, ah=3.0, wp=1.0, ws=1.0, outs=None, workspace=one, **null):
        head = [None if n in null else one for n in names]
        n_out = 8 if f is fit else 5
        tail = [B, V, C, center] + ([iters] if f is fit else []) + list(outs or [one] * n_out)
        return f(*head, flags, huber, ah, wp, ws, *tail, workspace, None)
    for f in (fit, lin):
        assert call(f, B=-1) == 1 and 'B=-1' in err()
        assert call(f, V=0) == 1 and 'V=0' in err()
        assert call(f, center=24) == 1 and 'center_idx=24' in err()
        assert call(f, center=-2) == 1 and 'center_idx=-2' in err()
        assert call(f, wp=-1.0) == 1 and 'priors' in err()
        assert call(f, ws=float('nan')) == 1 and 'priors' in err()
        for n in names:
            if n not in ('reg_verts', 'reg_count', 'views', 'anchor', 'info'):
                assert call(f, **{n: None}) == 1 and 'null buffer' in err(), n
        assert call(f, reg_verts=None) == 1 and 'come together' in err()
        assert call(f, reg_count=None) == 1 and 'come together' in err()
        assert call(f, anchor=None) == 1 and 'anchor and info come together' in err()
        assert call(f, info=None) == 1 and 'anchor and info come together' in err()
        assert call(f, workspace=None) == 1 and 'null buffer' in err()
        assert call(f, C=0) == 1 and 'V=0 views' in err()
        assert call(f, C=7) == 1 and 'XAS_TRI_MAX_VIEWS' in err()
        assert call(f, flags=2) == 1 and 'unknown flag bits' in err()
        assert call(f, huber=-1.0) == 1 and 'huber' in err() and 'anchor_huber' not in err()
        assert call(f, huber=float('inf')) == 1 and 'huber' in err()
        assert call(f, ah=-1.0) == 1 and 'anchor_huber' in err()
        assert call(f, ah=float('nan')) == 1 and 'anchor_huber' in err()
        n_out = 8 if f is fit else 5
        for i in range(n_out):
            assert call(f, outs=[None if k == i else one for k in range(n_out)]) == 1 and 'null output' in err()
        # B == 0 is valid and touches nothing, the null pointers included
        assert call(f, B=0, outs=[None] * n_out, workspace=None, **{n: None for n in names}) == 0
    assert call(iters=-1) == 1 and 'max_iters=-1' in err()
    assert call(iters=201) == 1 and 'max_iters=201' in err()


def test_host_wrapper_needs_a_start():
    import torch
    from xas_amd import ops_smplfit
    with pytest.raises(RuntimeError, match='init is required'):
        ops_smplfit.fit_smpl_views(torch.zeros(1, 1, 18, 3), torch.zeros(1, 1, 3, 4), None, None, None)


def test_cases_plant_what_their_names_say():
    s = vc.oracle_samples('one_camera_ray_V70')
    assert s[1].used[2] == 0x01 and s[1].used[5] == 0x01 and s[1].used[7] == 0 and s[2].used[9] == 0x80 and s[0].used.tolist() == [0x81] * 18
    c = vc.build('one_camera_ray_V70')
    rank = [np.linalg.matrix_rank(vo.tao.sym(c['info'][0, k].astype(np.float64)), tol=1e-9) for k in range(18)]
    assert rank == [1] * 18                                                         # ray_information's matrices
    s = vc.oracle_samples('two_cameras_huber_V70')
    assert s[0].used[1] == 1 and s[0].used[8] == 2 and s[1].used[4] == 2 and s[0].used[10] == 3 and s[1].used[13] == 0
    v, k = vc.build('six_cameras_behind_V70')['behind'][0]
    s = vc.oracle_samples('six_cameras_behind_V70')
    assert vc.build('six_cameras_behind_V70')['points'][0, v, k, 2] > 0 and not (s[0].used[k] >> v) & 1
    assert sum(int((u >> v) & 1) for u in s[0].used) == 3                           # the close-up's other joints stay
    assert float(np.abs(vc.build('six_cameras_behind_V70')['x0'][1, 3:6]).min()) > 8e3
    s = vc.oracle_samples('passed_V70')
    assert s[0].n_used == 5 and s[0].passed() and s[1].passed() and not s[2].passed()
    s = vc.oracle_samples('four_cameras_full_V513')
    assert s[0].used[3] == 0x0f and s[1].used.tolist() == [0x8b] * 18


@pytest.mark.parametrize('name', sorted(vc.CASES))
def test_oracle_assemblies_agree_and_lm_descends(name):
    tails = 0
    for s in vc.oracle_samples(name):
        if s.passed():
            r = s.lm(vc.FIT_ITERS)
            assert r['status'] == 2 and r['iters'] == 0 and r['cost'][0] == r['cost'][1] or not np.isfinite(r['cost'][0])
            continue
        H, g = s.normal_rows(s.x0)
        Hb, gb = s.normal_blocks(s.x0)
        assert vo.rel(Hb, H) <= 1e-12 and vo.rel(gb, g) <= 1e-11
        C, front = s.cost(s.x0)
        assert front and abs(float(s.blocks(s.x0)[2].sum()) + sum(s.wp * float(t) ** 2 for t in s.x0[6:75])
                             + sum(s.ws * float(t) ** 2 for t in s.x0[75:]) - C) <= 1e-10 * C
        w, psi = s.weights(s.x0)
        tails += int((w < (s.os * s.os) * (1 - 1e-12)).sum()) + int((psi < 1).sum())
        r = s.lm(vc.FIT_ITERS)
        assert r['cost'][1] <= r['cost'][0] and r['iters'] == vc.FIT_ITERS and r['status'] == 1
        kept = [c for c, a in zip(r['costs'], r['accepts']) if a]
        assert all(b < a for a, b in zip([r['cost'][0]] + kept, kept)) and any(r['accepts'])
    c = vc.build(name)
    if c['huber'] > 0 or (c['anchor_huber'] > 0 and c['anchor'] is not None):
        assert tails >= 2                                                           # some terms lie on Huber's linear part


def test_planted_golden_is_the_generators():
    z, q, p = vc.load_planted(), vc.planted_inputs(), vc.PLANTED
    for k in ('x0', 'points', 'P', 'anchor', 'info', 'clean', 'decoy'):
        assert np.array_equal(z[k], q[k], equal_nan=True), k
    assert z['points'].shape == (p['N'], 1, 18, 3) and p['N'] == 12 and int(z['decoy'].sum()) == round(0.1 * 12 * 18)
    centre = vc.tai.centres(z['P'])[:, 0]
    ray = z['anchor'].astype(np.float64) - centre[:, None]
    truth = z['clean'] - centre[:, None]
    down = np.linalg.norm(ray, axis=-1) - np.linalg.norm(truth, axis=-1)
    assert (down[z['decoy']] > 250 - 5 * 30).all() and (down[z['decoy']] < 600 + 5 * 30).all() and 20 < down[~z['decoy']].std() < 40
    px = np.linalg.norm(vc.project(z['P'][0].astype(np.float64), z['clean'][0])[0] - z['points'][0, 0, :, :2], axis=-1)
    assert 0.5 < px.mean() < 6.0
    assert np.array_equal(z['warm'], z['joints_x'].astype(np.float32).astype(np.float64)) and float(z['margin'].min()) >= 1e-9
    fig = vc.planted_figures(z['joints_joints'], z['views_joints'], z['clean'])
    assert fig == tuple(z['figures']) and fig[1] < fig[0]                           # the pixel fit is the closer one
    # one sample end to end: the golden is what the oracle gives today
    b, m = 4, vc.model(p['V'])[1]
    s = vo.Sample(m, z['warm'][b], z['points'][b], z['P'][b], None, z['anchor'][b], z['info'][b], False, 0.0, p['anchor_huber'], *p['views_priors'], 0)
    r = s.lm(p['iters'])
    assert r['iters'] == int(z['views_iters'][b]) and vo.rel(r['x'], z['views_x'][b]) <= 1e-9
