"""eval.py --calibrate / --calibration (model_params.calibrate / calibration): the flags and their model_params keys without a
GPU; on the GPU modules.util.apply_calibration and ops_calib.rigs_of, and on the planted evaluation batch of
tests/test_gpu_tri_robust.py with one camera bumped, what --calibrate adds (a file, one line per rig, nothing else moves) and
that --calibration of that file lowers the triangulation's error."""
import os
import subprocess
import sys
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

import _calib_inputs as ci
from test_eval_fit_cli import PlantedDetector, _cfg

FLAGS = ['--calibrate', '--calibration', '--calib-iters', '--calib-prior-rot', '--calib-prior-trans', '--calib-free']


def _parse(argv):
    import eval as xeval
    parser = ArgumentParser()
    for flag, kw in xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT + xeval.CLI_CALIB:
        parser.add_argument(flag, **kw)
    return xeval, parser.parse_args(['--config', 'c.yaml'] + argv)


def test_flags_and_their_config_keys():
    xeval, opt = _parse([])
    flags = dict(xeval.CLI_CALIB)
    assert list(flags) == FLAGS
    assert not set(flags) & (set(dict(xeval.CLI)) | set(dict(xeval.CLI_VOLUME)) | set(dict(xeval.CLI_FIT)))
    assert opt.calibrate is None and opt.calibration is None and opt.calib_iters == 30
    assert opt.calib_prior_rot is None and opt.calib_prior_trans is None and opt.calib_free is None
    cfg = {'model_params': {}}
    xeval.mirror_calib_options(cfg, opt)
    assert cfg['model_params'] == {'calibrate': None, 'calibration': None, 'calib_iters': 30}
    xeval, opt = _parse(['--calibrate', 'out/c.npz', '--calib-iters', '12', '--calib-prior-rot', '7.5', '--calib-prior-trans', '0.5',
                         '--calib-free', '6'])
    xeval.mirror_calib_options(cfg, opt)
    assert cfg['model_params'] == {'calibrate': 'out/c.npz', 'calibration': None, 'calib_iters': 12, 'calib_prior_rot': 7.5,
                                   'calib_prior_trans': 0.5, 'calib_free': 6}


def test_the_two_flags_together_and_several_ranks_are_errors(monkeypatch):
    xeval, opt = _parse(['--calibrate', 'a.npz', '--calibration', 'b.npz'])
    with pytest.raises(ValueError, match='do not go together'):
        xeval.mirror_calib_options({'model_params': {}}, opt)
    with pytest.raises(ValueError, match='do not go together'):
        xeval.Eval(_cfg([0, 1], calibrate='a.npz', calibration='b.npz'), torch.nn.Identity(), [], 'log')
    with pytest.raises(ValueError, match='calibrate needs 2 to'):
        xeval.Eval(_cfg([0], calibrate='a.npz'), torch.nn.Identity(), [], 'log')
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='WORLD_SIZE == 1'):
        xeval.Eval(_cfg([0, 1], calibrate='a.npz'), torch.nn.Identity(), [], 'log')


def test_the_calibration_module_is_not_imported_without_the_flags():
    import eval as xeval
    pkg = os.path.dirname(os.path.abspath(xeval.__file__))
    code = "import sys; sys.path[:0] = %r; import eval; print('xas_amd.ops_calib' in sys.modules)" % ([pkg, os.path.dirname(pkg)],)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == 'False', r.stderr[-2000:]


def test_correction_matrix_is_the_oracles():
    import _calib_oracle as co
    from modules.util import correction_matrix
    d = torch.tensor([[0.0] * 6, [1e-9, 0, 0, 1, 2, 3], [0.01, -0.02, 0.03, 5, -6, 7], [1.0, 2.0, -0.5, 0, 0, 0]], dtype=torch.float64)
    assert torch.equal(correction_matrix(d), co.correction_matrix(d))
    R = correction_matrix(d)[:, :3, :3]
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-15


def _batch(case):
    """A batch dict whose cameras are the case's (K [R | t] recovered from the fp32 P by the generator's own arrays)."""
    rng = np.random.default_rng(3)
    x, N, V = {}, case['N'], case['V']
    rigs = [ci.ring_cameras(V, rng) for _ in range(case['R'])]
    for v in range(V):
        x['cam_%d_k_mat' % v] = torch.tensor(np.stack([rigs[r][0][v] for r in case['rig']]), dtype=torch.float32).cuda()
        x['cam_%d_rot_world' % v] = torch.tensor(np.stack([rigs[r][1][v] for r in case['rig']]), dtype=torch.float32).cuda()
        x['cam_%d_trans_world' % v] = torch.tensor(np.stack([rigs[r][2][v] for r in case['rig']]), dtype=torch.float32).cuda()
    return x


@pytest.mark.gpu
def test_rigs_of_and_apply_calibration():
    from modules.util import apply_calibration, correction_matrix
    from xas_amd import ops_calib, ops_eval
    case = ci.make('typical')
    cams = list(range(case['V']))
    x = _batch(case)
    pm = lambda d: torch.stack([ops_eval.projection_matrix(d['cam_%d_k_mat' % v], d['cam_%d_rot_world' % v], d['cam_%d_trans_world' % v])
                                for v in cams], dim=1)
    P = pm(x)
    rig, keys = ops_calib.rigs_of(P)
    assert keys.shape == (2, case['V'], 3, 4) and torch.equal(keys[rig].view(torch.int32), P.view(torch.int32))
    truth = torch.as_tensor(case['rig']).cuda()
    assert torch.equal(rig, truth) or torch.equal(rig, 1 - truth)                    # the same grouping, in the order of unique
    many = torch.arange(17 * 2 * 12, dtype=torch.float32, device='cuda').reshape(17, 2, 3, 4)
    with pytest.raises(RuntimeError, match='17 different camera rigs'):
        ops_calib.rigs_of(many)
    delta = torch.tensor(np.random.default_rng(1).normal(size=(2, case['V'], 6)) * ([5e-3] * 3 + [10.0] * 3), device='cuda')
    y = apply_calibration(x, cams, keys, delta)
    assert y is not x and all(y[k] is x[k] for k in x if 'k_mat' in k)
    want = P.double() @ correction_matrix(delta)[rig]
    got = pm(y).double()
    # fp32: rot and trans are rounded once (half an ulp each), the kernel's three products and two sums add an ulp each of the
    # largest term, which the largest entry of the row bounds: 8 ulps of that entry
    ulp = torch.as_tensor(np.spacing(want.abs().amax(dim=-1, keepdim=True).float().cpu().numpy())).cuda().double()
    ratio = float(((got - want).abs() / ulp).max())
    print('apply_calibration: largest distance %.2f ulps of the row maximum' % ratio)
    assert ratio <= 8.0
    rig2, keys2 = ops_calib.rigs_of(pm(y))
    assert torch.equal(rig2, rig) or torch.equal(rig2, 1 - rig)
    z = dict(x)
    z['cam_1_trans_world'] = x['cam_1_trans_world'] + 1.0
    with pytest.raises(RuntimeError, match='match none'):
        apply_calibration(z, cams, keys, delta)


def _setup():
    from test_gpu_tri_robust import eval_case
    x, kps, _ = eval_case()
    cams = [0, 1, 2, 3]
    xd = {k: v.cuda() for k, v in x.items()}
    det = PlantedDetector()
    det.kps = {}
    for i, c in enumerate(cams):
        xd['cam_%d_img' % c] = torch.full((1, 3, 256, 256), float(i), device='cuda')
        det.kps[i] = kps[c][1].cuda()
    w = torch.tensor([0.004, -0.003, 0.005], dtype=torch.float64)                    # camera 2 bumped: 0.4 degrees and 12 mm
    E = torch.as_tensor(ci.rodrigues(w.numpy())).cuda()
    R = xd['cam_2_rot_world'].double()
    xd['cam_2_rot_world'] = (R @ E).float()
    xd['cam_2_trans_world'] = (xd['cam_2_trans_world'].double() + R @ torch.tensor([8.0, -6.0, 7.0], dtype=torch.float64).cuda()).float()
    return cams, xd, det


@pytest.mark.gpu
def test_calibrate_writes_its_file_and_calibration_uses_it(tmp_path):
    import eval as xeval
    from xas_amd import ops_calib
    cams, xd, det = _setup()
    path = str(tmp_path / 'out' / 'calib.npz')
    keys = dict(tri_refine='lm')
    texts, outs = {}, {}
    for tag, extra in (('today', {}), ('calibrate', dict(calibrate=path, calib_iters=10)), ('calibration', dict(calibration=path))):
        e = xeval.Eval(_cfg(cams, **keys, **extra), det, [dict(xd), dict(xd)], str(tmp_path / tag), tri='robust')
        outs[tag] = e.eval_batch(dict(xd), 'best')
        if tag == 'calibrate':
            e.calib_rows = []
        e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        if tag == 'calibrate':
            kept = {k: (None if e.calib_rows[0][k] is None else torch.cat([r[k] for r in e.calib_rows])) for k in e.calib_rows[0]}
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt').read().strip().split('\n')
    today, cal, used = outs['today'], outs['calibrate'], outs['calibration']
    bits = lambda t: t.reshape(-1).contiguous().view(torch.uint8)
    assert set(cal) == set(today) and all(torch.equal(bits(cal[k]), bits(today[k])) for k in today)
    n = len(texts['today'])
    assert texts['calibrate'][:n] == texts['today']                    # nothing but one last line per rig
    with np.load(path) as z:
        assert sorted(z.files) == ['cam_cov', 'cost', 'delta', 'keys', 'rms', 'status']
        R = z['keys'].shape[0]
        assert z['keys'].shape == (R, 4, 3, 4) and z['delta'].shape == (R, 4, 6) and z['cam_cov'].shape == (R, 24, 24)
        assert (z['delta'][:, 0] == 0).all() and np.abs(z['delta'][:, 2]).max() > 0
        assert (z['cost'][:, 1] <= z['cost'][:, 0]).all() and (z['rms'][:, 1] < z['rms'][:, 0]).all()
        rms = z['rms'].mean(0)
        file = {k: z[k] for k in z.files}
    # the oracle on what the batches kept, made to take the device's decisions at ties (test_gpu_calib): the file's figures
    # are its figures within 16 x the distance between the oracle's own two formulations, floored at 64 ulps
    import _calib_oracle as co
    from test_calib_abi import formulation_distance
    from test_gpu_calib import EPS, gpu_decisions
    rig, keys_dev = ops_calib.rigs_of(kept['pmat'])
    assert np.array_equal(keys_dev.cpu().numpy().view(np.uint32), file['keys'].view(np.uint32))
    kw = dict(free=None, weighted=False, huber_px=0.0, prior_rot=ops_calib.CALIB_PRIOR_ROT, prior_trans=ops_calib.CALIB_PRIOR_TRANS,
              num_rigs=R)
    dec = gpu_decisions(dict(points=kept['points'], pmat=kept['pmat'], init=kept['init'], rig=rig, views=kept['views']), kw, 10)
    host = {k: (None if v is None else v.cpu().numpy()) for k, v in kept.items()}
    rig_h = rig.cpu().numpy()
    for r in range(R):
        m = rig_h == r
        g = co.Rig(host['points'][m], host['pmat'][m], host['init'][m], None if host['views'] is None else host['views'][m])
        a, b = co.follow(g, dec[r], 10)
        tol = max(16 * formulation_distance(a, b), 64 * EPS)
        scale = max(1.0, float(np.abs(b['X']).max()))
        dw = np.abs(file['delta'][r, :, :3] - b['delta'][:, :3]).max()
        dt = np.abs(file['delta'][r, :, 3:] - b['delta'][:, 3:]).max()
        print('eval rig %d: omega %.2e tau %.2e (tol %.2e), rms %s oracle %s, status %d' % (r, dw, dt / scale, tol, file['rms'][r], b['rms'],
                                                                                    file['status'][r]))
        assert int(file['status'][r]) == b['status'] and dw <= tol and dt <= tol * scale
        assert np.allclose(file['rms'][r], b['rms'], rtol=1e-9)
    rig_lines = texts['calibrate'][n:]
    assert len(rig_lines) == R and all(l.startswith('CALIBRATE rig %d (' % i) and ' of 10 trials, ' in l and ' px, largest |omega| ' in l and ' mm, ' in l
                                       for i, l in enumerate(rig_lines))
    assert not os.path.exists(path + '.tmp.npz')
    print('calibrate: rms %.3f -> %.3f px; tri mpjpe %.3f -> %.3f mm; refine px %.3f -> %.3f' % (
        rms[0], rms[1], float(today['mpjpe_tri'].mean()), float(used['mpjpe_tri'].mean()), float(today['tri_refine_px']),
        float(used['tri_refine_px'])))
    assert float(used['mpjpe_tri'].mean()) < float(today['mpjpe_tri'].mean())
    assert float(used['tri_refine_px']) < float(today['tri_refine_px'])
    assert torch.equal(used['world_gt'], today['world_gt'])            # the ground truth reads the cameras as given
