"""eval.py --fit-smpl (model_params.fit_smpl): the flags and their model_params keys without a GPU; on the GPU, on the planted
evaluation batch of tests/test_gpu_tri_robust.py with the synthetic body of tests/_smplfit_inputs.py, what the flag adds to
eval_batch, the file it writes and the line eval_result.txt gains, and that nothing moves without it."""
import os
import subprocess
import sys
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

import _smplfit_inputs as si


def _parse(argv):
    import eval as xeval
    parser = ArgumentParser()
    for flag, kw in xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT:
        parser.add_argument(flag, **kw)
    return xeval, parser.parse_args(['--config', 'c.yaml'] + argv)


def test_flags_and_their_config_keys():
    xeval, opt = _parse([])
    flags = dict(xeval.CLI_FIT)
    assert list(flags) == ['--fit-smpl', '--smpl-model', '--fit-iters', '--fit-pose-prior', '--fit-shape-prior']
    assert not set(flags) & (set(dict(xeval.CLI)) | set(dict(xeval.CLI_VOLUME)))
    assert opt.fit_smpl is None and opt.smpl_model is None and opt.fit_iters == 30 and opt.fit_pose_prior is None
    cfg = {'model_params': {}}
    xeval.mirror_fit_options(cfg, opt)
    assert cfg['model_params'] == {'fit_smpl': None, 'smpl_model': None, 'fit_iters': 30}
    xeval, opt = _parse(['--fit-smpl', 'out/bank.npz', '--smpl-model', 'smpl.npz', '--fit-iters', '12', '--fit-pose-prior', '7.5',
                         '--fit-shape-prior', '0.5'])
    xeval.mirror_fit_options(cfg, opt)
    assert cfg['model_params'] == {'fit_smpl': 'out/bank.npz', 'smpl_model': 'smpl.npz', 'fit_iters': 12, 'fit_pose_prior': 7.5,
                                   'fit_shape_prior': 0.5}
    with pytest.raises(ValueError, match='fit_smpl needs an SMPL layer'):
        xeval.Eval({'model_params': {'cam_id_list': [0, 1], 'fit_smpl': 'x.npz'}, 'dataset_params': {'dataset': {'name': 'mpi_inf_3dhp'}}},
                   torch.nn.Identity(), [], 'log')


def test_the_fit_module_is_not_imported_without_the_flag():
    import eval as xeval
    pkg = os.path.dirname(os.path.abspath(xeval.__file__))
    code = "import sys; sys.path[:0] = %r; import eval; print('xas_amd.ops_smplfit' in sys.modules)" % ([pkg, os.path.dirname(pkg)],)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == 'False', r.stderr[-2000:]


class PlantedDetector(torch.nn.Module):
    num_kp = 18

    def forward(self, img):
        return self.kps[int(img[0, 0, 0, 0].item())], None


def _setup(tmp_path):
    from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer
    from test_gpu_tri_robust import eval_case
    x, kps, _ = eval_case()
    cams = [0, 1, 2, 3]
    xd = {k: v.cuda() for k, v in x.items()}
    det = PlantedDetector()
    det.kps = {}
    for i, c in enumerate(cams):
        xd['cam_%d_img' % c] = torch.full((1, 3, 256, 256), float(i), device='cuda')
        det.kps[i] = kps[c][1].cuda()
    a = si.arrays(70)
    path = str(tmp_path / 'smpl.npz')
    np.savez(path, **{k: np.asarray(v) for k, v in a.items()})
    return cams, xd, det, path, (SMPL_Layer.from_arrays(a, center_idx=0), torch.as_tensor(a['h36m_regressor']))


def _cfg(cams, **keys):
    cfg = {'model_params': {'cam_id_list': list(cams)}, 'dataset_params': {'dataset': {'name': 'mpi_inf_3dhp'}}}
    cfg['model_params'].update(keys)
    return cfg


@pytest.mark.gpu
@pytest.mark.parametrize('keys', [{}, dict(tri_refine='lm', tri_weight='spread')], ids=['plain', 'lm-spread'])
def test_eval_batch_fits_only_when_asked(tmp_path, keys):
    import eval as xeval
    from xas_amd import ops_smplfit
    cams, xd, det, model, smpl = _setup(tmp_path)
    if keys:                                       # the spread needs a detector with heat-maps: planted weights instead
        det.forward_spread = lambda img, pairs: (det(img)[0], None, torch.ones(xd['cam_0_joints'].shape[0], 18, 5, device='cuda'))
    today = xeval.Eval(_cfg(cams, **keys), det, [], str(tmp_path)).eval_batch(xd, 'best')
    off = xeval.Eval(_cfg(cams, fit_smpl=None, smpl_model=model, **keys), det, [], str(tmp_path)).eval_batch(xd, 'best')
    assert set(off) == set(today) and all(torch.equal(off[k], today[k]) for k in today)
    fit = xeval.Eval(_cfg(cams, fit_smpl=str(tmp_path / 'bank.npz'), smpl_model=model, fit_iters=8, **keys), det, [], str(tmp_path)).eval_batch(xd, 'best')
    new = {'fit_pose', 'fit_betas', 'fit_trans', 'fit_cost', 'fit_status', 'fit_joint_rms_mm'}
    assert set(fit) == set(today) | new and all(torch.equal(fit[k], today[k]) for k in today)
    B = today['world_tri'].shape[0]
    assert fit['fit_pose'].shape == (B, 72) and fit['fit_betas'].shape == (B, 10) and fit['fit_cost'].shape == (B, 2)
    assert (fit['fit_cost'][:, 1] <= fit['fit_cost'][:, 0]).all() and torch.isfinite(fit['fit_joint_rms_mm']).all()
    if not keys:                                   # the direct call on the triangulated joints with unit weights agrees
        tri = today['world_tri']
        w = torch.isfinite(tri).all(-1).float()
        r = ops_smplfit.fit_smpl(tri, w, smpl[0].cuda(), smpl[1].cuda(), iters=8)
        assert torch.equal(r['pose'].float(), fit['fit_pose']) and torch.equal(r['status'], fit['fit_status'])


@pytest.mark.gpu
def test_result_file_and_bank(tmp_path):
    import eval as xeval
    from xas_amd.pseudo import PseudoSynth
    cams, xd, det, model, smpl = _setup(tmp_path)
    texts = {}
    bank = str(tmp_path / 'out' / 'bank.npz')
    for tag, keys in (('today', {}), ('fit', dict(fit_smpl=bank, smpl_model=model, fit_iters=8))):
        e = xeval.Eval(_cfg(cams, **keys), det, [dict(xd), dict(xd)], str(tmp_path / tag))
        e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt').read()
    old, new = texts['today'].strip().split('\n'), texts['fit'].strip().split('\n')
    assert new[:-1] == old                                            # nothing but one last line
    assert new[-1].startswith('FIT smpl (8 trials, pose prior ') and 'joint RMS ' in new[-1] and 'passed through ' in new[-1]
    B = xd['cam_0_joints'].shape[0]
    with np.load(bank) as z:
        assert sorted(z.files) == ['betas', 'cost', 'joint_rms_mm', 'pose', 'status', 'trans']
        assert z['pose'].shape == (2 * B, 72) and z['pose'].dtype == np.float32 and z['status'].shape == (2 * B,)
        assert np.array_equal(z['pose'][:B], z['pose'][B:])              # the same batch twice
    synth = PseudoSynth(bank, smpl[0], smpl[1])
    assert tuple(synth.pose.shape) == (2 * B, 72) and torch.isfinite(synth.root).all()
