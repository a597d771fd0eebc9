"""eval.py --fit-shape track (model_params.fit_shape): the flags and their model_params keys and that the default imports nothing
new, without a GPU; on the GPU, on the planted evaluation batch of tests/test_eval_fit_cli.py, the file the option writes, that
PseudoSynth reads it, and that a run without the flag writes what it wrote before."""
import os
import subprocess
import sys
from argparse import ArgumentParser

import numpy as np
import pytest
import torch


def _parse(argv):
    import eval as xeval
    parser = ArgumentParser()
    for flag, kw in xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT + xeval.CLI_FIT_SHAPE:
        parser.add_argument(flag, **kw)
    return xeval, parser.parse_args(['--config', 'c.yaml'] + argv)


def test_flags_and_their_config_keys():
    xeval, opt = _parse([])
    flags = dict(xeval.CLI_FIT_SHAPE)
    assert list(flags) == ['--fit-shape', '--fit-gap']
    assert not set(flags) & (set(dict(xeval.CLI)) | set(dict(xeval.CLI_VOLUME)) | set(dict(xeval.CLI_FIT)))
    assert opt.fit_shape is None and opt.fit_gap is None
    cfg = {'model_params': {}}
    xeval.mirror_fit_shape_options(cfg, opt)
    assert cfg['model_params'] == {}                                       # not given: the defaults stay where Eval has them
    xeval, opt = _parse(['--fit-smpl', 'bank.npz', '--fit-shape', 'track', '--fit-gap', '3'])
    xeval.mirror_fit_shape_options(cfg, opt)
    assert cfg['model_params'] == {'fit_shape': 'track', 'fit_gap': 3}
    xeval, opt = _parse(['--fit-smpl', 'bank.npz', '--fit-shape', 'frame'])
    cfg = {'model_params': {}}
    xeval.mirror_fit_shape_options(cfg, opt)
    assert cfg['model_params'] == {'fit_shape': 'frame'}
    with pytest.raises(SystemExit):
        _parse(['--fit-shape', 'sequence'])


def test_track_is_refused_without_fit_smpl():
    xeval, opt = _parse(['--fit-shape', 'track'])
    with pytest.raises(ValueError, match='needs --fit-smpl'):
        xeval.mirror_fit_shape_options({'model_params': {}}, opt)
    base = {'dataset_params': {'dataset': {'name': 'mpi_inf_3dhp'}}}
    with pytest.raises(ValueError, match='needs fit_smpl'):
        xeval.Eval(dict(base, model_params={'cam_id_list': [0, 1], 'fit_shape': 'track'}), torch.nn.Identity(), [], 'log')
    xeval.Eval(dict(base, model_params={'cam_id_list': [0, 1], 'fit_shape': 'frame'}), torch.nn.Identity(), [], 'log')


def test_the_default_imports_nothing_new():
    import eval as xeval
    pkg = os.path.dirname(os.path.abspath(xeval.__file__))
    code = ("import sys; sys.path[:0] = %r; import eval, torch; "
            "eval.Eval({'model_params': {'cam_id_list': [0, 1]}, 'dataset_params': {'dataset': {'name': 'mpi_inf_3dhp'}}}, torch.nn.Identity(), [], 'log'); "
            "print([m for m in ('xas_amd.ops_smplfit', 'xas_amd.ops_track') if m in sys.modules])" % ([pkg, os.path.dirname(pkg)],))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == '[]', r.stderr[-2000:]


@pytest.mark.gpu
def test_track_file_and_bank(tmp_path):
    import eval as xeval
    from test_eval_fit_cli import _cfg, _setup
    from xas_amd.pseudo import PseudoSynth
    cams, xd, det, model, smpl = _setup(tmp_path)
    B = xd['cam_0_joints'].shape[0]
    # two sequences, interleaved in every batch; the second one's batches lie 5 frames further apart, which --fit-gap 3 cuts
    paths = [['seq%d/img_%06d.jpg' % (i % 2, b * (B + 5 * (i % 2)) + i // 2) for i in range(B)] for b in range(2)]
    batches = [dict(xd, cam_0_img_path=paths[b]) for b in range(2)]
    banks, texts = {}, {}
    for tag, keys in (('frame', {}), ('named', dict(fit_shape='frame')), ('track', dict(fit_shape='track', fit_gap=3))):
        banks[tag] = str(tmp_path / tag / 'bank.npz')
        e = xeval.Eval(_cfg(cams, fit_smpl=banks[tag], smpl_model=model, fit_iters=8, **keys), det, [dict(b) for b in batches], str(tmp_path / tag))
        e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt').read().strip().split('\n')
    assert texts['track'][:-1] == texts['frame'][:-1] and texts['track'][-1].startswith(texts['frame'][-1].split(': joint RMS')[0])
    assert 'shape per track: ' in texts['track'][-1] and 'within-track std of the per-frame betas' in texts['track'][-1]
    assert 'shape per track' not in texts['frame'][-1]
    with np.load(banks['frame']) as z:
        old = {k: z[k] for k in z.files}
    with np.load(banks['named']) as z:
        named = {k: z[k] for k in z.files}
    # the default file, array for array, is what the per-sample fit gives on the batches' triangulated joints (what the option's
    # own tests pin: unit weights on this planted batch), rebuilt here from a direct fit_smpl and the file's own formulas
    from xas_amd import ops_smplfit
    tri = xeval.Eval(_cfg(cams), det, [], str(tmp_path)).eval_batch(dict(xd), 'best')['world_tri']
    ok = torch.isfinite(tri).all(-1)
    r = ops_smplfit.fit_smpl(tri, ok.float(), smpl[0].cuda(), smpl[1].cuda(), iters=8)
    d2 = ((r['joints'] - torch.where(ok.unsqueeze(-1), tri.double(), r['joints'])) ** 2).sum(dim=-1)
    rms = (d2.sum(dim=1) / ok.double().sum(dim=1).clamp(min=1.0)).sqrt()
    twice = lambda v: np.concatenate([v.cpu().numpy()] * 2)             # the same batch twice
    expect = {'pose': twice(r['pose'].float()), 'betas': twice(r['betas'].float()), 'trans': twice(r['trans'].float()),
              'cost': twice(r['cost'].float()), 'status': twice(r['status']), 'joint_rms_mm': twice(rms.float())}
    assert sorted(old) == sorted(expect) == sorted(named)
    for k, v in expect.items():
        assert old[k].dtype == v.dtype == named[k].dtype and np.array_equal(old[k], v) and np.array_equal(named[k], v), k
    assert texts['named'] == texts['frame']                             # fit_shape frame is no key at all
    with np.load(banks['track']) as z:
        new = {k: z[k] for k in z.files}
    assert sorted(new) == sorted(list(old) + ['betas_per_frame', 'track', 'frame', 'track_betas', 'track_status', 'track_trials'])
    assert np.array_equal(new['betas_per_frame'], old['betas']) and new['pose'].dtype == np.float32 and new['pose'].shape == (2 * B, 72)
    S = len(new['track_betas'])
    assert S == len(np.unique(new['track'])) >= 2 and new['track_trials'].shape == (S,)
    for s in range(S):
        rows = new['track'] == s
        fitted = rows & (new['status'] != 2)
        assert (new['betas'][fitted] == new['track_betas'][s]).all()
    assert (new['cost'][:, 1] <= new['cost'][:, 0]).all()
    synth = PseudoSynth(banks['track'], smpl[0], smpl[1])
    assert tuple(synth.pose.shape) == (2 * B, 72) and torch.isfinite(synth.root).all()
