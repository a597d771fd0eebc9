"""eval.py --fit-data (model_params.fit_data) without a GPU: the flag and its key, the combinations it refuses at the command
line and in Eval before anything is loaded onto a device."""
from argparse import ArgumentParser

import pytest
import torch


def _parse(argv):
    import eval as xeval
    parser = ArgumentParser()
    for flag, kw in xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT + xeval.CLI_FIT_SHAPE + xeval.CLI_FIT_SMOOTH + xeval.CLI_FIT_DATA:
        parser.add_argument(flag, **kw)
    return xeval, parser.parse_args(['--config', 'c.yaml'] + argv)


def test_flag_and_its_config_key():
    xeval, opt = _parse([])
    assert list(dict(xeval.CLI_FIT_DATA)) == ['--fit-data'] and opt.fit_data is None
    taken = [dict(t) for t in (xeval.CLI, xeval.CLI_VOLUME, xeval.CLI_FIT, xeval.CLI_CALIB, xeval.CLI_SMOOTH, xeval.CLI_RESOLVE_TRACK,
                               xeval.CLI_SMOOTH_ANCHOR, xeval.CLI_SMOOTH_BONES, xeval.CLI_FIT_SHAPE, xeval.CLI_FIT_SMOOTH)]
    assert not any('--fit-data' in t for t in taken)
    cfg = {'model_params': {}}
    xeval.mirror_fit_data_options(cfg, opt)
    assert cfg['model_params'] == {}                                   # not given: no key, today's calls
    for value in ('joints', 'reproj'):
        xeval, opt = _parse(['--fit-smpl', 'bank.npz', '--fit-data', value])
        cfg = {'model_params': {}}
        xeval.mirror_fit_data_options(cfg, opt)
        assert cfg['model_params'] == {'fit_data': value}
    with pytest.raises(SystemExit):
        _parse(['--fit-data', 'pixels'])


def test_refused_combinations_at_the_command_line():
    xeval, opt = _parse(['--fit-data', 'reproj'])
    with pytest.raises(ValueError, match='needs --fit-smpl'):
        xeval.mirror_fit_data_options({'model_params': {}}, opt)
    xeval, opt = _parse(['--fit-smpl', 'b.npz', '--fit-data', 'reproj', '--fit-shape', 'track'])
    with pytest.raises(ValueError, match='does not go with --fit-shape track'):
        xeval.mirror_fit_data_options({'model_params': {}}, opt)
    xeval, opt = _parse(['--fit-smpl', 'b.npz', '--fit-data', 'reproj', '--flip'])
    with pytest.raises(ValueError, match='does not go with --flip'):
        xeval.mirror_fit_data_options({'model_params': {}}, opt)
    xeval, opt = _parse(['--fit-data', 'joints', '--flip'])             # the default mode refuses nothing
    xeval.mirror_fit_data_options({'model_params': {}}, opt)


def test_refused_combinations_in_eval(tmp_path):
    import numpy as np
    import eval as xeval
    import _smplfit_inputs as si
    path = str(tmp_path / 'smpl.npz')
    np.savez(path, **{k: np.asarray(v) for k, v in si.arrays(70).items()})
    base = {'cam_id_list': [0, 1], 'smpl_model': path}
    cfg = lambda **keys: {'model_params': dict(base, **keys), 'dataset_params': {'dataset': {'name': 'mpi_inf_3dhp'}}}
    make = lambda c, **kw: xeval.Eval(c, torch.nn.Identity(), [], 'log', **kw)
    with pytest.raises(ValueError, match='fit_data reproj is a mode of --fit-smpl'):
        make(cfg(fit_data='reproj'))
    with pytest.raises(ValueError, match='fit_data is joints or reproj'):
        make(cfg(fit_smpl='b.npz', fit_data='pixels'))
    with pytest.raises(ValueError, match='does not go with --fit-shape track'):
        make(cfg(fit_smpl='b.npz', fit_data='reproj', fit_shape='track'))
    with pytest.raises(ValueError, match='does not go with --flip'):
        make(cfg(fit_smpl='b.npz', fit_data='reproj'), flip_test=True)
