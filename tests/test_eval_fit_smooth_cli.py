"""eval.py --fit-smooth [W_ROT] / --fit-smooth-trans W (model_params.fit_smooth, fit_smooth_trans) without a GPU: the flags and
their model_params keys, the refusals without --fit-shape track, and that without the flags the option set and the keys are
what they were."""
from argparse import ArgumentParser

import numpy as np
import pytest
import torch


def _parse(argv, smooth=True):
    import eval as xeval
    parser = ArgumentParser()
    for flag, kw in xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT + xeval.CLI_FIT_SHAPE + (xeval.CLI_FIT_SMOOTH if smooth else ()):
        parser.add_argument(flag, **kw)
    return xeval, parser.parse_args(['--config', 'c.yaml'] + argv)


def test_flags_and_their_config_keys():
    from xas_amd import ops_smplfit
    xeval, opt = _parse([])
    flags = dict(xeval.CLI_FIT_SMOOTH)
    assert list(flags) == ['--fit-smooth', '--fit-smooth-trans']
    assert not set(flags) & (set(dict(xeval.CLI)) | set(dict(xeval.CLI_VOLUME)) | set(dict(xeval.CLI_FIT)) | set(dict(xeval.CLI_FIT_SHAPE)))
    assert opt.fit_smooth is None and opt.fit_smooth_trans is None
    cfg = {'model_params': {}}
    xeval.mirror_fit_smooth_options(cfg, opt)
    assert cfg['model_params'] == {}                                       # not given: no key at all
    head = ['--fit-smpl', 'bank.npz', '--fit-shape', 'track']
    xeval, opt = _parse(head + ['--fit-smooth'])
    xeval.mirror_fit_smooth_options(cfg, opt)
    assert cfg['model_params'] == {'fit_smooth': ops_smplfit.FIT_SMOOTH_ROT}  # the bare flag: the default weight
    cfg = {'model_params': {}}
    xeval, opt = _parse(head + ['--fit-smooth', '250', '--fit-smooth-trans', '0.5'])
    xeval.mirror_fit_smooth_options(cfg, opt)
    assert cfg['model_params'] == {'fit_smooth': 250.0, 'fit_smooth_trans': 0.5}
    cfg = {'model_params': {}}
    xeval, opt = _parse(head + ['--fit-smooth-trans', '2'])
    xeval.mirror_fit_smooth_options(cfg, opt)
    assert cfg['model_params'] == {'fit_smooth_trans': 2.0}
    assert (ops_smplfit.FIT_SMOOTH_ROT, ops_smplfit.FIT_SMOOTH_TRANS) == (1e4, 1.0)


def test_refused_without_fit_shape_track():
    for argv in (['--fit-smooth'], ['--fit-smooth-trans', '1'], ['--fit-smpl', 'b.npz', '--fit-smooth', '3'],
                 ['--fit-smpl', 'b.npz', '--fit-shape', 'frame', '--fit-smooth']):
        xeval, opt = _parse(argv)
        with pytest.raises(ValueError, match='needs --fit-shape track'):
            xeval.mirror_fit_smooth_options({'model_params': {}}, opt)
    base = {'dataset_params': {'dataset': {'name': 'mpi_inf_3dhp'}}}
    for keys in ({'fit_smooth': 1e4}, {'fit_smooth_trans': 1.0}):
        with pytest.raises(ValueError, match='needs fit_smpl'):
            xeval.Eval(dict(base, model_params=dict({'cam_id_list': [0, 1]}, **keys)), torch.nn.Identity(), [], 'log')


def test_without_the_flags_the_option_set_is_unchanged():
    xeval, with_tables = _parse([])
    _, without = _parse([], smooth=False)
    extra = set(vars(with_tables)) - set(vars(without))
    assert extra == {'fit_smooth', 'fit_smooth_trans'} and all(getattr(with_tables, k) is None for k in extra)
    assert {k: v for k, v in vars(with_tables).items() if k not in extra} == vars(without)
    with pytest.raises(SystemExit):
        _parse(['--fit-smooth'], smooth=False)


def test_joint_acceleration_of_the_file():
    import eval as xeval
    rng = np.random.Generator(np.random.PCG64(3))
    f = np.asarray([0, 1, 3, 4, 9, 2, 0, 1, 2], np.int32)                    # track 0 with uneven steps and a frame passed through; track 1
    track = np.asarray([0, 0, 0, 0, 0, 0, 1, 1, 1], np.int32)
    fitted = np.ones(9, bool)
    fitted[5] = False
    a, b = rng.standard_normal((2, 18, 3))
    J = a[None] + b[None] * f[:, None, None].astype(np.float64)              # linear in the frame number: no acceleration
    acc = xeval.joint_accel_mm(J, track, f, fitted)
    assert np.isnan(acc[[0, 4, 5, 6, 8]]).all() and np.abs(acc[[1, 2, 3, 7]]).max() <= 1e-12
    J2 = J + 0.5 * (f[:, None, None].astype(np.float64) ** 2) * np.asarray([3.0, 0.0, 4.0])
    acc = xeval.joint_accel_mm(J2, track, f, fitted)                         # x'' = (3, 0, 4): the stencil gives (h0 + h1) / 2 times it
    assert acc[1] == pytest.approx(5.0 * 1.5) and acc[2] == pytest.approx(5.0 * 1.5) and acc[7] == pytest.approx(5.0)
