"""eval.py --smooth-data (model_params.smooth_data) without a GPU: the flags and their model_params keys, the defaults that
ops_track holds, and the errors: two cameras without --tri-volume, and one camera without the flag as before."""
from argparse import ArgumentParser

import pytest
import torch

from test_eval_fit_cli import _cfg

FLAGS = ['--smooth-data', '--smooth-depth', '--smooth-anchor-huber']


def _parse(argv):
    import eval as xeval
    parser = ArgumentParser()
    for flag, kw in xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT + xeval.CLI_CALIB + xeval.CLI_SMOOTH + xeval.CLI_RESOLVE_TRACK + xeval.CLI_SMOOTH_ANCHOR:
        parser.add_argument(flag, **kw)
    return xeval, parser.parse_args(['--config', 'c.yaml'] + argv)


def test_flags_and_their_config_keys():
    xeval, opt = _parse([])
    flags = dict(xeval.CLI_SMOOTH_ANCHOR)
    assert list(flags) == FLAGS
    earlier = xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT + xeval.CLI_CALIB + xeval.CLI_SMOOTH + xeval.CLI_RESOLVE_TRACK
    assert not set(flags) & set(dict(earlier))
    assert opt.smooth_data is None and opt.smooth_depth is None and opt.smooth_anchor_huber is None
    cfg = {'model_params': {}}
    xeval.mirror_smooth_anchor_options(cfg, opt)
    assert cfg['model_params'] == {}                                    # nothing given: nothing moves
    xeval, opt = _parse(['--smooth', 's.npz', '--smooth-data', 'anchor', '--smooth-depth', '1e-3', '--smooth-anchor-huber', '2',
                         '--resolve-track', 'r.npz'])
    xeval.mirror_smooth_anchor_options(cfg, opt)
    assert cfg['model_params'] == {'smooth_data': 'anchor', 'smooth_depth': 1e-3, 'smooth_anchor_huber': 2.0}
    with pytest.raises(SystemExit):
        _parse(['--smooth-data', 'pixels'])
    assert 'sigma^2' in flags['--smooth-data']['help'] and '--smooth-acc' in flags['--smooth-data']['help']


def test_defaults_come_from_ops_track():
    import eval as xeval
    from xas_amd import ops_track
    e = xeval.Eval(_cfg([0], smooth='a.npz', smooth_data='anchor'), torch.nn.Identity(), [], 'log')
    assert e.smooth_data == 'anchor' and e.smooth_depth == ops_track.TRACK_DEPTH_W == 4e-4
    assert e.smooth_anchor_huber == ops_track.TRACK_ANCHOR_HUBER == 3.0 and e.smooth_acc == ops_track.TRACK_ACC_W
    e = xeval.Eval(_cfg([0], smooth='a.npz', smooth_data='anchor', smooth_depth=1e-3, smooth_anchor_huber=0.0), torch.nn.Identity(), [], 'log')
    assert e.smooth_depth == 1e-3 and e.smooth_anchor_huber == 0.0
    e = xeval.Eval(_cfg([0, 1], smooth='a.npz'), torch.nn.Identity(), [], 'log')
    assert e.smooth_data == 'reproj'
    assert xeval.Eval(_cfg([0]), torch.nn.Identity(), [], 'log').smooth_data == 'reproj'


def test_errors():
    import eval as xeval
    with pytest.raises(ValueError, match='--tri-volume'):
        xeval.Eval(_cfg([0, 1], smooth='a.npz', smooth_data='anchor'), torch.nn.Identity(), [], 'log')
    xeval.Eval(_cfg([0, 1], smooth='a.npz', smooth_data='anchor', tri_volume=True), torch.nn.Identity(), [], 'log')
    with pytest.raises(ValueError, match='smooth needs 2 to'):           # without --smooth-data one camera is refused as before
        xeval.Eval(_cfg([0], smooth='a.npz'), torch.nn.Identity(), [], 'log')
    with pytest.raises(ValueError, match='smooth needs 2 to'):
        xeval.Eval(_cfg([0], smooth='a.npz', smooth_data='reproj'), torch.nn.Identity(), [], 'log')
    with pytest.raises(ValueError, match='Unknown smoothing data'):
        xeval.Eval(_cfg([0, 1], smooth='a.npz', smooth_data='pixels'), torch.nn.Identity(), [], 'log')
