"""train.py --pseudo-online / --pseudo-look / --smpl-model without a GPU: the flags parse, sit in a table of their own after an
unchanged CLI, and without --pseudo-online the module behind them is never imported."""
import os
import subprocess
import sys
from argparse import ArgumentParser

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'x-as-supervision_amd')
CLI_FLAGS = ['--config', '--log_dir', '--checkpoint', '--batch_size', '--epoch', '--worker', '--extra_tag', '--finetune', '--seed',
             '--synthetic', '--mv-2d', '--mv-3d', '--mv-huber', '--mv-detach']


def _parser(xtrain):
    parser = ArgumentParser()
    for flag, kw in xtrain.CLI + xtrain.CLI_PSEUDO:
        parser.add_argument(flag, **kw)
    return parser


def test_flags_parse_and_cli_is_unchanged():
    import train as xtrain
    assert [f for f, _ in xtrain.CLI] == CLI_FLAGS
    assert [f for f, _ in xtrain.CLI_PSEUDO] == ['--pseudo-online', '--pseudo-look', '--smpl-model']
    assert not set(dict(xtrain.CLI)) & set(dict(xtrain.CLI_PSEUDO))
    p = _parser(xtrain)
    opt = p.parse_args(['--config', 'c.yaml'])
    assert (opt.pseudo_online, opt.pseudo_look, opt.smpl_model) == (None, 'shade', None)
    opt = p.parse_args(['--config', 'c.yaml', '--synthetic', '2', '--pseudo-online', 'bank.npz', '--pseudo-look', 'parts',
                        '--smpl-model', 'models/smpl'])
    assert (opt.pseudo_online, opt.pseudo_look, opt.smpl_model, opt.synthetic) == ('bank.npz', 'parts', 'models/smpl', 2)
    with pytest.raises(SystemExit):
        p.parse_args(['--config', 'c.yaml', '--pseudo-look', 'texture'])


def test_help_lists_the_flags():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train.py'), '--help'], capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr
    assert '--pseudo-online BANK.npz' in r.stdout and '--pseudo-look {shade,parts}' in r.stdout and '--smpl-model ROOT' in r.stdout


def test_without_the_flag_nothing_new_is_imported():
    code = ('import sys, types\n'
            'import train\n'
            'opt = types.SimpleNamespace(pseudo_online=None, pseudo_look="shade", smpl_model=None, seed=-1)\n'
            'assert train.pseudo_source(opt, {"dataset_params": {}}, None) is None\n'
            'assert "xas_amd.pseudo" not in sys.modules and "xas_amd.ops_render" not in sys.modules\n'
            'print("clean")\n')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0 and r.stdout.strip().endswith('clean'), r.stderr


def test_trainer_leaves_the_batch_alone_without_a_source():
    import inspect
    import train as xtrain
    p = inspect.signature(xtrain.Trainer.__init__).parameters
    assert list(p)[-1] == 'pseudo' and p['pseudo'].default is None
    src = inspect.getsource(xtrain.Trainer.train)
    assert 'if self.pseudo is not None:' in src
