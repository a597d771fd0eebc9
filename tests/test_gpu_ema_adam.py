"""Averaged weights of FusedAdam (`ema_decay`): the shadow arena that xas_adam_step_ema / xas_adam_step_guarded_ema maintain in
the launch that writes the parameters.

Arena sizes, those of test_gpu_guarded_adam.py: one float4 (255 idle threads), ragged against 256 x 4, the odd parameter shapes
(an arena with zero-padded slots) and 4096 * 256 * 4 + 4 (the grid cap reached, exactly one float4 goes round the loop).

Bound of the shadow against its float64 replay e64 = d * e64 + omd * p (d, omd: the fp32 factors the kernel was handed; p: the
fp32 parameters the kernel itself produced, read back after every step).  A step rounds twice, the product omd * p and the
fused multiply-add, each by at most 2^-24 * max(|e|, |p|); the error of earlier steps is multiplied by d < 1.  So after T steps
|e - e64| <= T * 2^-23 * max(|p|, |e|): 2.4e-6 for T = 20 and parameters uniform in (-1, 1).  Asserted as written, from T.
"""
import argparse
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'x-as-supervision_amd')
LR, BETAS = 2e-4, (0.5, 0.999)
SIZES = {'n4': [(4,)], 'n1028': [(1028,)], 'odd': [(64, 3, 7, 7), (64,), (17, 5), (1,), (128, 64, 3, 3)],
         'cap': [(4096 * 256 * 4 + 4,)]}
ARENA = {'n4': 4, 'n1028': 1028, 'odd': 9408 + 64 + 88 + 4 + 73728, 'cap': 4096 * 256 * 4 + 4}
FORMS = {'plain': {}, 'guarded': {'skip_nonfinite': True}}
_inputs = {}


def _uniform(shape, g):
    return torch.rand(shape, generator=g) * 2 - 1


def _data(size):
    """Initial parameters and two gradient sets per size, uniform in (-1, 1): made once, on the device, never written."""
    if size not in _inputs:
        g = torch.Generator().manual_seed(11 + len(_inputs))
        _inputs[size] = tuple([_uniform(s, g).cuda() for s in SIZES[size]] for _ in range(3))
    return _inputs[size]


def _grads(size, it):
    """Gradients of step `it`: the two sets in turn, scaled 0.1 + it % 3 (the scales of test_gpu_guarded_adam.py)."""
    return [x * (0.1 + it % 3) for x in _data(size)[1 + it % 2]]


def _make(size, **opts):
    from xas_amd.optim import FusedAdam
    ps = [nn.Parameter(p.clone()) for p in _data(size)[0]]
    opt = FusedAdam(ps, lr=LR, betas=BETAS, **opts)
    opt.zero_grad()
    assert opt._flat['n'] == ARENA[size]
    return ps, opt


def _step(ps, opt, grads):
    for p, gr in zip(ps, grads):
        p.grad.copy_(gr)
    opt.step()


def _gnorm(grads):
    return float(torch.cat([gr.double().reshape(-1) for gr in grads]).norm())


def _sample(size):
    """Arena indices the float64 replay follows: everything, or on the large arena a stride plus the first and last float4."""
    n = ARENA[size]
    if n <= 100000:
        return torch.arange(n).cuda()
    return torch.cat([torch.arange(4), torch.arange(4, n - 4, 4099), torch.arange(n - 4, n)]).cuda()


@pytest.mark.parametrize('size', list(SIZES))
@pytest.mark.parametrize('form', ['plain', 'clipped', 'unclipped'])
def test_the_update_itself_is_untouched(size, form):
    """p, m, v after three steps: bit for bit those of the entry point without the shadow."""
    opts = {'plain': {}, 'clipped': {'max_grad_norm': 0.5 * min(_gnorm(_grads(size, it)) for it in range(3))},
            'unclipped': {'max_grad_norm': 1e9}}[form]
    (pa, oa), (pb, ob) = _make(size, **opts), _make(size, ema_decay=0.999, **opts)
    for it in range(3):
        _step(pa, oa, _grads(size, it))
        _step(pb, ob, _grads(size, it))
    if form != 'plain':
        from xas_amd import _lib
        scale = float(ob._flat['guard'][_lib.GUARD_SCALE])
        assert (scale < 0.51) if form == 'clipped' else (scale == 1.0)
    for k in ('p', 'm', 'v'):
        assert torch.equal(oa._flat[k], ob._flat[k]), k
    assert not torch.equal(ob._flat['ema'], ob._flat['p'])


class _Replay:
    """The shadow's float64 replay on the sampled indices, asserted against the bound after every step taken."""

    def __init__(self, size, ps, opt):
        self.size, self.ps, self.opt, self.idx = size, ps, opt, _sample(size)
        assert torch.equal(opt._flat['ema'], opt._flat['p'])               # the shadow starts as a copy of the parameters
        self.e64 = opt._flat['p'][self.idx].cpu().double()
        self.t, self.peak, self.err, self.bound = 0, float(self.e64.abs().max()), 0.0, 0.0

    def step(self, grads):
        d, omd = self.opt._ema_factors
        _step(self.ps, self.opt, grads)
        self.t += 1
        p = self.opt._flat['p'][self.idx].cpu().double()
        e = self.opt._flat['ema'][self.idx].cpu().double()
        self.e64 = d * self.e64 + omd * p
        self.peak = max(self.peak, float(p.abs().max()), float(e.abs().max()))
        self.bound = self.t * 2.0 ** -23 * self.peak
        self.err = float((e - self.e64).abs().max())
        assert self.err <= self.bound, 'step %d: shadow %.3g from its float64 replay, bound %.3g' % (self.t, self.err, self.bound)


@pytest.mark.parametrize('size', list(SIZES))
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('decay', [0.999, 0.5])
def test_shadow_vs_float64(size, form, decay):
    T = 20
    ps, opt = _make(size, ema_decay=decay, **FORMS[form])
    r = _Replay(size, ps, opt)
    for it in range(T):
        r.step(_grads(size, it))
    print('%s %s decay %g: shadow %.3g from float64 after %d steps (bound %.3g)' % (size, form, decay, r.err, r.t, r.bound))
    assert r.t == T and r.bound <= T * 2.0 ** -23 * 1.05      # 2.4e-6: |p|, |e| stay close to (-1, 1) at this learning rate
    assert float((opt._flat['ema'] - opt._flat['p']).abs().max()) > 1e-5       # an average, not a copy


@pytest.mark.parametrize('size', list(SIZES))
@pytest.mark.parametrize('form', list(FORMS))
def test_decay_zero_is_a_copy(size, form):
    ps, opt = _make(size, ema_decay=0.0, **FORMS[form])
    p0 = opt._flat['p'].clone()
    for it in range(3):
        _step(ps, opt, _grads(size, it))
        assert torch.equal(opt._flat['ema'], opt._flat['p'])
    assert not torch.equal(opt._flat['p'], p0)


@pytest.mark.parametrize('size', list(SIZES))
def test_skipped_step_keeps_the_shadow(size):
    """step, skip, step: the skipped call leaves p, m, v and the shadow bit for bit; the replay that never saw it still holds."""
    ps, opt = _make(size, ema_decay=0.999, skip_nonfinite=True)
    f, r = opt._flat, _Replay(size, ps, opt)
    r.step(_grads(size, 0))
    before = {k: f[k].clone() for k in ('p', 'm', 'v', 'ema')}
    bad = _grads(size, 1)
    bad[-1].view(-1)[-1] = float('nan')                       # an input value: the last real element of the arena
    _step(ps, opt, bad)
    assert int(opt.skipped_steps) == 1
    for k, x in before.items():
        assert torch.equal(f[k], x), k
    r.step(_grads(size, 2))
    assert r.t == 2 and int(opt.skipped_steps) == 1
    for k, x in before.items():
        assert not torch.equal(f[k], x), k
    print('%s: step, skip, step: shadow %.3g from float64 (bound %.3g)' % (size, r.err, r.bound))


def test_entry_points_and_allocation(monkeypatch):
    from xas_amd import _lib
    names, orig = [], _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *args: (names.append(name), orig(name, *args))[1])
    ps, opt = _make('n1028')
    _step(ps, opt, _grads('n1028', 0))
    assert names == ['xas_adam_step'] and 'ema' not in opt._flat and opt.ema_arena is None
    with pytest.raises(RuntimeError):
        opt.ema_views()
    with pytest.raises(RuntimeError):
        with opt.averaged():
            pass
    names.clear()
    ps, opt = _make('n1028', ema_decay=0.9)
    _step(ps, opt, _grads('n1028', 0))
    assert names == ['xas_adam_step_ema'] and opt.ema_arena is opt._flat['ema']
    names.clear()
    ps, opt = _make('n1028', ema_decay=0.9, max_grad_norm=1.0)
    _step(ps, opt, _grads('n1028', 0))
    assert names == ['xas_grad_guard', 'xas_adam_step_guarded_ema']


def test_views_load_and_rehoming():
    ps, opt = _make('odd', ema_decay=0.9)
    for it in range(2):
        _step(ps, opt, _grads('odd', it))
    views = opt.ema_views()
    assert [v.shape for v in views] == [p.shape for p in ps]
    assert all(v.data_ptr() == opt.ema_arena.data_ptr() + 4 * o for v, o in zip(views, opt._flat['offs']))
    saved = [v.clone() for v in views]
    # a parameter moved onto storage of its own is re-homed by the next step; its shadow slot keeps its average
    with torch.no_grad():
        ps[2].data = ps[2].data.clone()
    d, omd = opt._ema_factors
    _step(ps, opt, _grads('odd', 2))
    assert ps[2].data_ptr() == opt.param_arena.data_ptr() + 4 * opt._flat['offs'][2]
    want = d * saved[2].double() + omd * ps[2].detach().double()
    assert float((views[2].double() - want).abs().max()) <= 2.0 ** -23 * 1.01
    ps2, opt2 = _make('odd', ema_decay=0.9)
    opt2.load_ema(saved)
    assert all(torch.equal(a, b) for a, b in zip(opt2.ema_views(), saved))
    with pytest.raises(ValueError):
        opt2.load_ema(saved[:-1])


def test_state_snapshot_and_restore_carry_the_shadow():
    """xas_amd.state (bench.py's variant check, the reproducibility tests): the same steps from the same state give the same
    shadow; a step object as small as the module reads it."""
    import types
    from xas_amd import state
    ps, opt = _make('odd', ema_decay=0.9, skip_nonfinite=True)
    _step(ps, opt, _grads('odd', 0))
    step = types.SimpleNamespace(opt_det=opt, opt_disc=None, model=nn.Identity(), disc=nn.Identity(), cur_step=1)
    sn = state.snapshot(step)
    kept = {k: opt._flat[k].clone() for k in ('p', 'm', 'v', 'ema')}
    runs = []
    for _ in range(2):
        for it in (1, 2):
            _step(ps, opt, _grads('odd', it))
        runs.append({k: opt._flat[k].clone() for k in kept})
        assert not torch.equal(runs[-1]['ema'], kept['ema'])
        state.restore(step, sn)
        assert all(torch.equal(opt._flat[k], x) for k, x in kept.items())
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in kept)


def test_averaged_context_swaps_weights_and_packed_copies():
    """A convolution on the MFMA path (packed / split weight copies cached per optimizer epoch) evaluates the averaged weights
    inside the context and the trained ones after it."""
    from xas_amd import layers as L
    from xas_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(5)
    layer = L.Conv2d(32, 32, 3, padding=1).cuda()
    opt = FusedAdam(layer.parameters(), lr=1e-2, betas=BETAS, ema_decay=0.9)
    opt.zero_grad()
    x = torch.randn(2, 32, 8, 8, generator=g).cuda()
    for _ in range(3):
        for p in layer.parameters():
            p.grad.copy_(torch.randn(p.shape, generator=g).cuda())
        opt.step()
    with torch.no_grad():
        y_live = layer(x).clone()                              # (fills the layer's weight cache with the trained weights)
        live = [p.detach().clone() for p in layer.parameters()]
        ema = [v.clone() for v in opt.ema_views()]
        assert not torch.equal(live[0], ema[0]) and not torch.equal(live[1], ema[1])
        fresh = L.Conv2d(32, 32, 3, padding=1).cuda()
        fresh.weight.copy_(ema[0])
        fresh.bias.copy_(ema[1])
        y_ref = fresh(x)
        assert not torch.equal(y_ref, y_live)
        with opt.averaged():
            assert torch.equal(layer.weight, ema[0]) and torch.equal(layer.bias, ema[1])
            assert all(torch.equal(v, w) for v, w in zip(opt.ema_views(), live))
            assert torch.equal(layer(x), y_ref)
            with pytest.raises(RuntimeError):
                opt.step()
            with pytest.raises(RuntimeError):
                with opt.averaged():
                    pass
        assert all(torch.equal(p, w) for p, w in zip(layer.parameters(), live))
        assert all(torch.equal(v, w) for v, w in zip(opt.ema_views(), ema))
        assert torch.equal(layer(x), y_live)
    for p in layer.parameters():                               # and the optimizer goes on
        p.grad.copy_(torch.randn(p.shape, generator=g).cuda())
    opt.step()
    assert not torch.equal(layer.weight, live[0])


@pytest.mark.multiproc
@pytest.mark.limit(400)
def test_checkpoint_round_trip(tmp_path, monkeypatch):
    """The synthetic train entry with train_params.ema_decay: the checkpoint carries 'unsup_model_ema', a resume restores the
    shadow from it, eval.py --ema builds the detector from it; without the key nothing is added."""
    import yaml
    from _ranks import free_port, release_gpu_memory
    from xas_amd.synthetic import model_config
    env = dict(os.environ, PYTHONPATH=PKG, MASTER_ADDR='127.0.0.1')
    saved, cfgs = {}, {}
    for tag, extra in (('ema', {'ema_decay': 0.9}), ('off', {})):
        cfg = model_config('HM36_Multi_SurS2')
        cfg['dataset_params']['cam_id_list'] = [0, 1]
        cfg['train_params'].update(num_epochs=1, batch_size=2, checkpoint_freq=1, epoch_milestones=[40], **extra)
        (tmp_path / tag).mkdir()
        cfg_path = tmp_path / tag / 'HM36_Multi_SurS2.yaml'
        cfg_path.write_text(yaml.safe_dump(cfg))
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=1', '--master-addr', '127.0.0.1',
               '--master-port', str(free_port()), os.path.join(PKG, 'train.py'), '--config', str(cfg_path), '--synthetic', '2',
               '--log_dir', str(tmp_path / tag / 'log'), '--seed', '3']
        release_gpu_memory()                     # the child needs the card's memory, not this process's cache
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=150)
        assert r.returncode == 0, r.stderr[-3000:]
        runs = os.listdir(tmp_path / tag / 'log')
        assert len(runs) == 1
        saved[tag] = tmp_path / tag / 'log' / runs[0] / '00000_ckpt.pth.tar'
        cfgs[tag] = cfg
    base = {'unsup_model', 'unsup_disc', 'epochs', 'optimizer_detector', 'optimizer_discriminator'}
    assert set(torch.load(saved['off'], map_location='cpu')) == base
    sd = torch.load(saved['ema'], map_location='cpu')
    assert set(sd) == base | {'unsup_model_ema'}
    live, ema = sd['unsup_model'], sd['unsup_model_ema']
    assert list(ema) == list(live)

    # resume in this process, the way the entry does: Trainer._load_checkpoint
    monkeypatch.setenv('LOCAL_RANK', '0')
    import train as xtrain
    from xas_amd import engine
    cfg = cfgs['ema']
    cfg['model_params']['cam_id_list'] = cfg['dataset_params']['cam_id_list']          # train.py main()
    nets = engine.prepare_model(cfg)
    trainer = xtrain.Trainer(cfg, nets[0], nets[1], [], nets[2], str(tmp_path), checkpoint_path=str(saved['ema']),
                             optimizer_discriminator=nets[3], mode='train')
    opt = trainer.optimizer_detector
    names = trainer._ema_param_names()
    params = set(names)
    assert params <= {n for n, _ in nets[0].named_parameters()} and len(names) == len(opt.ema_views()) > 100
    for k in live:
        if k in params:
            assert ema[k].shape == live[k].shape
        else:
            assert torch.equal(ema[k], live[k]), k              # buffers: those of the live model
    differ = [k for k in names if not torch.equal(ema[k], live[k])]
    assert 'regressor.net.backbone.conv1.weight' in differ and 'physique_network.encoder.0.0.weight' in differ
    assert len(differ) > len(names) // 2, (len(differ), len(names))
    for n, v, p in zip(names, opt.ema_views(), opt.arena_params()):
        assert torch.equal(v.cpu(), ema[n]), n                   # the shadow: bit for bit the checkpoint's
        assert torch.equal(p.detach().cpu(), live[n]), n

    # a checkpoint whose entry lacks a parameter: refused, never a mix of averaged and raw weights
    partial = dict(sd, unsup_model_ema={k: v for k, v in ema.items() if k != names[3]})
    with monkeypatch.context() as mp:
        mp.setattr(torch, 'load', lambda *a, **k: partial)
        with pytest.raises(KeyError, match=names[3].replace('.', '[.]')):
            trainer._load_checkpoint(str(saved['ema']), 'train')

    # a checkpoint without the key: the shadow starts from the loaded parameters
    nets = engine.prepare_model(cfg)
    trainer = xtrain.Trainer(cfg, nets[0], nets[1], [], nets[2], str(tmp_path), checkpoint_path=str(saved['off']),
                             optimizer_discriminator=nets[3], mode='finetune')
    opt = trainer.optimizer_detector
    assert torch.equal(opt.ema_arena, opt.param_arena)
    del trainer, nets, opt

    # eval.py's model preparation
    import eval as xeval
    det = xeval.prepare_model(cfg, argparse.Namespace(checkpoint=str(saved['ema']), ema=True))
    got = det.state_dict()
    assert got and all(torch.equal(v, ema['regressor.' + k]) for k, v in got.items())
    assert not torch.equal(got['net.backbone.conv1.weight'], live['regressor.net.backbone.conv1.weight'])
    det = xeval.prepare_model(cfg, argparse.Namespace(checkpoint=str(saved['ema']), ema=False))
    assert torch.equal(det.state_dict()['net.backbone.conv1.weight'], live['regressor.net.backbone.conv1.weight'])
    with pytest.raises(KeyError, match='unsup_model_ema'):
        xeval.prepare_model(cfg, argparse.Namespace(checkpoint=str(saved['off']), ema=True))
