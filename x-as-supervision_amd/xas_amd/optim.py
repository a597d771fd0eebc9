"""Fused Adam over flat arenas (reference: two torch.optim.Adam(betas=(0.5, 0.999)) at train.py:257-264).

Parameters of one optimizer are re-homed into ONE contiguous fp32 arena (each nn.Parameter becomes a view),
gradients into a second arena (`.grad` views, so autograd accumulates in place), moments into two more.
`step()` is one kernel launch over the arena (csrc/optim.hip: one kernel template for the plain, guarded and averaged
forms); `zero_grad()` is one memset.  The contiguous gradient arena
is also what the data-parallel reducer all-reduces in large buckets (xas_amd/dp.py).
state_dict()/load_state_dict() speak torch.optim.Adam's format so reference checkpoints resume.

Guarded step (opt-in: `max_grad_norm` and / or `skip_nonfinite`): `step()` is then two enqueues, `xas_grad_guard` (one read
of the gradient arena: its L2 norm, the clipping scale of torch.nn.utils.clip_grad_norm_, and whether a non-finite gradient
makes this a step to skip) and `xas_adam_step_guarded` (the same update on g * scale; a skipped step stores nothing).  The
decision and the count of APPLIED steps live in a small guard record on the device (include/xas_hip.h), so a skipped step
costs no synchronisation and does not advance the bias correction - as if step() had not been called.

Averaged weights (opt-in: `ema_decay`): one more arena, the shadow, holds an exponential moving average of the parameters.  It
starts as a copy of the parameter arena (so it needs no bias correction and no warm-up of the decay) and `step()` maintains it in
the launch that writes the parameters - `xas_adam_step_ema` / `xas_adam_step_guarded_ema` in place of the plain entry points, the
same number of enqueues: ema = fmaf(decay, ema, (1 - decay) * p_new) per element, and a skipped step leaves it alone.  The
shadow is not part of state_dict() (which stays torch.optim.Adam's): `ema_views()` / `load_ema()` carry it to and from a
checkpoint, `averaged()` puts it in the parameters' place for an evaluation.  A parameter whose storage was replaced (module.to(),
a load onto new storage) is re-homed into the parameter arena as always; its shadow slot keeps the value it had.
Data parallel: nothing to exchange per step.  engine.TrainStep broadcasts rank 0's shadow once, right after rank 0's parameters
(the arenas are built before that broadcast, so until then a rank's shadow is a copy of ITS OWN initial parameters; a shadow
restored from a checkpoint is rank 0's as well and survives).  From there on the parameters are identical on every rank after the
all-reduced step and the shadow update is elementwise and deterministic, so the shadows stay identical too.
"""
import contextlib
import ctypes
import math

import torch

from . import _lib, ops_nn
from ._lib import ptr


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False,
                 ema_decay=None):
        params = list(params)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        if len(self.param_groups) != 1:
            raise ValueError('FusedAdam updates one flat arena with one set of hyper-parameters: pass a single param group')
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError('FusedAdam: max_grad_norm must be positive (None = no clipping), got %r' % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None or math.isinf(float(max_grad_norm)) else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self._ema_factors = None             # (decay, 1 - decay) as the fp32 values the kernels take
        if ema_decay is not None:
            d = ctypes.c_float(self.ema_decay).value                      # (0.99999999 is 1.0f: no average at all)
            if not 0.0 <= d < 1.0:
                raise ValueError('FusedAdam: ema_decay must be in [0, 1) as fp32 (None = no averaged weights), got %r' % (ema_decay,))
            self._ema_factors = (d, ctypes.c_float(1.0 - d).value)        # 1 - decay: rounded once, from double
        self._averaged = False               # inside averaged(): the parameter arena holds the shadow
        self._flat = None
        self._steps = 0
        self._epoch = [0]            # bumped whenever this optimizer rewrites its parameters (ops_nn._PackCache key)

    # ---- arenas -------------------------------------------------------------------------------------
    def _build(self):
        ps = [p for g in self.param_groups for p in g['params']]
        if not ps:
            raise RuntimeError('FusedAdam: no parameters')
        dev = ps[0].device
        if dev.type != 'cuda':
            raise RuntimeError('FusedAdam runs on the GPU only (move the model first); no CPU fallback')
        offs, n = [], 0
        for p in ps:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4                  # 16-byte aligned slots
        arena = torch.zeros(n, device=dev, dtype=torch.float32)
        grads = torch.zeros(n, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for p, o in zip(ps, offs):
                v = arena[o:o + p.numel()].view(p.shape)
                v.copy_(p.data)
                p.data = v
                g = grads[o:o + p.numel()].view(p.shape)
                if p.grad is not None:
                    g.copy_(p.grad)
                p.grad = g
        self._flat = dict(params=ps, offs=offs, n=n, p=arena, g=grads, m=torch.zeros_like(arena), v=torch.zeros_like(arena))
        if self.guarded:
            rec = torch.zeros(_lib.GUARD_FLOATS, device=dev, dtype=torch.float32)       # the guard record (xas_hip.h)
            rec_i = rec.view(torch.int32)
            rec_i[_lib.GUARD_T] = self._steps
            ws = torch.empty((_lib.query('xas_grad_guard_workspace_bytes', n) + 7) // 8, device=dev, dtype=torch.float64)
            self._flat.update(guard=rec, guard_i=rec_i, guard_ws=ws)
        if self.ema_decay is not None:
            self._flat['ema'] = arena.clone()                                           # the shadow starts at the parameters
        for p in ps:
            p._xas_epoch = self._epoch
        self._epoch[0] += 1

    @property
    def grad_arena(self):
        if self._flat is None:
            self._build()
        return self._flat['g']

    @property
    def param_arena(self):
        if self._flat is None:
            self._build()
        return self._flat['p']

    def arena_params(self):
        """The parameters in arena order: the order of ema_views() and of the list load_ema() takes."""
        if self._flat is None:
            self._build()
        return list(self._flat['params'])

    @property
    def ema_arena(self):
        """The shadow arena (laid out like param_arena), None without `ema_decay`."""
        if self.ema_decay is None:
            return None
        if self._flat is None:
            self._build()
        return self._flat['ema']

    def ema_views(self):
        """The averaged weights: tensors shaped like the parameters, in parameter order, views of the shadow arena."""
        e = self.ema_arena
        if e is None:
            raise RuntimeError('FusedAdam: no averaged weights (ema_decay is None)')
        f = self._flat
        return [e[o:o + p.numel()].view(p.shape) for p, o in zip(f['params'], f['offs'])]

    @torch.no_grad()
    def load_ema(self, tensors):
        """Copy a list like ema_views() (e.g. from a checkpoint) into the shadow arena."""
        views, tensors = self.ema_views(), list(tensors)
        if len(tensors) != len(views):
            raise ValueError('FusedAdam.load_ema: %d tensors for %d parameters' % (len(tensors), len(views)))
        if self._averaged:
            raise RuntimeError('FusedAdam.load_ema inside averaged(): the shadow arena holds the parameters there')
        for v, t in zip(views, tensors):
            v.copy_(t)

    @contextlib.contextmanager
    def averaged(self):
        """Inside the context the parameters hold the averaged weights (and the shadow the trained ones): the contents of the
        two arenas are exchanged on entry and again on exit.  Checkpoint / evaluation time, not the step: plain copies through
        one temporary.  step() raises inside."""
        if self.ema_arena is None:
            raise RuntimeError('FusedAdam: no averaged weights (ema_decay is None)')
        if self._averaged:
            raise RuntimeError('FusedAdam.averaged() does not nest')
        self._swap_ema()
        self._averaged = True
        try:
            yield self
        finally:
            self._averaged = False
            self._swap_ema()

    @torch.no_grad()
    def _swap_ema(self):
        self._check_views()                      # a parameter on storage of its own joins the arena before the exchange
        f = self._flat
        tmp = f['p'].clone()
        f['p'].copy_(f['ema'])
        f['ema'].copy_(tmp)
        self._epoch[0] += 1                      # packed / split weight copies (ops_nn) are stale

    def _guard_word(self, i, as_int=False):
        if not self.guarded:
            return None
        if self._flat is None:
            self._build()
        return self._flat['guard_i' if as_int else 'guard'][i]

    @property
    def grad_norm(self):
        """0-dim device tensor, a view of the guard record: L2 norm of the gradient arena as the last step() saw it (before
        clipping).  None without the guard."""
        return self._guard_word(_lib.GUARD_NORM)

    @property
    def skipped_steps(self):
        """0-dim device int32 tensor (view): step() calls skipped so far because of a non-finite gradient.  None without the
        guard."""
        return self._guard_word(_lib.GUARD_SKIPPED, as_int=True)

    def _check_views(self):
        """Re-home parameters and gradients whose storage was replaced.  The shadow arena is not touched: the slot of a re-homed
        parameter keeps its average."""
        f = self._flat
        for p, o in zip(f['params'], f['offs']):
            if p.data_ptr() != f['p'].data_ptr() + 4 * o:           # e.g. after module.to()/load onto new storage
                with torch.no_grad():
                    v = f['p'][o:o + p.numel()].view(p.shape)
                    v.copy_(p.data)
                    p.data = v
                self._epoch[0] += 1
            if p.grad is None:
                p.grad = f['g'][o:o + p.numel()].view(p.shape)
            elif p.grad.data_ptr() != f['g'].data_ptr() + 4 * o:
                with torch.no_grad():
                    g = f['g'][o:o + p.numel()].view(p.shape)
                    g.copy_(p.grad)
                    p.grad = g

    # ---- optimizer API ------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        if self._averaged:
            raise RuntimeError('FusedAdam.step() inside averaged(): the parameter arena holds the averaged weights')
        if self._flat is None:
            self._build()
        ops_nn.join_side_stream()                    # weight gradients accumulated on the side stream
        self._check_views()
        f = self._flat
        g0 = self.param_groups[0]
        self._steps += 1
        b1, b2 = g0['betas']
        ema = self._ema_factors
        if not self.guarded:
            if ema is None:
                _lib.call('xas_adam_step', ptr(f['p']), ptr(f['g']), ptr(f['m']), ptr(f['v']), f['n'], float(g0['lr']),
                          float(b1), float(b2), float(g0['eps']), self._steps)
            else:
                _lib.call('xas_adam_step_ema', ptr(f['p']), ptr(f['g']), ptr(f['m']), ptr(f['v']), ptr(f['ema']), f['n'],
                          float(g0['lr']), float(b1), float(b2), float(g0['eps']), self._steps, ema[0], ema[1])
        else:        # (self._steps counts the calls here; the steps APPLIED are counted on the device)
            _lib.call('xas_grad_guard', ptr(f['g']), f['n'], float(self.max_grad_norm or 0.0), int(self.skip_nonfinite),
                      float(g0['lr']), float(b1), float(b2), ptr(f['guard']), ptr(f['guard_ws']))
            if ema is None:
                _lib.call('xas_adam_step_guarded', ptr(f['p']), ptr(f['g']), ptr(f['m']), ptr(f['v']), f['n'], float(b1),
                          float(b2), float(g0['eps']), ptr(f['guard']))
            else:
                _lib.call('xas_adam_step_guarded_ema', ptr(f['p']), ptr(f['g']), ptr(f['m']), ptr(f['v']), ptr(f['ema']),
                          f['n'], float(b1), float(b2), float(g0['eps']), ema[0], ema[1], ptr(f['guard']))
        self._epoch[0] += 1          # packed weight copies of THIS optimizer's parameters are stale now

    def zero_grad(self, set_to_none=False):
        """One memset of the gradient arena.  `set_to_none` is ignored on purpose: .grad must stay a view of the arena
        (kernels accumulate into it by pointer)."""
        if self._flat is None:
            self._build()
        ops_nn.join_side_stream()
        self._check_views()
        self._flat['g'].zero_()

    def state_dict(self):
        """torch.optim.Adam layout: state[i] = {step, exp_avg, exp_avg_sq}."""
        if self._flat is None:
            self._build()
        f = self._flat
        steps = int(f['guard_i'][_lib.GUARD_T]) if self.guarded else self._steps      # guarded: the steps applied
        state = {}
        for i, (p, o) in enumerate(zip(f['params'], f['offs'])):
            state[i] = {'step': torch.tensor(float(steps)),
                        'exp_avg': f['m'][o:o + p.numel()].view(p.shape).clone(),
                        'exp_avg_sq': f['v'][o:o + p.numel()].view(p.shape).clone()}
        groups = [{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups]
        idx = 0
        for g, pg in zip(groups, self.param_groups):
            g['params'] = list(range(idx, idx + len(pg['params'])))
            idx += len(pg['params'])
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, sd):
        if self._flat is None:
            self._build()
        f = self._flat
        for g, sg in zip(self.param_groups, sd['param_groups']):
            for k in ('lr', 'betas', 'eps', 'initial_lr'):
                if k in sg:
                    g[k] = sg[k]
        steps = set()
        with torch.no_grad():
            for i, (p, o) in enumerate(zip(f['params'], f['offs'])):
                st = sd['state'].get(i, sd['state'].get(str(i)))
                if st is None:
                    continue
                f['m'][o:o + p.numel()].view(p.shape).copy_(st['exp_avg'])
                f['v'][o:o + p.numel()].view(p.shape).copy_(st['exp_avg_sq'])
                steps.add(int(float(st['step'])))
        if len(steps) > 1:
            raise ValueError('FusedAdam keeps ONE step counter for the arena; the checkpoint has per-parameter steps %s' % sorted(steps))
        if steps:
            self._steps = steps.pop()
            if self.guarded:
                f['guard_i'][_lib.GUARD_T] = self._steps
