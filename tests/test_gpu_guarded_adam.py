"""Guarded FusedAdam step (on-device gradient norm, clipping, non-finite skip) against torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam on float64 CPU copies of the same fp32 values.

Arena sizes: one float4 (255 idle threads), ragged against 256 x 4, the odd parameter shapes of test_fused_adam_vs_torch (an
arena with zero-padded slots) and 4096 * 256 * 4 + 4 (the grid cap reached, exactly one float4 goes round the grid-stride loop).

Bounds.
* Norm: 1 ulp of fp32 around the float64 norm rounded to fp32 - every sum is accumulated in double, the only fp32 rounding is
  the final conversion (the double sums' own error, ~1e-16 * sqrt(n) relative, can move that rounding by one ulp at most).
* Parameters, moments: 2e-7 max-abs, the bar of test_fused_adam_vs_torch for the same shapes and learning rate.  Against a
  float64 oracle an fp32 value x carries its storage rounding, up to 2^-24 |x| per step, whatever kernel wrote it: three steps
  stay under 2e-7 only for |x| < 1.1 or so.  The bar is about the update arithmetic, so the values the test chooses keep the
  storage rounding under it: initial parameters uniform in (-1, 1) (trained weights are far inside; the default arithmetic of the
  convolutions needs |w| < 64 anyway); where the moments are compared the gradients are uniform in (-1, 1) times the scale
  (|m| < 2.1: at most 1.75 * 2^-24 * 2 = 2.1e-7 in the very worst case of three same-sign roundings, 6e-8 typically); v = O(1e-3).
  The gradient scales 0.1 + it and, for the clipped steps, normal gradients are those of test_fused_adam_vs_torch.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

LR, BETAS, BAR = 2e-4, (0.5, 0.999), 2e-7
SIZES = {'n4': [(4,)], 'n1028': [(1028,)], 'odd': [(64, 3, 7, 7), (64,), (17, 5), (1,), (128, 64, 3, 3)],
         'cap': [(4096 * 256 * 4 + 4,)]}
ARENA = {'n4': 4, 'n1028': 1028, 'odd': 9408 + 64 + 88 + 4 + 73728, 'cap': 4096 * 256 * 4 + 4}


def _word(opt, i, as_int=False):
    return opt._flat['guard_i' if as_int else 'guard'][i].item()


def _rec(opt):
    from xas_amd import _lib
    return {'norm': _word(opt, _lib.GUARD_NORM), 'scale': _word(opt, _lib.GUARD_SCALE), 'skip': _word(opt, _lib.GUARD_SKIP, True),
            't': _word(opt, _lib.GUARD_T, True), 'skipped': _word(opt, _lib.GUARD_SKIPPED, True)}


def _uniform(shape, g):
    return torch.rand(shape, generator=g) * 2 - 1


def _make(size, seed=0, **guard):
    """-> generator, device parameters + FusedAdam, float64 CPU copies + torch.optim.Adam."""
    from xas_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(seed)
    ps = [_uniform(s, g) for s in SIZES[size]]
    a = [nn.Parameter(p.clone().cuda()) for p in ps]
    b = [nn.Parameter(p.clone().double()) for p in ps]
    oa = FusedAdam(a, lr=LR, betas=BETAS, **guard)
    ob = torch.optim.Adam(b, lr=LR, betas=BETAS)
    oa.zero_grad()
    assert oa._flat['n'] == ARENA[size]
    return g, a, oa, b, ob


def _set_grads(a, b, grads):
    for pa, pb, gr in zip(a, b, grads):
        pa.grad.copy_(gr.cuda())
        pb.grad = gr.double().clone()


def _norm64(grads):
    return float(torch.cat([gr.double().reshape(-1) for gr in grads]).norm())


def _ulps(got, ref64):
    ref32 = np.float32(ref64)
    return abs(float(np.float32(got)) - float(ref32)) / float(np.spacing(ref32))


def _dist(xs, ys):
    return max(float((x.detach().cpu().double() - y.detach().double()).abs().max()) for x, y in zip(xs, ys))


def _moments(oa, ob, b, key):
    sa, sb = oa.state_dict()['state'], ob.state_dict()['state']
    return [sa[i][key] for i in range(len(b))], [sb[i][key] for i in range(len(b))]


@pytest.mark.parametrize('size', list(SIZES))
def test_norm_is_the_float64_norm_and_reproducible(size):
    g, a, oa, b, ob = _make(size, skip_nonfinite=True)
    grads = [torch.randn(s, generator=g) * 1.7 for s in SIZES[size]]
    _set_grads(a, b, grads)
    oa.step()
    n1 = oa.grad_norm.clone()
    oa.step()                                       # the same arena again (nothing zeroed it)
    n2 = oa.grad_norm.clone()
    assert oa.grad_norm.dim() == 0 and oa.grad_norm.is_cuda and oa.grad_norm.dtype == torch.float32
    ref = _norm64(grads)
    print('%s: norm %.9g, float64 %.17g, %.2f ulp' % (size, float(n1), ref, _ulps(float(n1), ref)))
    assert _ulps(float(n1), ref) <= 1.0
    assert n1.view(torch.int32).item() == n2.view(torch.int32).item()
    r = _rec(oa)
    assert r['skip'] == 0 and r['t'] == 2 and r['skipped'] == 0 and r['scale'] == 1.0


@pytest.mark.parametrize('size', list(SIZES))
def test_clipped_steps_vs_float64(size):
    """Step 0 passes unclipped (scale == 1.0f exactly), steps 1 and 2 are clipped: max_grad_norm is the geometric mean of the
    float64 norms of step 0 and of the smaller of the other two."""
    g = torch.Generator().manual_seed(1)
    steps = [[torch.randn(s, generator=g) * (0.1 + it) for s in SIZES[size]] for it in range(3)]
    norms = [_norm64(gr) for gr in steps]
    max_norm = float(np.float32(np.sqrt(norms[0] * min(norms[1:]))))       # (a value fp32 holds exactly: the ABI takes a float)
    assert norms[0] * 1.01 < max_norm < min(norms[1:]) / 1.01, norms
    _, a, oa, b, ob = _make(size, max_grad_norm=max_norm)
    for it, grads in enumerate(steps):
        _set_grads(a, b, grads)
        oa.step()
        r = _rec(oa)
        assert _ulps(r['norm'], norms[it]) <= 1.0
        if it == 0:
            assert r['scale'] == 1.0
        else:
            # computed in double on the device, rounded once to fp32: 2^-24 = 6e-8 relative
            assert abs(r['scale'] / (max_norm / (norms[it] + 1e-6)) - 1) < 1e-7 and r['scale'] < 1.0
        assert r['skip'] == 0 and r['t'] == it + 1
        total = torch.nn.utils.clip_grad_norm_(b, max_norm)
        assert abs(float(total) - norms[it]) < 1e-12 * norms[it]
        ob.step()
        oa.zero_grad()
    d = _dist(a, b)
    print('%s: clipped, parameters %.3g from float64' % (size, d))
    assert d < BAR


@pytest.mark.parametrize('size', list(SIZES))
def test_unclipped_guarded_steps_vs_float64(size):
    g, a, oa, b, ob = _make(size, seed=2, skip_nonfinite=True)
    for it in range(3):
        _set_grads(a, b, [_uniform(s, g) * (0.1 + it) for s in SIZES[size]])
        oa.step()
        ob.step()
        r = _rec(oa)
        assert r['scale'] == 1.0 and r['skip'] == 0 and r['t'] == it + 1 and r['skipped'] == 0
    dp, dm, dv = _dist(a, b), _dist(*_moments(oa, ob, b, 'exp_avg')), _dist(*_moments(oa, ob, b, 'exp_avg_sq'))
    print('%s: unclipped, p %.3g  m %.3g  v %.3g from float64' % (size, dp, dm, dv))
    assert dp < BAR and dm < BAR and dv < BAR
    assert float(oa.state_dict()['state'][0]['step']) == 3.0


def _plant(kind):
    def plant(grads):
        if kind == 'nan_last':
            grads[-1].view(-1)[-1] = float('nan')            # the last real element of the arena
        else:
            grads[0].view(-1)[0] = float('inf')
        return grads
    return plant


@pytest.mark.parametrize('size', list(SIZES))
@pytest.mark.parametrize('kind', ['nan_last', 'inf_first'])
def test_nonfinite_gradient_skips_the_step(size, kind):
    """step, skip, step: the skipped call leaves p, m, v bit for bit and t alone; the step after it equals a float64 Adam that
    never saw the skipped one (its bias correction uses t = 2, not the number of calls)."""
    g, a, oa, b, ob = _make(size, seed=3, skip_nonfinite=True)
    f = oa._flat
    _set_grads(a, b, [_uniform(s, g) * 0.6 for s in SIZES[size]])
    oa.step()
    ob.step()
    before = [f[k].clone() for k in ('p', 'm', 'v')]
    assert _rec(oa)['t'] == 1
    bad = _plant(kind)([_uniform(s, g) * 0.6 for s in SIZES[size]])
    for pa, gr in zip(a, bad):
        pa.grad.copy_(gr.cuda())
    epoch = oa._epoch[0]
    oa.step()
    r = _rec(oa)
    assert r['skip'] == 1 and r['skipped'] == 1 and r['t'] == 1
    assert int(oa.skipped_steps) == 1 and oa.skipped_steps.is_cuda
    for k, x in zip(('p', 'm', 'v'), before):
        assert torch.equal(f[k], x), k
    assert oa._epoch[0] == epoch + 1                          # the re-pack after a skipped step is harmless and unconditional
    _set_grads(a, b, [_uniform(s, g) * 1.1 for s in SIZES[size]])
    oa.step()
    ob.step()
    r = _rec(oa)
    assert r['skip'] == 0 and r['skipped'] == 1 and r['t'] == 2
    dp, dm, dv = _dist(a, b), _dist(*_moments(oa, ob, b, 'exp_avg')), _dist(*_moments(oa, ob, b, 'exp_avg_sq'))
    print('%s %s: after step, skip, step: p %.3g  m %.3g  v %.3g from float64' % (size, kind, dp, dm, dv))
    assert dp < BAR and dm < BAR and dv < BAR
    assert float(oa.state_dict()['state'][0]['step']) == 2.0


@pytest.mark.parametrize('size', ['n4', 'odd'])
def test_sum_of_squares_beyond_fp32_is_no_reason_to_skip(size):
    """|g| = 1.5e19 everywhere: the sum of squares (>= 9e38) overflows fp32, the norm (>= 3e19) does not."""
    g, a, oa, b, ob = _make(size, seed=4, skip_nonfinite=True)
    grads = [torch.sign(_uniform(s, g)) * 1.5e19 for s in SIZES[size]]
    assert not np.isfinite(np.float32(sum(float((gr.double() ** 2).sum()) for gr in grads)))
    _set_grads(a, b, grads)
    oa.step()
    ob.step()
    r = _rec(oa)
    assert np.isfinite(r['norm']) and _ulps(r['norm'], _norm64(grads)) <= 1.0
    assert r['skip'] == 0 and r['skipped'] == 0 and r['t'] == 1 and r['scale'] == 1.0
    assert _dist(a, b) < BAR


def test_default_launches_only_the_plain_step(monkeypatch):
    from xas_amd import _lib
    from xas_amd.optim import FusedAdam
    a = [nn.Parameter(torch.ones(5, 3).cuda())]
    oa = FusedAdam(a, lr=LR, betas=BETAS)
    oa.zero_grad()
    a[0].grad.fill_(0.25)
    names, orig = [], _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *args: (names.append(name), orig(name, *args))[1])
    oa.step()
    oa.step()
    assert names == ['xas_adam_step', 'xas_adam_step']
    assert oa.grad_norm is None and oa.skipped_steps is None and 'guard' not in oa._flat
    names.clear()
    ob = FusedAdam([nn.Parameter(torch.ones(5, 3).cuda())], lr=LR, betas=BETAS, max_grad_norm=1.0)
    ob.zero_grad()
    ob.step()
    assert names == ['xas_grad_guard', 'xas_adam_step_guarded']


def test_state_dict_counts_applied_steps_and_load_restores_them():
    from xas_amd import _lib
    from xas_amd.optim import FusedAdam
    mk = lambda: FusedAdam([nn.Parameter(torch.full((6,), 0.5).cuda())], lr=LR, betas=BETAS, skip_nonfinite=True, max_grad_norm=10.0)
    oa = mk()
    oa.zero_grad()
    p = oa._flat['params'][0]
    for val in (0.25, float('nan'), -0.5):                   # step, skip, step
        p.grad.fill_(val)
        oa.step()
    sd = oa.state_dict()
    assert float(sd['state'][0]['step']) == 2.0
    ob = mk()
    ob.load_state_dict(sd)
    assert _word(ob, _lib.GUARD_T, True) == 2 and _word(ob, _lib.GUARD_SKIPPED, True) == 0
    with torch.no_grad():
        ob._flat['p'].copy_(oa._flat['p'])
    for o in (oa, ob):                                        # the resumed optimizer continues at t = 3, like the original
        o._flat['params'][0].grad.fill_(0.125)
        o.step()
    assert torch.equal(oa._flat['p'], ob._flat['p']) and _word(ob, _lib.GUARD_T, True) == 3
