"""Soft-argmax head on the launch paths that tests/test_gpu_head.py and tests/test_gpu_head_sizes.py do not reach: joint
tiles over gridDim.z (exact, ragged, the widest single tile), two depth bins per lane just above D = 64, the tie rule at
D = 128, more hypotheses than peaks, D = 4 and power-of-two sides too wide for one block, the second pass alone over records
built on the host, and logits of the magnitude a trained final layer with bias produces.

Inputs: table EDGES of tests/golden/head_sizes_inputs.py; golden `head_edges.npz` (tests/golden/make_golden_head_sizes.py).
Bars: the rule of tests/test_gpu_head_sizes.py - within 4 x the reference's own float32 deviation from float64 (`dev_*`) of
the float64 restatement, evaluated here on the device, and within 5 x of the float32 golden; the gradient relative to the
float64 gradient's maximum.  Peak indices: bit for bit against float64 for every joint.  Against the golden as well, except
the joints of `edge_unordered` - the exact tie of tie128 (torch.topk returns the higher of two equal bins first at that size)
and the one-peak joints of h6 (five equal zero scores: topk returned bins 13..18) - whose order the reference does not
define: those joints are left out of every golden comparison and are held to float64 and to the literal lists instead."""
import functools

import numpy as np
import pytest
import torch

import head_sizes_inputs as hs
from conftest import golden

gpu = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
ALL = list(hs.EDGES)
# (case, policy): every case as shipped; D = 4 also with every power-of-two side on the general policy (only K = 4 changes)
RUNS = [(n, 'shipped') for n in ALL] + [(n, 'general') for n in hs.E4]


@functools.lru_cache(maxsize=None)
def G():
    return golden('head_edges')


def restated(lg, gw, K, hy, nb, dtype=torch.float64):
    """The restatement and its autograd gradient in `dtype` on the device of lg."""
    l = lg.to(dtype).contiguous().requires_grad_(True)
    k, pz, idx = hs.restate(l, K, hy, nb)
    (k * gw.to(dtype)).sum().backward()
    return {'kps': k.detach(), 'pz': pz.detach(), 'idx': idx, 'grad': l.grad, 'gmax': float(l.grad.abs().max())}


@functools.lru_cache(maxsize=None)
def case(name):
    """Logits on the device (NHWC storage) and the float64 restatement with its gradient: computed once, never modified."""
    D, K, B, hy, nb, seed = hs.spec(name)
    lg = T(hs.edge_logits(name) if name in hs.EDGES else hs.logits(name)).cuda().contiguous(memory_format=torch.channels_last)
    gw = T(hs.grad_kps(name)).cuda()
    c = restated(lg, gw, K, hy, nb)
    keep = torch.ones(B, K, dtype=torch.bool, device='cuda')       # joints whose hypothesis order the reference defines
    for b, k in hs.edge_unordered(name):
        keep[b, k] = False
    c.update(lg=lg, gw=gw, keep=keep)
    return c


def err(a, b, mask=None):
    d = (a.detach().double().cpu() - b.detach().double().cpu()).abs()
    return float((d * mask.cpu()).max() if mask is not None else d.max())


def check(name, group, e64, eg, what):
    d = float(G()['%s_dev_%s' % (name, group)])
    print('%s %s %s: |hip - f64| %.3e (bar %.3e)  |hip - golden| %.3e (bar %.3e)' % (name, what, group, e64, 4 * d, eg, 5 * d))
    assert e64 <= 4 * d, '%s %s %s: %.3e from float64, bar %.3e' % (name, what, group, e64, 4 * d)
    assert eg <= 5 * d, '%s %s %s: %.3e from the golden, bar %.3e' % (name, what, group, eg, 5 * d)


def policy(which):
    from xas_amd import _lib
    _lib.query('xas_set_tuning', _lib.TUNE_GENERAL_KERNELS if which == 'general' else 0)    # (conftest resets it after the test)


def forward(name, lg=None):
    from xas_amd import ops_head
    D, K, B, hy, nb, seed = hs.spec(name)
    lg = case(name)['lg'] if lg is None else lg
    if nb:
        return ops_head.softargmax_multi(lg, K, hy, nb)
    kps, dmap = ops_head.softargmax_single(lg, K)
    return kps, dmap, None


def backward(name, lg=None, gw=None):
    """-> (kps, grad_logits through autograd)."""
    c = case(name)
    lg = (c['lg'] if lg is None else lg).detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    kps, _, _ = forward(name, lg=lg)
    (kps * (c['gw'] if gw is None else gw)).sum().backward()
    return kps.detach(), lg.grad


# ------------------------------------------------------------------ every case, forward and backward
@gpu
@pytest.mark.parametrize('name,which', RUNS)
def test_forward_vs_golden_and_float64(name, which):
    D, K, B, hy, nb, seed = hs.EDGES[name]
    c, g = case(name), G()
    policy(which)
    kps, dmap, idx = forward(name)
    assert kps.shape == (B, hy, K, 3) and dmap.shape == (K, D)
    keep = c['keep']
    if nb:
        assert idx.dtype == torch.int64 and idx.shape == (B, K, hy)
        assert torch.equal(idx, c['idx'])                       # every joint, ties and fill-ins included
        assert torch.equal(idx[keep].cpu(), T(g[name + '_z_peak_indices'])[keep.cpu()])
        for (b, k), want in hs.edge_expected(name).items():
            assert idx[b, k].tolist() == want, (name, b, k, idx[b, k].tolist(), want)
    check(name, 'kps', err(kps, c['kps']), err(kps, T(g[name + '_kps']), keep.view(B, 1, K, 1)), 'forward')
    check(name, 'dmap', err(dmap, c['pz'][0]), err(dmap, T(g[name + '_depth_prob_map'])), 'forward')


@gpu
@pytest.mark.parametrize('name,which', RUNS)
def test_backward_vs_golden_and_float64(name, which):
    D, K, B, hy, nb, seed = hs.EDGES[name]
    c, g = case(name), G()
    policy(which)
    _, grad = backward(name)
    assert grad.shape == c['lg'].shape
    e64 = err(grad, c['grad']) / c['gmax']
    kg = c['keep'].view(B, K, 1, 1, 1).expand(B, K, D, D, D).reshape(-1)[::hs.GRAD_STRIDE]
    sub = grad.contiguous().reshape(-1)[::hs.GRAD_STRIDE]
    eg = err(sub, T(g[name + '_grad_logits_sub']), kg) / c['gmax']
    check(name, 'grad', e64, eg, 'backward')
    d = float(g[name + '_dev_grad'])
    amax = float((grad.contiguous().view(B, K, D, D, D) * c['keep'].view(B, K, 1, 1, 1)).abs().max())
    ea = abs(amax - float(g[name + '_grad_amax'])) / c['gmax']
    assert ea <= 5 * d, '%s: max |grad| %.3e from the golden (relative), bar %.3e' % (name, ea, 5 * d)


@gpu
@pytest.mark.parametrize('name', ['t12c', 't68'])
def test_recorded_maximum_equals_the_gradient_maximum(name):
    """xas_head_softargmax_bwd_amax with joint tiles (the block index that selects the sub-maximum has a gridDim.z term)."""
    from xas_amd import ops_head, ops_nn
    from xas_amd._lib import call, ptr
    D, K, B, hy, nb, seed = hs.EDGES[name]
    c = case(name)
    lg = c['lg']
    kps = torch.empty(B, hy, K, 3, device='cuda')
    z_idx = torch.empty(B, K, hy, device='cuda', dtype=torch.int64)
    dmap = torch.empty(1, K, D, device='cuda')
    stats = torch.empty(B, K, ops_head.HEAD_STATS, device='cuda')
    ws = torch.empty(ops_head.query('xas_head_workspace_floats', B, K, D), device='cuda')
    call('xas_head_softargmax_fwd', ptr(lg), B, K, D, hy, nb, ptr(kps), ptr(z_idx), ptr(dmap), 1, ptr(stats), ptr(ws))
    grad = torch.empty_like(lg)
    coef = torch.empty(B * K * (4 + D), device='cuda')
    slot = torch.zeros(ops_nn.AMAX_SLOT_FLOATS, device='cuda')
    call('xas_head_softargmax_bwd_amax', ptr(lg), ptr(stats), ptr(z_idx), ptr(c['gw']), B, K, D, hy, nb, ptr(grad), ptr(coef),
         ptr(slot))
    assert float(slot.max()) == float(grad.abs().max()) > 0.0
    assert int((slot != 0).sum()) <= 32                                   # one sub-maximum per 128 bytes, nothing else written
    assert torch.equal(grad, backward(name)[1])                           # the same launch as the autograd op's


# ------------------------------------------------------------------ pass 2 alone
def host_records(lg):
    """[B, K*D, H, W] float32 logits -> float32 records [B][nchunk][K][3 + D] of 64 pixels each, computed in float64 and
    rounded once: chunk maximum (a logit: exact), sum e*w, sum e*h, sum e per depth bin, e = exp(v - chunk maximum)."""
    B, C, H, W = lg.shape
    D = H
    K = C // D
    v = lg.double().reshape(B, K, D, H * W)
    n = -(-H * W // 64)
    pix = torch.arange(H * W, device=lg.device)
    fw, fh = (pix % W).double(), (pix // W).double()
    rec = torch.zeros(B, n, K, 3 + D, dtype=torch.float64, device=lg.device)
    for c in range(n):
        s = slice(64 * c, min(64 * c + 64, H * W))
        m = v[..., s].amax(dim=(2, 3), keepdim=True)
        e = torch.exp(v[..., s] - m)
        rec[:, c, :, 0] = m[:, :, 0, 0]
        rec[:, c, :, 1] = (e.sum(2) * fw[s]).sum(-1)
        rec[:, c, :, 2] = (e.sum(2) * fh[s]).sum(-1)
        rec[:, c, :, 3:] = e.sum(3)
    return rec.float().contiguous(), n


@gpu
@pytest.mark.parametrize('offset', [0.0, -60.0])
@pytest.mark.parametrize('name', ['d24', 'e68'])
def test_finalize_alone_over_host_records(name, offset):
    """xas_head_softargmax_from_partials over records it did not produce: 9 chunks at D = 24 (K = 18), 73 at D = 68 (K = 3;
    the last one holds 16 pixels) - neither is the family's own count.  offset = -60: the logits of image 1 are lowered by 60
    on every other chunk, so those chunks' weight exp(max - M) is 9e-27 and their terms vanish in the float32 sums; the outputs
    must still be those of float64 on the same logits.  Bars: 4 x `dev_kps` / `dev_dmap` of the case; the log-sum-exp in
    stats[0] within 8 float32 spacings at its magnitude (M is exact, log S carries S's relative error of a few 1e-7, the
    fast logarithm's few units in the last place and the final rounding)."""
    from xas_amd import ops_head
    from xas_amd._lib import call, ptr
    D, K, B, hy, nb, seed = hs.spec(name)
    c = case(name)
    lg = c['lg'].contiguous()                                             # NCHW here: the records are built from the logical tensor
    if offset:
        lg = lg.clone().reshape(B, K * D, D * D)
        for ch in range(0, -(-D * D // 64), 2):
            lg[1, :, 64 * ch:64 * ch + 64] += offset
        lg = lg.reshape(B, K * D, D, D)
    ref = restated(lg, c['gw'], K, hy, nb) if offset else c
    lse64 = torch.logsumexp(lg.double().reshape(B, K, -1), dim=2)
    rec, n = host_records(lg)
    assert n == {24: 9, 68: 73}[D]
    kps = torch.zeros(B, hy, K, 3, device='cuda')
    idx = torch.zeros(B, K, hy, device='cuda', dtype=torch.int64)
    dmap = torch.zeros(1, K, D, device='cuda')
    stats = torch.zeros(B, K, ops_head.HEAD_STATS, device='cuda')
    call('xas_head_softargmax_from_partials', ptr(rec), B, K, D, n, hy, nb, ptr(kps), ptr(idx), ptr(dmap), 1, ptr(stats))
    g = golden('head_sizes') if name in hs.CASES else G()
    dk, dd = float(g[name + '_dev_kps']), float(g[name + '_dev_dmap'])
    ek, ed, el = err(kps, ref['kps']), err(dmap[0], ref['pz'][0]), err(stats[:, :, 0], lse64)
    bar_l = 8 * float(np.spacing(np.float32(lse64.abs().max().item())))
    print('%s offset %g: kps %.3e (bar %.3e)  dmap %.3e (bar %.3e)  lse %.3e (bar %.3e)' % (name, offset, ek, 4 * dk, ed, 4 * dd, el, bar_l))
    assert torch.equal(idx, ref['idx'])
    assert ek <= 4 * dk and ed <= 4 * dd and el <= bar_l


# ------------------------------------------------------------------ logit magnitude
MAGNITUDE = ['+40', '-40', 'x4']


@gpu
@pytest.mark.parametrize('how', MAGNITUDE)
def test_logit_magnitude_vs_float64(how):
    """The d24 cube with every logit moved by a constant (+40 / -40: a bias; the softmax does not see it) or scaled by 4 (a
    confident layer), forward and backward against float64.  Yardstick: restate() in float32 on the same input on the device,
    with torch's own softmax backward; bar 4 x its deviation from float64, measured here.  Peak indices bit for bit.
    Maximum deviation from float64 as measured on an MI355X (kps and depth map absolute, gradient relative to the float64
    gradient's maximum):

        transform   float32 restate: kps / dmap / grad      HIP head: kps / dmap / grad
        +40         3.65e-07 / 8.37e-08 / 3.99e-07          3.32e-07 / 9.24e-08 / 9.67e-07
        -40         2.96e-07 / 9.28e-08 / 4.00e-07          3.32e-07 / 8.74e-08 / 8.41e-07
        x4          3.09e-07 / 2.42e-07 / 9.80e-06          3.70e-07 / 1.16e-07 / 6.65e-06

    The backward's exp(v - lse) with lse rounded to float32 shows at +-40 (2.4 x / 2.1 x the yardstick) and stays inside the
    bar of 4 x; the kernel is unchanged.  (A build that carries exp(lse - M) / S beside lse measured 4.63e-07 / 5.35e-07 /
    8.07e-06: the remedy if a larger offset ever matters.)
    """
    D, K, B, hy, nb, seed = hs.CASES['d24']
    c = case('d24')
    lg = (c['lg'] * 4.0 if how == 'x4' else c['lg'] + float(how)).contiguous(memory_format=torch.channels_last)
    f64 = restated(lg, c['gw'], K, hy, nb)
    f32 = restated(lg, c['gw'], K, hy, nb, torch.float32)
    lgr = lg.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    kps, dmap, idx = forward('d24', lg=lgr)
    (kps * c['gw']).sum().backward()
    dev = {'kps': err(f32['kps'], f64['kps']), 'dmap': err(f32['pz'], f64['pz']), 'grad': err(f32['grad'], f64['grad']) / f64['gmax']}
    hip = {'kps': err(kps, f64['kps']), 'dmap': err(dmap, f64['pz'][0]), 'grad': err(lgr.grad, f64['grad']) / f64['gmax']}
    for k in dev:
        print('magnitude %s %s: float32 restate %.3e  hip %.3e  (bar %.3e)' % (how, k, dev[k], hip[k], 4 * dev[k]))
    assert torch.equal(f32['idx'], f64['idx']) and torch.equal(idx, f64['idx'])
    for k in dev:
        assert hip[k] <= 4 * dev[k], 'magnitude %s %s: %.3e from float64, bar %.3e' % (how, k, hip[k], 4 * dev[k])
