"""Soft-argmax head at cube sides other than 16/32/64 (the general policy of csrc/head.hip) on the GPU, against the
reference-generated golden `head_sizes.npz` (tests/golden/make_golden_head_sizes.py) and against float64 autograd through
the restatement of tests/golden/head_sizes_inputs.py (evaluated here, in float64 on the device).

Tolerances: the rule of tests/test_gpu_reproject.py.  The generator stores, per case and output group, the reference's own
float32 deviation from float64 (`dev_*`); the HIP result must be within 4 x that of float64 and within 5 x of the float32
golden (that bar plus the golden's own deviation).  The gradient is measured relative to the float64 gradient's maximum.
Deviations of the reference as generated:

    case   D    K   B   dev kps     dev dmap    dev grad (rel)
    d12    12   3   2   1.76e-07    6.25e-08    3.60e-07
    d24    24  18   2   4.41e-07    2.09e-07    7.40e-07
    d40    40   2   2   4.86e-07    1.23e-07    7.59e-07
    d96    96  18   2   2.34e-06    1.23e-06    2.09e-05
    d128  128   2   1   3.42e-05    1.69e-05    1.23e-04

Peak indices are compared bit for bit, the planted tie included (head_sizes_inputs.py says how the tie is made exact)."""
import functools

import numpy as np
import pytest
import torch

import head_sizes_inputs as hs
import inputs as gi
from conftest import golden

gpu = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
ALL = list(hs.CASES)
MULTI = [n for n in ALL if hs.CASES[n][4] > 0]
PAIRS = [n for n in ALL if hs.CASES[n][2] == 2]


@functools.lru_cache(maxsize=None)
def G():
    return golden('head_sizes')


@functools.lru_cache(maxsize=None)
def case(name):
    """Logits on the device (NHWC storage) and the float64 restatement with its autograd gradient: computed once per case,
    never modified."""
    D, K, B, hy, nb, seed = hs.CASES[name]
    lg = T(hs.logits(name)).cuda().contiguous(memory_format=torch.channels_last)
    gw = T(hs.grad_kps(name)).cuda()
    l64 = lg.double().contiguous().requires_grad_(True)
    k64, pz64, i64 = hs.restate(l64, K, hy, nb)
    (k64 * gw.double()).sum().backward()
    return {'lg': lg, 'gw': gw, 'kps64': k64.detach(), 'pz64': pz64.detach(), 'idx64': i64, 'grad64': l64.grad,
            'gmax64': float(l64.grad.abs().max())}


def err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def check(name, group, e64, eg, what):
    d = float(G()['%s_dev_%s' % (name, group)])
    print('%s %s %s: |hip - f64| %.3e (bar %.3e)  |hip - golden| %.3e (bar %.3e)' % (name, what, group, e64, 4 * d, eg, 5 * d))
    assert e64 <= 4 * d, '%s %s %s: %.3e from float64, bar %.3e' % (name, what, group, e64, 4 * d)
    assert eg <= 5 * d, '%s %s %s: %.3e from the golden, bar %.3e' % (name, what, group, eg, 5 * d)


def forward(name, groups=1, lg=None):
    from xas_amd import ops_head
    D, K, B, hy, nb, seed = hs.CASES[name]
    lg = case(name)['lg'] if lg is None else lg
    if nb:
        return ops_head.softargmax_multi(lg, K, hy, nb, groups=groups)
    kps, dmap = ops_head.softargmax_single(lg, K, groups=groups)
    return kps, dmap, None


def backward(name):
    """-> (kps, grad_logits through autograd)."""
    c = case(name)
    lg = c['lg'].detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    kps, _, _ = forward(name, lg=lg)
    (kps * c['gw']).sum().backward()
    return kps.detach(), lg.grad


# ------------------------------------------------------------------ forward
@gpu
@pytest.mark.parametrize('name', ALL)
def test_forward_vs_golden_and_float64(name):
    D, K, B, hy, nb, seed = hs.CASES[name]
    c, g = case(name), G()
    kps, dmap, idx = forward(name)
    assert kps.shape == (B, hy, K, 3) and dmap.shape == (K, D)
    if nb:
        assert idx.dtype == torch.int64 and idx.shape == (B, K, hy)
        assert np.array_equal(idx.cpu().numpy(), g[name + '_z_peak_indices'])                 # bit exact, tie included
        assert torch.equal(idx, c['idx64'])
    check(name, 'kps', err(kps, c['kps64']), err(kps, T(g[name + '_kps'])), 'forward')
    check(name, 'dmap', err(dmap, c['pz64'][0]), err(dmap, T(g[name + '_depth_prob_map'])), 'forward')


@gpu
def test_planted_peaks_are_found_where_they_were_put():
    """Bins 1 and D-2, the tie pair in the order of the rule, and at D = 128 the peaks at 62 / 66 whose windows straddle
    bins 63/64 (their depth coordinate is covered by test_forward_vs_golden_and_float64)."""
    for name in MULTI:
        D = hs.CASES[name][0]
        idx = forward(name)[2].cpu()
        for (b, k), (cz, amp) in hs.planted(name).items():
            if len(cz) == 3:
                assert idx[b, k].tolist() == [c for _, c in sorted(zip(amp, cz), reverse=True)], (name, b, k)
            else:
                qa, qb = hs.tie_quads(D)
                assert idx[b, k].tolist() == [4 * qa + 1, 4 * qb + 1, cz[1]], (name, idx[b, k].tolist())
    assert forward('d128')[2][0, 0].tolist() == [62, 66, 20]
    assert forward('d96')[2][0, 1].tolist() == [61, 65, 20]                      # equal values on either side of bin 63/64


# ------------------------------------------------------------------ backward
@gpu
@pytest.mark.parametrize('name', ALL)
def test_backward_vs_golden_and_float64(name):
    c, g = case(name), G()
    _, grad = backward(name)
    assert grad.shape == c['lg'].shape
    e64 = err(grad, c['grad64']) / c['gmax64']
    sub = grad.contiguous().reshape(-1)[::hs.GRAD_STRIDE]
    eg = err(sub, T(g[name + '_grad_logits_sub'])) / c['gmax64']
    check(name, 'grad', e64, eg, 'backward')
    d = float(g[name + '_dev_grad'])
    ea = abs(float(grad.abs().max()) - float(g[name + '_grad_amax'])) / c['gmax64']
    assert ea <= 5 * d, '%s: max |grad| %.3e from the golden (relative), bar %.3e' % (name, ea, 5 * d)


@gpu
@pytest.mark.parametrize('name', ALL)
def test_recorded_maximum_equals_the_gradient_maximum(name):
    """xas_head_softargmax_bwd_amax: the slot's maximum over its sub-maxima is max |grad_logits|, exactly."""
    from xas_amd import ops_head, ops_nn
    from xas_amd._lib import call, ptr
    D, K, B, hy, nb, seed = hs.CASES[name]
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


# ------------------------------------------------------------------ the family against itself
@gpu
@pytest.mark.selfcheck
@pytest.mark.parametrize('name', PAIRS)
def test_groups_give_one_depth_map_per_sub_batch(name):
    D, K, B, hy, nb, seed = hs.CASES[name]
    c = case(name)
    kps, dmap, idx = forward(name)
    kps2, dmap2, idx2 = forward(name, groups=2)
    assert dmap2.shape == (2, K, D)
    assert torch.equal(dmap2[0], dmap)
    d = float(G()[name + '_dev_dmap'])
    for i in range(2):
        assert err(dmap2[i], c['pz64'][i]) <= 4 * d
    assert torch.equal(kps, kps2)
    if nb:
        assert torch.equal(idx, idx2)


@gpu
@pytest.mark.selfcheck
@pytest.mark.parametrize('name', ALL)
def test_forward_and_backward_are_bit_reproducible(name):
    a, b = (forward(name) + backward(name) for _ in range(2))
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v)


@gpu
@pytest.mark.selfcheck
@pytest.mark.parametrize('name', ['d24', 'd96'])
def test_from_partials_reproduces_the_one_call_forward(name):
    """xas_head_softargmax_from_partials over the records that the general policy's own first pass left in the workspace."""
    from xas_amd import ops_head
    from xas_amd._lib import call, ptr
    D, K, B, hy, nb, seed = hs.CASES[name]
    lg = case(name)['lg']

    def outputs():
        return (torch.zeros(B, hy, K, 3, device='cuda'), torch.zeros(B, K, hy, device='cuda', dtype=torch.int64),
                torch.zeros(1, K, D, device='cuda'), torch.zeros(B, K, ops_head.HEAD_STATS, device='cuda'))
    n = ops_head.query('xas_head_workspace_floats', B, K, D)
    nchunk = n // (B * K * (3 + D))
    assert n == B * nchunk * K * (3 + D) and nchunk > 1
    ws = torch.empty(n, device='cuda')
    kps, idx, dmap, stats = outputs()
    call('xas_head_softargmax_fwd', ptr(lg), B, K, D, hy, nb, ptr(kps), ptr(idx), ptr(dmap), 1, ptr(stats), ptr(ws))
    kps2, idx2, dmap2, stats2 = outputs()
    call('xas_head_softargmax_from_partials', ptr(ws), B, K, D, nchunk, hy, nb, ptr(kps2), ptr(idx2), ptr(dmap2), 1, ptr(stats2))
    assert torch.equal(kps, kps2) and torch.equal(idx, idx2) and torch.equal(dmap, dmap2)
    assert torch.equal(stats, stats2)                                     # (zero-filled: the unused entries are equal too)
    k0, d0, i0 = forward(name)
    assert torch.equal(kps, k0) and torch.equal(idx, i0) and torch.equal(dmap[0], d0)


@gpu
def test_refused_sizes_fail_with_the_accepted_range():
    from xas_amd import ops_head
    for D in (10, 132):
        with pytest.raises(RuntimeError, match=r'multiple of 4 in \[4,128\]'):
            ops_head.softargmax_multi(torch.zeros(1, 2 * D, D, D, device='cuda'), 2, 3, 5)
    with pytest.raises(RuntimeError, match=r'D == H == W with D a multiple of 4 in \[4,128\]'):
        ops_head.softargmax_multi(torch.zeros(1, 2 * 24, 24, 20, device='cuda'), 2, 3, 5)


# ------------------------------------------------------------------ end to end
def _detectors(D, multi=True):
    from modules.keypoint_detector_integral import KPDetector3D
    from modules.keypoint_detector_integral_multi import KPDetector3DMulti
    from oracle import step as ostep
    ora = ostep.Regressor('resnet_multi', 18, D, 3, 15) if multi else ostep.Regressor('resnet', 18, D)
    gi.seeded_fill_(ora, seed=61)
    with torch.no_grad():
        ora.net.head.features[9].bias.copy_(T(gi.planted_depth_bias(18, D, seed=62)))
    hip = KPDetector3DMulti('resnet_multi', 18, D, 3, 15) if multi else KPDetector3D('resnet', 18, D)
    hip.load_state_dict(ora.state_dict(), strict=True)
    return hip.cuda(), ora


@gpu
def test_detector_depth24_vs_oracle():
    """KPDetector3DMulti(depth_dim=24) on [2,3,96,96], forward and backward, against oracle/nets.py + oracle/head.py with
    the same seeded weights, at the bars of test_gpu_nn.test_detector_vs_golden_and_oracle: joints 1e-4, depth map 1e-5, peak
    indices bit exact, parameter gradients max(3e-3, 4 x DEV) with that test's DEV per tensor."""
    from xas_amd import ops_nn
    hip, ora = _detectors(24)
    hip.train()
    ora.train()
    x = T(gi.synthetic_batch(2, [0], seed=63, S=96)['cam_0_img'])
    gw = T(np.random.Generator(np.random.PCG64(64)).standard_normal((2, 3, 18, 3)).astype(np.float32))
    before = dict(ops_nn.head_stats)
    kps, dmap = hip(x.cuda())
    assert ops_nn.head_stats['separate'] == before['separate'] + 1 and ops_nn.head_stats['fused'] == before['fused']
    assert kps.shape == (2, 3, 18, 3) and dmap.shape == (18, 24)
    from oracle import head as ohead
    logits = ora.net(x)
    ko, do, io = ohead.softargmax_multi(logits, 18, 3, 15)
    print('detector D=24: |kps - oracle| %.3e (bar 1e-4)  |dmap - oracle| %.3e (bar 1e-5)' % (err(kps, ko), err(dmap, do)))
    assert err(kps, ko) < 1e-4
    assert err(dmap, do) < 1e-5
    assert np.array_equal(io.numpy(), hip.last_peak_indices.cpu().numpy())
    (kps * gw.cuda()).sum().backward()
    (ko * gw).sum().backward()
    rel = lambda a, b: float((a.detach().cpu().double() - b.detach().double()).norm() / (b.detach().double().norm() + 1e-30))
    DEV = {'g_conv1': 1.07e-2, 'g_l1c2': 9.0e-3, 'g_l2ds': 1.04e-2, 'g_dc0': 4.4e-3, 'g_fin_b': 3.5e-5, 'g_bn1_w': 8.5e-3,
           'norms': 1.0e-2}
    GT = lambda k: max(3e-3, 4.0 * DEV[k])                       # noqa: E731
    p, q = dict(hip.named_parameters()), dict(ora.named_parameters())
    picks = [('g_conv1', 'net.backbone.conv1.weight', slice(None), slice(None)),
             ('g_l1c2', 'net.backbone.layer1.0.conv2.weight', slice(0, 8), slice(None)),
             ('g_l2ds', 'net.backbone.layer2.0.downsample.0.weight', slice(0, 4), slice(0, 16)),
             ('g_dc0', 'net.head.features.0.weight', slice(0, 4), slice(0, 4)),
             ('g_fin_b', 'net.head.features.9.bias', slice(None), None),
             ('g_bn1_w', 'net.backbone.bn1.weight', slice(None), None)]
    for key, pname, s0, s1 in picks:
        a, b = (p[pname].grad[s0], q[pname].grad[s0]) if s1 is None else (p[pname].grad[s0, s1], q[pname].grad[s0, s1])
        print('detector D=24: %s %.3e (bar %.3e)' % (key, rel(a, b), GT(key)))
        assert rel(a, b) < GT(key), key
    for pname in ('net.backbone.layer4.2.conv3.weight', 'net.head.features.6.weight'):
        r = abs(float(p[pname].grad.norm()) / float(q[pname].grad.norm()) - 1)
        print('detector D=24: norm %s %.3e (bar %.3e)' % (pname, r, GT('norms')))
        assert r < GT('norms'), pname


@gpu
@pytest.mark.parametrize('S,multi', [(96, False), (160, True), (384, True)])
def test_detectors_run_at_other_input_sizes(S, multi):
    """depth_dim = S / 4: forward and backward run, the outputs are finite and the softmax gradient reaches the stem."""
    from modules.keypoint_detector_integral import KPDetector3D
    from modules.keypoint_detector_integral_multi import KPDetector3DMulti
    torch.manual_seed(S)
    det = (KPDetector3DMulti('resnet_multi', 18, S // 4, 3, 15) if multi else KPDetector3D('resnet', 18, S // 4)).cuda().train()
    x = torch.rand(1 if S > 256 else 2, 3, S, S, device='cuda')
    kps, dmap = det(x)
    assert kps.shape == (x.shape[0], 3 if multi else 1, 18, 3) and dmap.shape == (18, S // 4)
    assert bool(torch.isfinite(kps).all()) and float(kps.abs().max()) <= 1.0
    assert abs(float(dmap.sum()) - 18.0) < 1e-3
    kps.square().sum().backward()
    g = det.net.backbone.conv1.weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    with pytest.raises(RuntimeError, match=r'depth_dim=%d\) takes square input patches of side 4 \* depth_dim = %d, got input' % (S // 4, S)):
        det(torch.rand(1, 3, S + 32, S + 32, device='cuda'))
