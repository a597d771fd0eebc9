"""The flip test end to end: KPDetector3DMulti.forward_flip / KPDetector3D.forward_flip (mirror-pair stack, one pass over 2B
images, the flip-merging head) against the float64 restatement of tests/test_gpu_head_flip.py applied to the detector's own
logits of net(x) and net(x.flip(3)), and Eval(flip_test=True).

The detector is small (ResNet-18, depth_dim 16, 64^2 patches, B = 2, eval()).  Its final convolution's weights are scaled down
and its bias plants three depth spikes per joint, at different bins and heights for the two joints of a pair, so the averaged
depth marginal's peaks do not depend on summation order (asserted: float64 margins above 1e-3).  Bars: those of
tests/test_gpu_head_sizes.py for this cube side (see test_gpu_head_flip.bars); peak indices exact."""
import functools

import numpy as np
import pytest
import torch

import inputs as gi
from test_gpu_head_flip import HM36_PAIRS, MARGIN, bars, err, flip64, perm_of

pytestmark = pytest.mark.gpu
K, D, S, B = 18, 16, 64, 2


def planted_bias(seed):
    """[K*D]: spikes of 6, 5, 4 (order drawn per joint) at bins 3, 8, 12; for the second joint of a pair spikes of 5.5, 4.5, 3.5
    at bins 5, 10, 14.  The bias is the same for an image and its mirror, so a paired joint's averaged marginal carries all six
    spikes, half a unit of logit apart in height."""
    rng = np.random.Generator(np.random.PCG64(seed))
    perm = perm_of(HM36_PAIRS, K)
    out = np.zeros((K, D), np.float32)
    for k in range(K):
        second = perm[k] < k
        out[k, [5, 10, 14] if second else [3, 8, 12]] = (np.array([6.0, 5.0, 4.0]) - 0.5 * second)[rng.permutation(3)]
    return out.reshape(-1)


@functools.lru_cache(maxsize=None)
def detector(multi):
    from modules.keypoint_detector_integral import KPDetector3D
    from modules.keypoint_detector_integral_multi import KPDetector3DMulti
    det = KPDetector3DMulti('resnet_multi', K, D, 3, 15, num_layers=18) if multi else KPDetector3D('resnet', K, D, num_layers=18)
    gi.seeded_fill_(det, seed=71)
    det = det.cuda().eval()
    last = det.net.head.features[-1]
    with torch.no_grad():                                 # scaled down: the logits of a channel vary by 0.3 (rms) over a heat-map
        last.bias.zero_()
        last.weight.mul_(0.3 / float(det.net(images()).std(dim=(2, 3)).mean()))
        last.bias.copy_(torch.from_numpy(planted_bias(72)).cuda())
    return det


@functools.lru_cache(maxsize=None)
def images():
    return torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(73)).cuda()


@functools.lru_cache(maxsize=None)
def reference(multi):
    """float64 head of the averaged heat-maps, from the detector's own logits of the images and of their mirrors."""
    det, x = detector(multi), images()
    with torch.no_grad():
        l = torch.cat([det.net(x), det.net(x.flip(3))]).cpu().numpy().reshape(2 * B, K, D, D, D)
    return flip64(l, perm_of(HM36_PAIRS, K), 3 if multi else 1, 15 if multi else 0)


def test_forward_flip_vs_float64():
    det = detector(True)
    kps64, pz64, idx64, margin = reference(True)
    assert margin > MARGIN, 'float64 peak margin %.3e' % margin
    with torch.no_grad():
        kps, dmap = det.forward_flip(images(), HM36_PAIRS)
        idx = det.last_peak_indices                                       # (the plain forward below leaves its own)
        plain = det(images())[0]
    assert kps.shape == (B, 3, K, 3) and dmap.shape == (K, D)
    bk, bd = bars(D)
    ek, ed = err(kps, kps64), err(dmap, pz64[0])
    print('forward_flip: |kps - f64| %.3e (bar %.3e)  |dmap - f64| %.3e (bar %.3e)' % (ek, bk, ed, bd))
    assert idx.dtype == torch.int64 and not torch.equal(idx, det.last_peak_indices)
    assert np.array_equal(idx.cpu().numpy(), idx64)
    assert ek <= bk and ed <= bd
    assert err(kps[..., 0], plain[..., 0]) > 1e-3                       # the mirrored image does move the joints
    perm = det._flip_perm
    with torch.no_grad():
        det.forward_flip(images(), [list(p) for p in HM36_PAIRS])
    assert det._flip_perm is perm                                         # built once per (pairs, device)


def test_forward_flip_single_hypothesis_vs_float64():
    det = detector(False)
    kps64, pz64, _, _ = reference(False)
    with torch.no_grad():
        kps, dmap = det.forward_flip(images(), HM36_PAIRS)
    assert kps.shape == (B, 1, K, 3) and dmap.shape == (K, D)
    bk, bd = bars(D)
    ek, ed = err(kps, kps64), err(dmap, pz64[0])
    print('forward_flip, single: |kps - f64| %.3e (bar %.3e)  |dmap - f64| %.3e (bar %.3e)' % (ek, bk, ed, bd))
    assert ek <= bk and ed <= bd


def test_forward_flip_at_depth64_runs_from_the_conv_epilogue():
    """depth_dim = 64: the final convolution's epilogue emits the records of all 2B images, and the flip merge is the only
    head launch of the pass."""
    from modules.keypoint_detector_integral_multi import KPDetector3DMulti
    from xas_amd import ops_nn
    torch.manual_seed(74)
    det = KPDetector3DMulti('resnet_multi', K, 64, 3, 15, num_layers=18).cuda().eval()
    before = dict(ops_nn.head_stats)
    with torch.no_grad():
        kps, dmap = det.forward_flip(torch.rand(1, 3, 256, 256, device='cuda'), HM36_PAIRS)
    assert ops_nn.head_stats['fused'] == before['fused'] + 1 and ops_nn.head_stats['separate'] == before['separate']
    assert kps.shape == (1, 3, K, 3) and dmap.shape == (K, 64) and det.last_peak_indices.shape == (1, K, 3)
    assert bool(torch.isfinite(kps).all()) and float(kps.abs().max()) <= 1.0
    assert abs(float(dmap.sum()) - K) < 1e-3


def test_forward_flip_is_an_inference_path():
    det, x = detector(True), images()
    with pytest.raises(RuntimeError, match='without a backward'):
        det.forward_flip(x, HM36_PAIRS)                                   # autograd would record the pass
    det.train()
    try:
        with torch.no_grad(), pytest.raises(RuntimeError, match=r'eval\(\)'):
            det.forward_flip(x, HM36_PAIRS)
    finally:
        det.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match='exceed the 384 images'):
        det.forward_flip(x[:1].expand(193, 3, S, S), HM36_PAIRS)
    with torch.no_grad(), pytest.raises(RuntimeError, match='flip pair'):
        det.forward_flip(x, [[1, 18]])


def test_eval_batch_with_and_without_the_flip_test():
    import eval as xeval
    from xas_amd.synthetic import synthetic_eval_batch
    cams = [0, 1]
    cfg = {'model_params': {'cam_id_list': cams, 'flip_pairs': HM36_PAIRS}, 'dataset_params': {'dataset': {'name': 'h36m'}}}
    x = synthetic_eval_batch(B, cams, torch.device('cuda'), seed=5, S=S)
    det = detector(True)
    flip = xeval.Eval(cfg, det, [], '/tmp', img_size=float(S), flip_test=True).eval_batch(x, 'best')
    off = xeval.Eval(cfg, det, [], '/tmp', img_size=float(S), flip_test=False).eval_batch(x, 'best')
    default = xeval.Eval(cfg, det, [], '/tmp', img_size=float(S)).eval_batch(x, 'best')
    assert set(flip) == set(off) == set(default)
    for k, v in flip.items():
        assert bool(torch.isfinite(v).all()), k
    for k in off:
        assert torch.equal(off[k], default[k]), k
    assert any(not torch.equal(flip[k], off[k]) for k in flip if k.startswith('err2d'))
