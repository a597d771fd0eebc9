"""xas_nchw_to_nhwc_mirror_pair: the batch a flip-test pass feeds the detector, bit-equal to torch.cat([x, x.flip(3)]) in
channels-last storage.  Sides that are a multiple of the wave (32 of 64 lanes, 256), one that is not (36), rows shorter than
the image is high, one image and three; nothing is written outside the result."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('H,W', [(20, 32), (36, 36), (256, 256)])
def test_mirror_pair_equals_flip_and_cat(B, H, W):
    from xas_amd import ops_nn
    from xas_amd._lib import call, ptr
    C = 3
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(B * 1000 + W)).cuda()
    want = torch.cat([x, x.flip(3)]).contiguous(memory_format=torch.channels_last)
    n, pad = 2 * B * C * H * W, 256
    buf = torch.full((n + 2 * pad,), 7.5, device='cuda')
    call('xas_nchw_to_nhwc_mirror_pair', ptr(x), B, C, H, W, ptr(buf[pad:]))
    got = buf[pad:pad + n].view(2 * B, H, W, C)
    assert torch.equal(got, want.permute(0, 2, 3, 1))
    assert bool((buf[:pad] == 7.5).all()) and bool((buf[pad + n:] == 7.5).all())
    y = ops_nn.mirror_pair_nchw(x)
    assert y.shape == (2 * B, C, H, W) and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, want)
    assert torch.equal(ops_nn.mirror_pair_nchw(x.contiguous(memory_format=torch.channels_last)), want)   # any input layout
