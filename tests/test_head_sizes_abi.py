"""Soft-argmax head at cube sides other than 16/32/64, without a GPU: the workspace query answers for every multiple of 4 up
to 128, refuses everything else with a message that names the range, keeps the power-of-two family's values, and the stored
golden cases still regenerate from their seeds."""
import os

import numpy as np
import pytest

import head_sizes_inputs as hs
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'x-as-supervision_amd', 'csrc')


def _ws(B, K, D):
    from xas_amd import _lib
    lib = _lib.load()
    return int(_lib.fn('xas_head_workspace_floats')(B, K, D)), lib.xas_last_error().decode()


def test_workspace_query_takes_the_new_sizes():
    for B, K, D in ((2, 18, 96), (1, 2, 128), (2, 3, 12), (2, 18, 24), (2, 2, 40)):
        n, _ = _ws(B, K, D)
        assert n > 0 and n % (B * K * (3 + D)) == 0, (B, K, D, n)        # B * nchunk * K * (3 + D)


@pytest.mark.parametrize('D', [10, 132, 0, 2, -4, 130])
def test_refused_sizes_name_the_accepted_range(D):
    n, err = _ws(2, 3, D)
    assert n == 0
    assert 'multiple of 4' in err and '[4,128]' in err and 'D == H == W' in err, err
    assert 'D=%d' % D in err, err


def test_power_of_two_sizes_keep_the_parent_values():
    """Values of the parent commit's build (B * nchunk * K * (3 + D) with that family's geometry)."""
    assert _ws(32, 18, 64)[0] == 32 * 32 * 18 * 67
    assert _ws(2, 2, 16)[0] == 2 * 2 * 2 * 19 == 152                      # P = 128 of HW = 256


def test_header_and_sources_state_the_range():
    hdr = open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()
    block = hdr[hdr.index('Soft-argmax ("integral") head.'):hdr.index('#define XAS_HEAD_STATS')]
    assert 'D % 4 == 0' in block and '4 <= D <= 128' in block
    for name in ('head.hip',):
        src = open(os.path.join(CSRC, name)).read()
        assert 'depth_dim must be a multiple of 4 in [4,128] (heat-map cube D == H == W)' in src, name


def test_conv_epilogue_still_takes_d64_only():
    """xas_conv_fwd_head_chunks: 0 for every D != 64 - the new sizes use the two-pass form."""
    src = open(os.path.join(ROOT, 'x-as-supervision_amd', 'modules', 'keypoint_detector_integral_multi.py')).read()
    assert 'depth_dim == 64' in src


@pytest.mark.parametrize('name', list(hs.CASES))
def test_golden_cases_regenerate_from_their_seeds(name):
    g = golden('head_sizes')
    D, K, B, hy, nb, seed = hs.CASES[name]
    lg = hs.logits(name)
    assert lg.shape == (B, K * D, D, D) and lg.dtype == np.float32
    assert hs.checksum(lg) == int(g[name + '_crc'])
    assert g[name + '_kps'].shape == (B, hy, K, 3) and g[name + '_depth_prob_map'].shape == (K, D)
    assert (name + '_z_peak_indices' in g.files) == (nb > 0)
    assert g[name + '_grad_logits_sub'].shape == (-(-lg.size // hs.GRAD_STRIDE),)
    for grp in ('kps', 'dmap', 'grad'):
        assert 0 < float(g['%s_dev_%s' % (name, grp)]) < 1e-3
    if nb and (0, 1) in hs.planted(name):                                 # the tie joint: lower bin first
        a, b = hs.tie_quads(D)
        assert g[name + '_z_peak_indices'][0, 1, :2].tolist() == [4 * a + 1, 4 * b + 1]
        q = lg.reshape(B, K, D, D, D)[0, 1]
        assert np.array_equal(q[4 * a:4 * a + 4], q[4 * b:4 * b + 4])


def test_synthetic_config_takes_a_patch_size():
    from xas_amd import synthetic
    c = synthetic.model_config()
    assert c['model_params']['detector_params']['depth_dim'] == 64 and c['train_params']['patch_width'] == 256
    c = synthetic.model_config(patch=384)
    assert c['model_params']['detector_params']['depth_dim'] == 96
    assert c['train_params']['patch_width'] == c['train_params']['patch_height'] == 384
    with pytest.raises(ValueError, match='multiple of 32'):
        synthetic.model_config(patch=100)
    with pytest.raises(ValueError, match='512'):
        synthetic.model_config(patch=1024)
