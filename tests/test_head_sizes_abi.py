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


# xas_head_workspace_floats(1, K, D) / (K * (3 + D)) = nchunk as the parent commit's library answered it for K = 1..69 (built from
# that commit, queried without a GPU): D -> (nchunk, the K it accepted); every other K was refused with 0.
_K8 = list(range(1, 17)) + list(range(18, 33, 2)) + list(range(36, 65, 4))
PARENT_POW2 = {4: (1, list(range(4, 65, 4))), 8: (1, _K8), 16: (2, _K8), 32: (8, _K8), 64: (32, _K8)}


def test_power_of_two_table_of_the_parent_and_no_refusal_left():
    """The dispatch rule is total: what the parent accepted keeps its workspace (and with it its policy's geometry), what it
    refused ("heat-map too small", "too wide for one workgroup") now runs on the general policy."""
    for D, (nchunk, accepted) in PARENT_POW2.items():
        for K in range(1, 70):
            n, err = _ws(1, K, D)
            assert n > 0 and n % (K * (3 + D)) == 0, (K, D, n, err)
            if K in accepted:
                assert n == nchunk * K * (3 + D), (K, D, n)


def test_workspace_query_takes_the_shapes_of_the_edge_table():
    for B, K, D in ((1, 3, 4), (1, 1, 4), (1, 257, 16), (1, 343, 12)):
        assert _ws(B, K, D)[0] > 0, (B, K, D)
    assert _ws(1, 343, 12)[0] == 2 * 343 * 15 and _ws(1, 61, 68)[0] == 37 * 61 * 71       # 128 pixels per block
    for name, (D, K, B, hy, nb, seed) in hs.EDGES.items():
        n, _ = _ws(B, K, D)
        assert n > 0 and n % (B * K * (3 + D)) == 0, name


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


@pytest.mark.parametrize('name', list(hs.EDGES))
def test_edge_cases_regenerate_from_their_seeds(name):
    g = golden('head_edges')
    D, K, B, hy, nb, seed = hs.EDGES[name]
    lg = hs.edge_logits(name)
    assert lg.shape == (B, K * D, D, D) and lg.dtype == np.float32
    assert hs.checksum(lg) == int(g[name + '_crc'])
    assert g[name + '_kps'].shape == (B, hy, K, 3) and g[name + '_depth_prob_map'].shape == (K, D)
    assert (name + '_z_peak_indices' in g.files) == (nb > 0)
    assert g[name + '_grad_logits_sub'].shape == (-(-lg.size // hs.GRAD_STRIDE),)
    for grp in ('kps', 'dmap', 'grad'):
        assert 0 < float(g['%s_dev_%s' % (name, grp)]) < 1e-3
    q = lg.reshape(B, K, D, D, D)
    for (b, k), (cz, amp, tie, noise) in hs.edge_planted(name).items():
        assert b < B and k < K and all(0 <= c <= D - 1 for c in cz), (name, b, k)
        if tie:                                                           # bit-equal quads: the marginals tie in any arithmetic
            assert np.array_equal(q[b, k, 4 * tie[0]:4 * tie[0] + 4], q[b, k, 4 * tie[1]:4 * tie[1] + 4])
    if nb:                                                                # the golden holds the rule wherever the reference defines the order
        unordered = hs.edge_unordered(name)
        for bk, want in hs.edge_expected(name).items():
            if bk not in unordered:
                assert g[name + '_z_peak_indices'][bk].tolist() == want, (name, bk)


def test_edge_table_is_the_issue_list():
    E = hs.EDGES
    assert [E[n][:5] for n in ('t12a', 't12b', 't12c')] == [(12, K, 2, 3, 5) for K in (341, 342, 343)]
    assert E['t68'][:5] == (68, 61, 1, 3, 15) and E['e68'][:5] == (68, 3, 2, 3, 15) and E['w16'][:5] == (16, 257, 1, 3, 7)
    assert E['tie128'][:5] == (128, 2, 1, 3, 15) and E['h6'][:5] == (24, 3, 2, 6, 5)
    assert sorted(E[n][:5] for n in hs.E4) == sorted((4, K, 2) + m for K in (1, 2, 3, 4, 5) for m in ((1, 0), (2, 3)))
    assert hs.edge_expected('e68') == {(0, 0): [1, 64, 66], (0, 1): [63, 30, 2], (0, 2): [61, 65, 20], (1, 0): [66, 1, 64],
                                       (1, 1): [30, 10, 50], (1, 2): [20, 40, 60]}
    assert hs.edge_expected('tie128') == {(0, 0): [62, 66, 20], (0, 1): [61, 65, 20]}
    assert hs.edge_unordered('tie128') == [(0, 1)] and hs.edge_unordered('h6') == [(0, 1), (1, 1)]


def test_one_peak_joint_fills_up_with_the_lowest_inner_bins():
    """h6, joint 1 (noise-free, one peak): the peak, then bins 1, 2, 3, ... skipping it - in the float32 and in the float64
    restatement; the six-peak joints come out by amplitude."""
    import torch
    D, K, B, hy, nb, seed = hs.EDGES['h6']
    lg = torch.from_numpy(hs.edge_logits('h6'))
    want = hs.edge_expected('h6')
    assert want[(0, 1)] == [9, 1, 2, 3, 4, 5] and want[(1, 1)] == [14, 1, 2, 3, 4, 5]
    for dtype in (torch.float32, torch.float64):
        kps, pz, idx = hs.restate(lg.to(dtype), K, hy, nb)
        for (b, k), w in want.items():
            assert idx[b, k].tolist() == w, (dtype, b, k, idx[b, k].tolist())
        for b, c in ((0, 9), (1, 14)):                                    # strictly monotone on either side of the peak
            d = pz[b, 1, 1:] - pz[b, 1, :-1]
            assert bool((d[:c] > 0).all()) and bool((d[c:] < 0).all())


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
