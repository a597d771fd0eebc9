"""The flip-merging second pass of the soft-argmax head (head_finalize_flip_kernel of csrc/head.hip) alone, through both C
entry points (xas_head_softargmax_fwd_flip from the logits, xas_head_softargmax_flip_from_partials from first-pass records),
against a float64 restatement written here in numpy: softmax each logit cube, mirror the second image's along W, gather joint
perm[k], average, take the three marginals and the expectation, then find_peak, top-k with the lowest index on ties and the
zero-padded windows - the arithmetic of keypoint_detector_integral_multi.py:24-64 applied to the averaged heat-map.

Inputs: every (image, joint) gets `num_hypo` spikes along depth on a noisy floor and an off-centre bump in (h, w).  Joint k of
image b and joint perm[k] of image B + b (the same limb, seen mirrored) carry their spikes at the same bins with different
amplitude orders, so that the average ranks them in an order neither image has on its own; the two joints of a pair carry them
at different bins, so a wrong table changes the indices, and the bump is off-centre, so a missing mirror changes x.

Tolerances are those of tests/test_gpu_head_sizes.py: the HIP result is within 4 x the reference's own float32 deviation from
float64, which that file lists per cube side (d12 1.76e-07 / 6.25e-08 for joints / depth map, d24 4.41e-07 / 2.09e-07, d40
4.86e-07 / 1.23e-07, d96 2.34e-06 / 1.23e-06, d128 3.42e-05 / 1.69e-05).  A case here takes the row of the largest listed side
that is not larger than its own (sides below 12: the row of 12), which is never the looser choice.  Peak indices are compared
exactly; every case asserts first that its float64 peak margins exceed 1e-3 relative, so no case depends on rounding."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = {12: (1.76e-07, 6.25e-08), 24: (4.41e-07, 2.09e-07), 40: (4.86e-07, 1.23e-07), 96: (2.34e-06, 1.23e-06),
       128: (3.42e-05, 1.69e-05)}
MARGIN = 1e-3
HM36_PAIRS = [[1, 4], [2, 5], [3, 6], [14, 11], [15, 12], [16, 13]]

# name: D, K, B, pairs, num_hypo, neighbor, groups, logit offset of the two halves, planted bins of joint 0 (None: drawn)
CASES = {
    'd4_single': (4, 4, 1, [[0, 1], [2, 3]], 1, 0, 1, 0.0, None),         # power-of-two policy needs K % 4 == 0 at D = 4
    'd8': (8, 2, 1, [[0, 1]], 3, 3, 1, 0.0, None),                        # power-of-two policy
    'd8_offset80': (8, 2, 1, [[0, 1]], 3, 3, 1, 80.0, None),              # maxima 160 apart: each image keeps its own normaliser
    'd12_k5_groups3': (12, 5, 3, [[0, 3], [1, 4]], 3, 15, 3, 0.0, None),  # general policy, two pairs + one unpaired joint
    'd12_single': (12, 5, 1, [[0, 3], [1, 4]], 1, 0, 1, 0.0, None),
    'd64': (64, 2, 1, [[0, 1]], 3, 15, 1, 0.0, None),
    'd68_k1': (68, 1, 1, [], 3, 15, 1, 0.0, (63, 30, 50)),                # second-bin lanes: a peak at bin 63, window 56..67
    'd128_k1': (128, 1, 1, [], 3, 15, 1, 0.0, (64, 100, 58)),             # a peak at bin 64 (window 57..71) and one at 58 (51..65)
}
SOURCES = ('logits', 'partials')


def bars(D):
    d = DEV[max([s for s in DEV if s <= D] or [12])]
    return 4 * d[0], 4 * d[1]


def perm_of(pairs, K):
    perm = list(range(K))
    for a, b in pairs:
        perm[a], perm[b] = b, a
    return perm


def planted(D, K, B, perm, hy, seed, offset=0.0, bins0=None):
    """-> float32 logits [2B, K, D, H, W] (images 0..B-1, then the images that stand for their mirrors)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    step = max(2, D // 6)
    amp1, amp2 = np.array([6.0, 5.0, 4.0]), np.array([4.5, 6.0, 5.0])
    g = np.arange(D, dtype=np.float64)
    out = np.empty((2 * B, K, D, D, D), np.float32)
    for b in range(B):
        bins = {}
        for k in range(K):                                # inner bins `step` apart; the second joint of a pair one bin further
            slots = list(range(1 + (perm[k] < k), D - 1, step))
            bins[k] = bins0 if (bins0 is not None and k == 0) else tuple(int(v) for v in rng.permutation(slots)[:hy])
        for k in range(K):
            cx, cy = rng.uniform(D * 0.15, D * 0.4), rng.uniform(D * 0.3, D * 0.7)
            for img, kk, amp, centre in ((b, k, amp1, cx), (B + b, perm[k], amp2, D - 1 - cx + rng.uniform(-1.0, 1.0))):
                fz = np.zeros(D)
                for a, c in zip(amp, bins[k]):
                    fz[c] = a
                sxy = D / 10.0 + 0.5
                fxy = np.exp(-0.5 * (((g[None, :] - centre) / sxy) ** 2 + ((g[:, None] - cy) / sxy) ** 2))
                vol = fz[:, None, None] + 3.0 * fxy[None] + 0.05 * rng.standard_normal((D, D, D), dtype=np.float32)
                out[img, kk] = (vol + (offset if img < B else -offset)).astype(np.float32)
    return out


def softmax64(l):
    """[n, K, D, H, W] float32 -> float64 softmax over (D, H, W)."""
    l = l.astype(np.float64)
    e = np.exp(l - l.max(axis=(2, 3, 4), keepdims=True))
    return e / e.sum(axis=(2, 3, 4), keepdims=True)


def head64(p, hy, nb):
    """Heat-maps p [B, K, D, H, W] float64 -> kps [B, hy, K, 3], pz [B, K, D], idx [B, K, hy], smallest relative peak margin."""
    B, K, D = p.shape[:3]
    ar = np.arange(D, dtype=np.float64)
    px, py, pz = p.sum(axis=(2, 3)), p.sum(axis=(2, 4)), p.sum(axis=(3, 4))
    x, y = (px * ar).sum(-1) / D * 2 - 1, (py * ar).sum(-1) / D * 2 - 1
    kps = np.empty((B, hy, K, 3))
    kps[..., 0], kps[..., 1] = x[:, None], y[:, None]
    idx = np.zeros((B, K, hy), np.int64)
    if nb == 0:
        kps[:, 0, :, 2] = (pz * ar).sum(-1) / D * 2 - 1
        return kps, pz, idx, np.inf
    mid = pz[..., 1:-1]
    score = np.where((mid >= pz[..., :-2]) & (mid >= pz[..., 2:]), mid, 0.0)
    order = np.argsort(-score, axis=-1, kind='stable')                   # value descending, lower index first
    idx = order[..., :hy] + 1
    ranked = np.take_along_axis(score, order, -1)
    with np.errstate(invalid='ignore'):              # fewer than hy peaks: 0 / 0, a margin of nan, which no case passes with
        margin = float(((ranked[..., :hy] - ranked[..., 1:hy + 1]) / ranked[..., :hy]).min())
    top = np.take_along_axis(pz, idx, -1)
    for side in (-1, 1):
        margin = min(margin, float(((top - np.take_along_axis(pz, idx + side, -1)) / top).min()))
    r = nb // 2
    win = np.abs(ar[None, None, None, :] - idx[..., None]) <= r           # zero padded window
    pzw = pz[:, :, None, :] * win
    kps[..., 2] = ((pzw * ar).sum(-1) / pzw.sum(-1)).transpose(0, 2, 1) / D * 2 - 1
    return kps, pz, idx, margin


def flip64(l, perm, hy, nb):
    """The reference: float32 logits [2B, K, D, H, W] -> head64 of the averaged heat-maps."""
    B = l.shape[0] // 2
    p = softmax64(l)
    return head64(0.5 * (p[:B] + p[B:, :, :, :, ::-1][:, perm]), hy, nb)


def device_logits(l):
    """[n, K, D, H, W] numpy -> [n, K*D, H, W] on the device with NHWC storage."""
    n, K, D = l.shape[:3]
    return torch.from_numpy(np.ascontiguousarray(l.reshape(n, K * D, D, D))).cuda().contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and the float64 reference: computed once per case, never modified."""
    D, K, B, pairs, hy, nb, groups, offset, bins0 = CASES[name]
    perm = perm_of(pairs, K)
    l = planted(D, K, B, perm, hy, seed=700 + sum(map(ord, name.replace('_offset80', ''))), offset=offset, bins0=bins0)
    kps, pz, idx, margin = flip64(l, perm, hy, nb)
    own = min(head64(softmax64(l), hy, nb)[3], margin)                  # each image's own marginal has its peaks too
    return {'l': l, 'lg': device_logits(l), 'perm': perm, 'perm_dev': torch.tensor(perm, dtype=torch.int32, device='cuda'),
            'kps': kps, 'pz': pz, 'idx': idx, 'margin': own}


def run_flip(lg, perm_dev, K, D, hy, nb, groups, source):
    """One of the two entry points -> kps, z_idx, depth maps [groups, K, D]."""
    from xas_amd import ops_head
    from xas_amd._lib import call, ptr, query
    B = lg.shape[0] // 2
    kps = torch.full((B, hy, K, 3), float('nan'), device='cuda')
    idx = torch.full((B, K, hy), -7, device='cuda', dtype=torch.int64)
    dmap = torch.full((groups, K, D), float('nan'), device='cuda')
    n = query('xas_head_workspace_floats', 2 * B, K, D)
    nchunk = n // (2 * B * K * (3 + D))
    assert n == 2 * B * nchunk * K * (3 + D) and nchunk >= 1
    ws = torch.empty(n, device='cuda')
    if source == 'logits':
        call('xas_head_softargmax_fwd_flip', ptr(lg), B, K, D, hy, nb, ptr(perm_dev), ptr(kps), ptr(idx), ptr(dmap), groups, ptr(ws))
    else:                        # the records that the plain head's own first pass leaves in its workspace
        k2 = torch.empty(2 * B, hy, K, 3, device='cuda')
        i2 = torch.empty(2 * B, K, hy, device='cuda', dtype=torch.int64)
        d2 = torch.empty(1, K, D, device='cuda')
        st = torch.empty(2 * B, K, ops_head.HEAD_STATS, device='cuda')
        call('xas_head_softargmax_fwd', ptr(lg), 2 * B, K, D, hy, nb, ptr(k2), ptr(i2), ptr(d2), 1, ptr(st), ptr(ws))
        call('xas_head_softargmax_flip_from_partials', ptr(ws), B, K, D, nchunk, hy, nb, ptr(perm_dev), ptr(kps), ptr(idx), ptr(dmap),
             groups)
    return kps, idx, dmap


def err(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.abs(a - b).max())


def check(name, what, D, kps, idx, dmap, ref_kps, ref_idx, ref_pz, nb, groups=1):
    bk, bd = bars(D)
    B = ref_kps.shape[0]
    ek, ed = err(kps, ref_kps), err(dmap, ref_pz[::B // groups])
    print('%s %s: |kps - f64| %.3e (bar %.3e)  |dmap - f64| %.3e (bar %.3e)' % (name, what, ek, bk, ed, bd))
    if nb:
        assert np.array_equal(idx.cpu().numpy(), ref_idx), (name, what, idx.cpu().tolist(), ref_idx.tolist())
    else:
        assert not bool(idx.any())
    assert ek <= bk, '%s %s: joints %.3e from float64, bar %.3e' % (name, what, ek, bk)
    assert ed <= bd, '%s %s: depth map %.3e from float64, bar %.3e' % (name, what, ed, bd)


@pytest.mark.parametrize('source', SOURCES)
@pytest.mark.parametrize('name', list(CASES))
def test_flip_vs_float64(name, source):
    D, K, B, pairs, hy, nb, groups, offset, bins0 = CASES[name]
    c = case(name)
    assert c['margin'] > MARGIN, '%s: float64 peak margin %.3e' % (name, c['margin'])
    kps, idx, dmap = run_flip(c['lg'], c['perm_dev'], K, D, hy, nb, groups, source)
    check(name, source, D, kps, idx, dmap, c['kps'], c['idx'], c['pz'], nb, groups)


def test_the_inputs_tell_a_wrong_table_and_a_missing_mirror():
    """What the planted inputs are for, in float64: with the identity table instead of the pairs the indices change, and without
    the mirror x moves by far more than any bar; each image alone ranks its peaks differently from the average."""
    D, K, B, pairs, hy, nb, groups, offset, bins0 = CASES['d12_k5_groups3']
    c = case('d12_k5_groups3')
    assert not np.array_equal(flip64(c['l'], list(range(K)), hy, nb)[2], c['idx'])
    p = softmax64(c['l'])
    unmirrored = head64(0.5 * (p[:B] + p[B:][:, c['perm']]), hy, nb)[0]
    assert np.abs(unmirrored[..., 0] - c['kps'][..., 0]).min() > 1e-2
    own = head64(p, hy, nb)[2]
    assert not np.array_equal(own[:B], c['idx']) and not np.array_equal(own[B:][:, c['perm']], c['idx'])
    assert c['idx'][0, 0].tolist() != c['idx'][0, 3].tolist()            # the two joints of a pair


def test_second_bin_lanes_pick_the_planted_peaks():
    """D = 68 and 128: the averaged marginal's order is that of amp1 + amp2 = (6 + 4.5, 5 + 6, 4 + 5) at the planted bins."""
    assert case('d68_k1')['idx'][0, 0].tolist() == [30, 63, 50]
    assert case('d128_k1')['idx'][0, 0].tolist() == [100, 64, 58]
    for name in ('d68_k1', 'd128_k1'):
        D, K, B, pairs, hy, nb, groups, offset, bins0 = CASES[name]
        c = case(name)
        assert run_flip(c['lg'], c['perm_dev'], K, D, hy, nb, 1, 'logits')[1].cpu().tolist() == c['idx'].tolist()


def test_separate_normalisers_under_the_offset():
    """The offset case's logits sit near +80 and -80; softmax does not see an offset, so float64 gives what the case without
    one gives up to the float32 rounding of the inputs, and the kernel agrees with both."""
    a, b = case('d8'), case('d8_offset80')
    assert float(a['lg'].max()) < 12 and float(b['lg'][:1].min()) > 75 and float(b['lg'][1:].max()) < -68
    assert np.array_equal(a['idx'], b['idx']) and err(a['kps'], b['kps']) < 1e-4


@pytest.mark.parametrize('name', ['d8', 'd12_k5_groups3', 'd12_single', 'd64', 'd68_k1'])
def test_a_mirrored_pair_swapped_copy_gives_the_plain_head(name):
    """Image B + b holds exactly the mirrored, pair-swapped logits of image b: the average is image b's own heat-map, so the
    result is that of xas_head_softargmax_fwd on image b (same bars against its float64, identical indices)."""
    from xas_amd import ops_head
    from xas_amd._lib import call, ptr, query
    D, K, B, pairs, hy, nb, groups, offset, bins0 = CASES[name]
    c = case(name)
    first = c['l'][:B]
    l = np.concatenate([first, first[:, c['perm']][..., ::-1]])
    ref_kps, ref_pz, ref_idx, margin = head64(softmax64(first), hy, nb)
    assert margin > MARGIN
    lg = device_logits(l)
    kps1 = torch.empty(B, hy, K, 3, device='cuda')
    idx1 = torch.zeros(B, K, hy, device='cuda', dtype=torch.int64)
    dmap1 = torch.empty(groups, K, D, device='cuda')
    st = torch.empty(B, K, ops_head.HEAD_STATS, device='cuda')
    ws = torch.empty(query('xas_head_workspace_floats', B, K, D), device='cuda')
    call('xas_head_softargmax_fwd', ptr(lg[:B]), B, K, D, hy, nb, ptr(kps1), ptr(idx1), ptr(dmap1), groups, ptr(st), ptr(ws))
    bk, bd = bars(D)
    for source in SOURCES:
        kps, idx, dmap = run_flip(lg, c['perm_dev'], K, D, hy, nb, groups, source)
        check(name, 'mirrored copy, ' + source, D, kps, idx, dmap, ref_kps, ref_idx, ref_pz, nb, groups)
        assert torch.equal(idx, idx1)
        assert err(kps, kps1) <= bk and err(dmap, dmap1) <= bd


@pytest.mark.parametrize('name', ['d8_offset80', 'd12_k5_groups3', 'd64'])
def test_swapping_the_halves_mirrors_x_and_swaps_the_pairs(name):
    D, K, B, pairs, hy, nb, groups, offset, bins0 = CASES[name]
    c = case(name)
    bk, bd = bars(D)
    kps, idx, dmap = run_flip(c['lg'], c['perm_dev'], K, D, hy, nb, groups, 'logits')
    swapped = torch.cat([c['lg'][B:], c['lg'][:B]]).contiguous(memory_format=torch.channels_last)
    kps2, idx2, dmap2 = run_flip(swapped, c['perm_dev'], K, D, hy, nb, groups, 'logits')
    want = kps[:, :, c['perm']].clone()
    want[..., 0] = -want[..., 0] - 2.0 / D
    assert torch.equal(idx2, idx[:, c['perm']])
    assert err(kps2, want) <= bk and err(dmap2, dmap[:, c['perm']]) <= bd
    assert torch.equal(kps2[..., 1:], want[..., 1:]) and torch.equal(dmap2, dmap[:, c['perm']])    # a + b == b + a


@functools.lru_cache(maxsize=None)
def epilogue_case():
    """B = 1, K = 18, D = 64 (the shape xas_conv_fwd_head takes, as tests/test_gpu_head.py builds it): the planted logits of two
    images through an identity 1x1 convolution whose epilogue emits the records.  The reference is taken from the
    convolution's own output, which equals its input only to split-arithmetic accuracy."""
    from xas_amd import layers as L
    K, D, hy = 18, 64, 3
    perm = perm_of(HM36_PAIRS, K)
    x = device_logits(planted(D, K, 1, perm, hy, seed=811))
    conv = L.Conv2d(K * D, K * D, 1, bias=True).cuda()
    conv.head_kd = (K, D)
    with torch.no_grad():
        conv.weight.copy_(torch.eye(K * D).view(K * D, K * D, 1, 1))
        conv.bias.zero_()
        y = conv(x)
    assert getattr(y, '_xas_head', None) is not None
    assert float((y - x).abs().max()) < 2e-5 * float(x.abs().max())
    kps, pz, idx, margin = flip64(y.cpu().numpy().reshape(2, K, D, D, D), perm, hy, 15)
    return {'y': y, 'perm': perm, 'kps': kps, 'pz': pz, 'idx': idx, 'margin': margin}


def test_records_of_the_conv_epilogue_and_the_python_entry():
    """ops_head.softargmax_flip takes the epilogue's records when the logits carry them (64-pixel records: another summation
    order) and the logits otherwise; both agree with float64 of the same logits."""
    from xas_amd import ops_head, ops_nn
    K, D, hy, nb = 18, 64, 3, 15
    c = epilogue_case()
    assert c['margin'] > MARGIN
    perm = ops_head.flip_perm(HM36_PAIRS, K, 'cuda')
    assert perm.tolist() == c['perm']
    before = dict(ops_nn.head_stats)
    kps, dmap, idx = ops_head.softargmax_flip(c['y'], K, hy, nb, perm)
    assert ops_nn.head_stats['fused'] == before['fused'] + 1 and ops_nn.head_stats['separate'] == before['separate']
    assert kps.shape == (1, hy, K, 3) and dmap.shape == (K, D) and idx.shape == (1, K, hy) and idx.dtype == torch.int64
    check('d64_k18', 'epilogue records', D, kps, idx, dmap[None], c['kps'], c['idx'], c['pz'], nb)
    kps2, dmap2, idx2 = ops_head.softargmax_flip(c['y'].clone(memory_format=torch.preserve_format), K, hy, nb, c['perm'])
    assert ops_nn.head_stats['separate'] == before['separate'] + 1
    check('d64_k18', 'logits', D, kps2, idx2, dmap2[None], c['kps'], c['idx'], c['pz'], nb)
    with pytest.raises(RuntimeError, match='inference path'):
        ops_head.softargmax_flip(c['y'].clone(memory_format=torch.preserve_format).requires_grad_(True), K, hy, nb, perm)
    with pytest.raises(RuntimeError, match='perm must hold 18 joint indices'):
        ops_head.softargmax_flip(c['y'], K, hy, nb, torch.tensor([18] + c['perm'][1:], dtype=torch.int32, device='cuda'))
