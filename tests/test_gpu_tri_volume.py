"""xas_triangulate_volume on the MI355X against its float64 restatement (tests/_volume_oracle.py), from the kernel up to
modules.util.triangulation_volume and the detectors' forward_logits.

Shapes are small and still reach every branch: B = 2, K = 3 (the channel stride K * D is no power of two), D in {8, 12},
V in {2, 3, 5}, G in {4, 7, 16} (64, 343 and 4096 voxels: fewer than, no multiple of and more than the 256 threads of a
workgroup), levels in {1, 3}.

Bars.  Both sides work in double from the same float32 inputs and the function is continuous in them, so they differ by the
order of the sums over at most 32^3 terms (about 1e-9 mm) and the one final rounding to float32:
  xyz   2 ulp_fp32(max |coordinate| of the joint) + 1e-6 mm
  cov   4 ulp_fp32 of the joint's largest |entry|
  status  equal, asserted only where the oracle's `lead` (the relative gap between the best face voxel and the best inner
          voxel) is above 1e-9; every case below is built to be far from that.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _volume_inputs as vi
import _volume_oracle as vo
from test_volume_oracle import BIMODAL, BIMODAL_GRID

pytestmark = pytest.mark.gpu
B, K = 2, 3
POISON_F, POISON_B = 12345.0, 0xAB


def ulp32(x):
    return float(np.spacing(np.float32(np.max(np.abs(x)))))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def nhwc(l):
    """numpy [B,H,W,K*D] -> the logical [B,K*D,H,W] device tensor over that same storage order."""
    return torch.from_numpy(l).cuda().permute(0, 3, 1, 2)


CAM_KEYS = ('trans_image', 'k_mat', 'pelvis', 'rot_world', 'trans_world')


def run(c, init=None, chan=None, views=None, weight=None, logits=None, cams=None, **kw):
    """ops_eval.triangulate_volume on a case of _volume_inputs -> numpy dict (xyz, cov, status)."""
    from xas_amd import ops_eval
    d = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a if dt is None else a.astype(dt))).cuda()
    cams = c['cams'] if cams is None else cams
    out = ops_eval.triangulate_volume([nhwc(l) for l in (c['logits'] if logits is None else logits)], d(chan, np.int32),
                                      *[d(cams[k]) for k in CAM_KEYS], d(c['init'] if init is None else init),
                                      views=d(views, np.uint8), weight=d(weight, np.float32), want=('cov', 'status'), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def oracle(c, init=None, chan=None, views=None, weight=None, logits=None, cams=None, **kw):
    return vo.fuse(c['logits'] if logits is None else logits, chan, c['cams'] if cams is None else cams,
                   c['init'] if init is None else init, views=views, weight=weight, **kw)


def check(got, want, what=''):
    """The bars of the module docstring, joint by joint."""
    assert got['xyz'].dtype == np.float32 and got['cov'].dtype == np.float32 and got['status'].dtype == np.uint8
    decided = want['lead'] > vo.STATUS_MIN_LEAD
    assert decided.all(), '%s: a status hangs on the last bits of a score (lead %.3e)' % (what, want['lead'].min())
    assert np.array_equal(got['status'], want['status']), (what, got['status'], want['status'])
    worst = [0.0, 0.0]
    for b in range(want['xyz'].shape[0]):
        for k in range(want['xyz'].shape[1]):
            if want['status'][b, k] in (1, 3):
                assert np.array_equal(bits(got['xyz'][b, k]), bits(want['xyz'][b, k].astype(np.float32))) and np.isnan(got['cov'][b, k]).all()
                continue
            ex = np.abs(got['xyz'][b, k].astype(np.float64) - want['xyz'][b, k]).max()
            bx = 2 * ulp32(want['xyz'][b, k]) + 1e-6
            ec = np.abs(got['cov'][b, k].astype(np.float64) - want['cov'][b, k]).max()
            bc = 4 * ulp32(want['cov'][b, k])
            worst = [max(worst[0], ex / bx), max(worst[1], ec / bc)]
            assert ex <= bx, '%s: xyz[%d,%d] off by %.3e mm (bar %.3e)' % (what, b, k, ex, bx)
            assert ec <= bc, '%s: cov[%d,%d] off by %.3e mm^2 (bar %.3e)' % (what, b, k, ec, bc)
    print('%s: xyz at %.2f of its bar, cov at %.2f' % (what, *worst))


@functools.lru_cache(maxsize=None)
def case(V, D, seed, inside=None):
    return vi.case(B, V, K, D, seed, inside=inside)


GRIDS = {   # name: (V, D, G, levels, side_mm)
    'v2_d8_g4_l1': (2, 8, 4, 1, 1200.0),
    'v3_d12_g7_l3': (3, 12, 7, 3, 1000.0),
    'v5_d8_g16_l1': (5, 8, 16, 1, 1600.0),
    'v5_d12_g16_l3': (5, 12, 16, 3, 1000.0),
    'v2_d12_g7_l1': (2, 12, 7, 1, 1400.0),
    'v3_d8_g4_l3': (3, 8, 4, 3, 1200.0),
}


@pytest.mark.parametrize('name', sorted(GRIDS))
def test_kernel_matches_the_oracle(name):
    V, D, G, levels, side = GRIDS[name]
    c = case(V, D, 100 + V + D)
    kw = dict(G=G, levels=levels, side_mm=side, beta=0.8, out_penalty=1.5)
    check(run(c, **kw), oracle(c, **kw), name)


def test_chan_views_and_weight_together_match_the_oracle():
    c = case(5, 12, 131)
    rng = np.random.Generator(np.random.PCG64(7))
    chan = np.stack([np.stack([rng.permutation(K) for _ in range(B)]) for _ in range(5)]).astype(np.int32)
    views = np.array([[0b11111, 0b10110, 0b01011], [0b00111, 0b11101, 0b11000]], np.uint8)
    weight = rng.uniform(0.3, 2.0, (5, B, K)).astype(np.float32)
    weight[4, 0, 0], weight[0, 1, 1], weight[2, 1, 0] = 0.0, np.inf, np.nan          # these views drop out
    kw = dict(G=7, levels=2, side_mm=1000.0)
    check(run(c, chan=chan, views=views, weight=weight, **kw), oracle(c, chan=chan, views=views, weight=weight, **kw), 'mixed')


def test_mode_outside_the_grid_is_status_2():
    c = case(3, 12, 115)
    init = c['world'] + np.array([600.0, 0.0, 0.0], np.float32)
    kw = dict(G=7, levels=1, side_mm=400.0)
    want = oracle(c, init=init, **kw)
    assert (want['status'] == 2).all()
    check(run(c, init=init, **kw), want, 'outside')
    inner = oracle(c, **dict(kw, side_mm=1000.0))                      # and the same cubes from the DLT point: 0
    assert (inner['status'] == 0).all()
    check(run(c, **dict(kw, side_mm=1000.0)), inner, 'inside')


def test_bimodal_view_lands_where_the_oracle_does():
    c = vi.case(**BIMODAL)
    want = oracle(c, **BIMODAL_GRID)
    got = run(c, **BIMODAL_GRID)
    check(got, want, 'bimodal')
    voxel = BIMODAL_GRID['side_mm'] / BIMODAL_GRID['G'] / 2 ** (BIMODAL_GRID['levels'] - 1)
    assert np.linalg.norm(got['xyz'] - c['init'], axis=-1).min() > 2 * voxel      # far from the DLT start
    assert np.linalg.norm(got['xyz'] - c['world'], axis=-1).max() < voxel / 2     # at the planted point


def test_chan_undoes_an_exchange_bit_for_bit():
    c = case(3, 12, 115)
    kw = dict(G=7, levels=2, side_mm=1000.0)
    plain = run(c, **kw)
    D = c['D']
    swapped = [l.copy() for l in c['logits']]
    swapped[1][..., 0:D], swapped[1][..., D:2 * D] = c['logits'][1][..., D:2 * D], c['logits'][1][..., 0:D]
    chan = np.tile(np.arange(K, dtype=np.int32), (3, B, 1))
    chan[1, :, 0], chan[1, :, 1] = 1, 0
    told = run(c, logits=swapped, chan=chan, **kw)
    untold = run(c, logits=swapped, **kw)
    for key in ('xyz', 'cov', 'status'):
        assert np.array_equal(bits(told[key]), bits(plain[key])), key
    assert not np.array_equal(untold['xyz'][:, :2], plain['xyz'][:, :2]) and np.array_equal(bits(untold['xyz'][:, 2]), bits(plain['xyz'][:, 2]))


def test_masked_view_is_a_dropped_view_and_weight_two_is_the_view_twice():
    c = case(3, 12, 115)
    kw = dict(G=7, levels=2, side_mm=1000.0)
    sub = lambda idx: dict(logits=[c['logits'][v] for v in idx], cams={k: c['cams'][k][list(idx)] for k in CAM_KEYS})
    masked = run(c, views=np.full((B, K), 0b101, np.uint8), **kw)
    dropped = run(c, **sub((0, 2)), **kw)
    weight = np.ones((3, B, K), np.float32)
    weight[1] = 2.0
    heavy = run(c, weight=weight, **kw)
    twice = run(c, **sub((0, 1, 1, 2)), **kw)
    for key in ('xyz', 'cov', 'status'):
        assert np.array_equal(bits(masked[key]), bits(dropped[key])), key
    # w + w rounds as 2 w does, but the sum reaches view 2 with another rounding history: equal to the bar, not to the bit
    check(heavy, dict(xyz=twice['xyz'].astype(np.float64), cov=twice['cov'].astype(np.float64), status=twice['status'],
                      lead=np.full((B, K), np.inf)), 'weight 2 vs twice')
    assert not np.array_equal(heavy['xyz'], run(c, **kw)['xyz'])


def test_voxels_outside_a_cube_and_behind_a_camera():
    c = case(3, 8, 141)
    kw = dict(G=7, levels=2, side_mm=5000.0, out_penalty=0.25)          # a 5 m grid round a 2 m cube
    off, _ = vo.voxel_offsets(7, 5000.0)
    w, h, d, z = vo.world_to_cube(c['cams'], 0, 0, c['init'][0, 0].astype(np.float64) + off, 8, vi.S, vi.RECT)
    assert (w < 0).any() and (w > 7).any() and (h < 0).any() and (h > 7).any() and (d < 0).any() and (d > 7).any() and (z > 0).all()
    check(run(c, **kw), oracle(c, **kw), 'outside a cube')
    c = case(3, 8, 151, inside=(1, 150.0))                              # camera 1 stands 150 mm from the origin
    kw = dict(G=7, levels=2, side_mm=1200.0)
    z = vo.world_to_cube(c['cams'], 1, 0, c['init'][0, 0].astype(np.float64) + vo.voxel_offsets(7, 1200.0)[0], 8, vi.S, vi.RECT)[3]
    assert (z <= 0).any() and (z > 0).any()
    check(run(c, **kw), oracle(c, **kw), 'behind a camera')


def test_pass_through_is_init_bit_for_bit():
    kw = dict(G=4, levels=1, side_mm=1200.0)
    one = vi.case(B, 1, K, 8, 161)
    got = run(one, **kw)
    assert (got['status'] == 1).all() and np.array_equal(bits(got['xyz']), bits(one['init'])) and np.isnan(got['cov']).all()
    c = case(3, 8, 141)
    init = c['init'].copy()
    init[0, 1, 2], init[1, 0, 0] = np.nan, np.inf
    got, ref = run(c, init=init, **kw), run(c, **kw)
    assert got['status'][0, 1] == 1 and got['status'][1, 0] == 1
    for b, k in ((0, 1), (1, 0)):
        assert np.array_equal(bits(got['xyz'][b, k]), bits(init[b, k])) and np.isnan(got['cov'][b, k]).all()
    keep = np.ones((B, K), bool)
    keep[0, 1] = keep[1, 0] = False
    for key in ('xyz', 'cov', 'status'):
        assert np.array_equal(bits(got[key][keep]), bits(ref[key][keep])), key
    check(got, oracle(c, init=init, **kw), 'nan init')


def test_a_logit_that_is_not_finite_stops_its_joint_only():
    c = case(3, 12, 115)
    kw = dict(G=7, levels=2, side_mm=1000.0)
    ref = run(c, **kw)
    D = c['D']
    w, h, d = np.clip(np.round(vi.cube_coords(c['cams'], c['world'], D)[0, 0, 1]).astype(int), 0, D - 1)   # view 0, b 0, joint 1
    for bad in (np.nan, np.inf):
        logits = [l.copy() for l in c['logits']]
        logits[0][0, h, w, 1 * D + d] = bad
        got = run(c, logits=logits, **kw)
        assert got['status'][0, 1] == 3 and np.array_equal(bits(got['xyz'][0, 1]), bits(c['init'][0, 1])) and np.isnan(got['cov'][0, 1]).all()
        keep = np.ones((B, K), bool)
        keep[0, 1] = False
        for key in ('xyz', 'cov', 'status'):
            assert np.array_equal(bits(got[key][keep]), bits(ref[key][keep])), key
        assert (oracle(c, logits=logits, **kw)['status'] == got['status']).all()


def _raw(c, xyz, cov, status, **over):
    """The C entry itself on caller-owned output buffers -> its return code."""
    from xas_amd import _lib
    V = len(c['logits'])
    keep = [nhwc(l) for l in c['logits']] + [torch.from_numpy(c['cams'][k]).cuda() for k in CAM_KEYS] + [torch.from_numpy(c['init']).cuda()]
    a = dict(B=B, V=V, K=K, D=c['D'], G=7, levels=2, side_mm=1000.0, beta=1.0, out_penalty=1.0, image_size=256.0, rect_width=2000.0)
    a.update(over)
    table = (ctypes.c_void_p * V)(*[t.data_ptr() for t in keep[:V]])
    rc = _lib.fn('xas_triangulate_volume')(table, None, *[t.data_ptr() for t in keep[V:V + 5]], keep[V + 5].data_ptr(), None, None,
                                           a['B'], a['V'], a['K'], a['D'], a['G'], a['levels'], a['side_mm'], a['beta'], a['out_penalty'],
                                           a['image_size'], a['rect_width'], xyz.data_ptr(), cov.data_ptr(), status.data_ptr(),
                                           _lib.stream())
    torch.cuda.synchronize()
    return rc


def _poisoned():
    return (torch.full((B, K, 3), POISON_F, device='cuda'), torch.full((B, K, 6), POISON_F, device='cuda'),
            torch.full((B, K), POISON_B, device='cuda', dtype=torch.uint8))


def test_two_calls_agree_bit_for_bit_and_every_output_is_written():
    c = case(5, 12, 131)
    first, second = _poisoned(), _poisoned()
    assert _raw(c, *first, G=16, levels=3) == 0 and _raw(c, *second, G=16, levels=3) == 0
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert not (first[0] == POISON_F).any() and not (first[1] == POISON_F).any() and not (first[2] == POISON_B).any()
    one = vi.case(B, 1, K, 8, 161)                                    # passed through: written as well
    out = _poisoned()
    assert _raw(one, *out) == 0
    assert not (out[0] == POISON_F).any() and torch.isnan(out[1]).all() and (out[2] == 1).all()


@pytest.mark.parametrize('over,msg', [
    (dict(D=6), 'D=6'), (dict(D=2), 'D=2'), (dict(D=132), 'D=132'),
    (dict(V=0), 'V=0 views'), (dict(V=7), 'V=7 views (needs 1 <= V <= XAS_TRI_MAX_VIEWS = 6)'),
    (dict(G=1), 'G=1'), (dict(G=33), 'G=33'), (dict(levels=0), 'levels=0'), (dict(levels=5), 'levels=5'),
    (dict(side_mm=0.0), 'side_mm'), (dict(side_mm=float('inf')), 'side_mm'), (dict(side_mm=float('nan')), 'side_mm'),
    (dict(beta=-1.0), 'beta'), (dict(beta=float('nan')), 'beta'),
    (dict(out_penalty=0.0), 'out_penalty'), (dict(out_penalty=float('inf')), 'out_penalty'),
])
def test_refusals_launch_nothing(over, msg):
    from xas_amd import _lib
    c = case(3, 12, 115)
    out = _poisoned()
    assert _raw(c, *out, **over) == 1
    assert msg in _lib.load().xas_last_error().decode()
    assert (out[0] == POISON_F).all() and (out[1] == POISON_F).all() and (out[2] == POISON_B).all()


def test_python_wrapper_refuses_what_does_not_fit():
    from xas_amd import ops_eval
    c = case(3, 12, 115)
    with pytest.raises(RuntimeError, match=r'V=7 views \(needs 1 <= V <= XAS_TRI_MAX_VIEWS = 6\)'):
        run(c, logits=[c['logits'][0]] * 7)
    with pytest.raises(RuntimeError, match='G=40'):
        run(c, G=40)
    with pytest.raises(RuntimeError, match='chan'):
        run(c, chan=np.zeros((3, B), np.int32))
    assert (ops_eval.TRI_VOL_G, ops_eval.TRI_VOL_LEVELS, ops_eval.TRI_VOL_SIDE_MM) == (16, 2, 800.0)


# ------------------------------------------------------------------------------------------------ the Python layer
def _batch_dict(c, cams):
    x = {}
    for i, cam in enumerate(cams):
        for k in CAM_KEYS:
            x['cam_%d_%s' % (cam, k)] = torch.from_numpy(c['cams'][k][i]).cuda()
        x['cam_%d_img' % cam] = torch.zeros(B, 3, 256, 256, device='cuda')
    return x


def test_triangulation_volume_is_the_direct_call():
    from modules import util as mu
    c = vi.case(B, 4, K, 12, 171)
    cams = [0, 1, 2, 5]
    x = _batch_dict(c, cams)
    logits = {'cam_%d' % cam: nhwc(c['logits'][i]) for i, cam in enumerate(cams)}
    chan = np.tile(np.arange(K, dtype=np.int32), (4, B, 1))
    chan[2, 1, 0], chan[2, 1, 1] = 1, 0
    views = np.array([[15, 7, 13], [15, 15, 6]], np.uint8)
    kw = dict(G=7, levels=2, side_mm=1000.0)
    xyz, r = mu.triangulation_volume(torch.from_numpy(c['init']).cuda(), logits, x, cams, torch.from_numpy(chan).cuda(),
                                     views=torch.from_numpy(views).cuda(), want=('cov', 'status'), **kw)
    direct = run(c, chan=chan, views=views, **kw)
    assert set(r) == {'xyz', 'cov', 'status', 'init'} and xyz is r['xyz']
    for key in ('xyz', 'cov', 'status'):
        assert np.array_equal(bits(r[key].cpu().numpy()), bits(direct[key])), key
    check(direct, oracle(c, chan=chan, views=views, **kw), 'batch dict')
    # a dict of patch predictions is triangulated by the DLT first: the start it reports is that DLT
    S = 256.0
    sel = {}
    for i, cam in enumerate(cams):
        coords = vi.cube_coords(c['cams'], c['world'], 12)[i]
        sel['cam_%d' % cam] = torch.from_numpy((coords / 12.0 * 2.0 - 1.0).astype(np.float32)).cuda()
    _, r2 = mu.triangulation_volume(sel, logits, x, cams, **kw)
    assert torch.equal(r2['init'], mu.triangulation(sel, x, cams)[..., :3])


@functools.lru_cache(maxsize=None)
def _detector(multi):
    import inputs as gi
    from modules.keypoint_detector_integral import KPDetector3D
    from modules.keypoint_detector_integral_multi import KPDetector3DMulti
    det = KPDetector3DMulti('resnet_multi', 18, 16, 3, 15, num_layers=18) if multi else KPDetector3D('resnet', 18, 16, num_layers=18)
    gi.seeded_fill_(det, seed=81)
    return det.cuda().eval()


@pytest.mark.parametrize('multi', [True, False])
def test_forward_logits_is_forward_plus_the_cubes(multi):
    det = _detector(multi)
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(82)).cuda()
    with torch.no_grad():
        kps, dmap = det(x)
    kps2, dmap2, logits = det.forward_logits(x)
    assert torch.equal(kps.view(torch.int32), kps2.view(torch.int32)) and torch.equal(dmap.view(torch.int32), dmap2.view(torch.int32))
    assert logits.shape == (B, 18 * 16, 16, 16) and logits.is_contiguous(memory_format=torch.channels_last) and not logits.requires_grad
    # the op takes the tensor as it is, and reads it in the layout the oracle reads
    cams = vi.rig(B, 2, 83)
    init = vi.planted(B, 18, 84)
    l = logits.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    c = dict(cams=cams, init=init, logits=[l, l], D=16)
    from xas_amd import ops_eval
    out = ops_eval.triangulate_volume([logits, logits], None, *[torch.from_numpy(cams[k]).cuda() for k in CAM_KEYS],
                                      torch.from_numpy(init).cuda(), G=4, levels=1, side_mm=1000.0, want=('cov', 'status'))
    want = oracle(c, G=4, levels=1, side_mm=1000.0)
    ok = want['lead'] > vo.STATUS_MIN_LEAD
    assert np.array_equal(out['status'].cpu().numpy()[ok], want['status'][ok])
    err = np.abs(out['xyz'].cpu().numpy() - want['xyz']).max(axis=-1)
    assert (err <= 2 * np.spacing(np.abs(want['xyz']).max(axis=-1).astype(np.float32)) + 1e-6).all()
