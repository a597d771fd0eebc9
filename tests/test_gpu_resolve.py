"""xas_multiview_resolve on the MI355X against its float64 restatement (tests/_resolve_oracle.py), from the kernel up to
Eval.eval_batch and the result file.

Every input is built on the CPU (CASES, eval_case): exact projections of planted world points through float32 projection
matrices (the rigs of tests/test_gpu_tri_robust.py), sub-pixel noise, Hy = 3 depth hypotheses per view and joint of which the
one in slot (joint index mod Hy) is the planted point and the others lie 180 / 220 mm away along the viewing ray, and
left/right exchanges.  The views a pair is exchanged in are SEARCHED with the oracle alone, as plant() does there: the
candidate masks rotate with the pair's number and the first one under which the pair meets the oracle's condition is taken;
no pair is dropped.  tests/test_resolve_abi.py runs the condition over every case without a GPU.
"""
import functools

import numpy as np
import pytest
import torch

import _resolve_oracle as ro
from test_gpu_tri_robust import PlantedDetector, _cfg, hand_rig, scene_rig
from test_oracle_evalpath import scene

pytestmark = pytest.mark.gpu
S = 256.0
DISPLACED = (0.0, 180.0, -220.0)                  # mm along the ray, by (slot - planted slot) mod Hy
# planted point vs triangulated: 0.3 px of noise on both axes is at most 0.3 * sqrt(2) * 5500 mm / 1100 px = 2.1 mm across one
# view's ray, and the least-squares point of several rays lies no farther from the planted one than the worst of them
WORLD_TOL_MM = 3.0
PAIRS18 = ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13))      # eval_utils.py:8
PAIRS5 = ((1, 4), (0, 2))                         # joint 3 stands alone
PAIRS7 = ((1, 4), (0, 2), (3, 6))                 # joint 5 stands alone


# ------------------------------------------------------------------------------------------------ inputs (CPU only)
def perm_of(K, pairs):
    perm = list(range(K))
    for a, c in pairs:
        perm[a], perm[c] = c, a
    return perm


def fields(rig, pairs, seed, Hy=3, noise_px=0.3, noise_mm=2.0):
    """A rig (points, P, world points) -> a case with nothing exchanged: noisy points, kps whose (x, y) follow the points and
    whose z names the slot, single-view world points per slot, labels in patch pixels at the noise-free place."""
    pts, P, wp = rig
    rng = np.random.Generator(np.random.PCG64(seed))
    B, V, K, _ = pts.shape
    noisy = pts.copy()
    noisy[..., :2] += rng.uniform(-noise_px, noise_px, (B, V, K, 2)).astype(np.float32)
    P64 = P.astype(np.float64)
    centre = -np.einsum('bvij,bvj->bvi', np.linalg.inv(P64[..., :3]), P64[..., 3])
    ray = wp[:, None].astype(np.float64) - centre[:, :, None]
    ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
    kps, world = np.zeros((B, V, Hy, K, 3), np.float32), np.zeros((B, V, Hy, K, 3), np.float32)
    for k in range(K):
        for h in range(Hy):
            off = DISPLACED[(h - k) % Hy]
            world[:, :, h, k] = wp[:, None, k] + off * ray[:, :, k] + rng.normal(0.0, noise_mm, (B, V, 3))
            kps[:, :, h, k, :2] = (noisy[:, :, k, :2] - 512.0) / 600.0
            kps[:, :, h, k, 2] = off / 1000.0 + 0.01 * k
    gt = np.zeros((B, V, K, 3), np.float32)
    gt[..., :2] = ((pts[..., :2] - 512.0) / 600.0 + 1.0) / 2.0 * (S - 1.0)
    return dict(points=noisy, P=P, kps=kps, world=world, gt=gt, wp=wp, pairs=tuple(pairs), perm=perm_of(K, pairs),
                planted=np.zeros((B, K), np.uint8), slot=np.arange(K) % Hy)


def exchange(c, b, a, cc, mask):
    """Exchange joints a and cc of sample b in the views of `mask`, in everything a detector would exchange (not the labels)."""
    for v in range(c['points'].shape[1]):
        if mask >> v & 1:
            c['points'][b, v, [a, cc]] = c['points'][b, v, [cc, a]]
            c['kps'][b, v, :, [a, cc]] = c['kps'][b, v, :, [cc, a]]
            c['world'][b, v, :, [a, cc]] = c['world'][b, v, :, [cc, a]]
    c['planted'][b, [a, cc]] ^= np.uint8(mask)


def plant(c, anchor=False, every=3, cover=True):
    """Exchange every pair of the case in some of its valid views: the masks that leave the pair's lowest valid view alone
    (`anchor`, a flag or a function of (sample, lower joint): the masks that include it) rotate with the pair's number, every
    `every`-th pair stays as it is, and the first mask is taken under which the oracle finds the pair decidable and finds
    exactly that mask (`anchor`: its complement over the valid views, the consistent mirror naming)."""
    B, V, K, _ = c['points'].shape
    n = 0
    for b in range(B):
        for a, cc in c['pairs']:
            a, cc = min(a, cc), max(a, cc)
            n += 1
            if every and n % every == 0:
                continue
            w = c['points'][b, :, [a, cc], 2]
            valid = sum(1 << v for v in range(V) if np.isfinite(w[:, v]).all() and (w[:, v] > 0).all())
            low = valid & -valid
            anc = anchor(b, a) if callable(anchor) else anchor
            masks = [m for m in range(1, 1 << V) if not m & ~valid and bool(m & low) == anc and m != valid]
            for r in range(len(masks)):
                m = masks[(5 * n + r) % len(masks)]
                pa, pc = c['points'][b, :, a].copy(), c['points'][b, :, cc].copy()
                bit = np.array([m >> v & 1 for v in range(V)], bool)[:, None]
                s = ro.stage1(np.where(bit, pc, pa), np.where(bit, pa, pc), c['P'][b])
                if s['mask'] == (m ^ valid if anc else m) and s['cost_gap'] >= ro.MIN_COST_GAP_PX2 and s['cost_rel'] >= ro.MIN_COST_REL:
                    exchange(c, b, a, cc, m)
                    break
            else:
                raise AssertionError('no decidable exchange for pair (%d, %d) of sample %d' % (a, cc, b))
    seen = np.bitwise_or.reduce(c['planted'].ravel())
    full = (1 << V) - 1
    assert not cover or seen & (full & ~1) == full & ~1, 'not every view but the anchor carries an exchange somewhere'
    return c


def _coincident():
    c = fields(hand_rig(2, 4, 5, 45), PAIRS5, 145)
    for key in ('points', 'world'):                # joints 1 and 4 are one point in space: every exchange costs the same
        c[key][..., 4, :] = c[key][..., 1, :]
    c['kps'][..., 4, 2] = c['kps'][..., 1, 2] + 0.03                  # same slots as joint 1, told apart by z
    c['slot'] = c['slot'].copy()
    c['slot'][4] = c['slot'][1]
    return c


def _dead_view():
    c = fields(hand_rig(2, 4, 5, 46), PAIRS5, 146)
    c['points'][:, 2, :, :2] += 300.0              # view 2: garbage with weight 0
    c['points'][:, 2, :, 2] = 0.0
    c['points'][1, 0, 2, 2] = np.nan               # pair (0, 2) of sample 1 loses view 0 too: its anchor is view 1
    plant(c, every=0, cover=False)                 # exchanges among the views that are left ...
    exchange(c, 0, 1, 4, 0b0100)                   # ... and one in the dead view, which nobody may notice
    c['planted'] &= np.uint8(0b1011)
    return c


def _one_valid():
    c = fields(hand_rig(2, 3, 5, 47), PAIRS5, 147)
    c['points'][:, 1:, :, 2] = 0.0                 # only view 0 is valid ...
    c['points'][1, 0, 3, 2] = -1.0                 # ... and for the lone joint of sample 1 not even that
    return c


def _hm36(planted):
    pts, P, wp = scene_rig('hm36_best')
    c = fields((pts[:2], P[:2], wp[:2]), PAIRS18, 141 + planted)
    return plant(c) if planted else c


CASES = {
    'clean_hand': lambda: fields(hand_rig(2, 4, 5, 41), PAIRS5, 141),
    'clean_hm36': lambda: _hm36(0),
    'ex_v2': lambda: plant(fields(hand_rig(2, 2, 5, 42), PAIRS5, 142), every=2),
    'ex_v3': lambda: plant(fields(hand_rig(2, 3, 7, 43), PAIRS7, 143)),
    'ex_v4': lambda: _hm36(1),
    'ex_v6': lambda: plant(fields(hand_rig(2, 6, 7, 44), PAIRS7, 144), every=0),
    'anchor': lambda: plant(fields(hand_rig(2, 4, 7, 48), PAIRS7, 148), anchor=True, every=0, cover=False),
    'coincident': _coincident,
    'dead_view': _dead_view,
    'one_valid': _one_valid,
    'identity': lambda: fields(hand_rig(2, 4, 5, 49), (), 149),
    'k64': lambda: plant(fields(hand_rig(2, 3, 64, 50), ((1, 4), (2, 63), (0, 62)), 150), every=0),
    'k1': lambda: fields(hand_rig(2, 4, 1, 51), (), 151),
    'hy1': lambda: plant(fields(hand_rig(2, 3, 5, 52), PAIRS5, 152, Hy=1), every=0),
}
CLEAN = ('clean_hand', 'clean_hm36')
PLANTED = ('ex_v2', 'ex_v3', 'ex_v4', 'ex_v6')
WITH_GT = ('clean_hand', 'ex_v4', 'anchor', 'dead_view', 'one_valid', 'eval')


@functools.lru_cache(maxsize=None)
def case(name, gt=False):
    """(inputs, oracle result) of one case, computed once per process and shared; treat both as read-only."""
    c = CASES[name]() if name != 'eval' else eval_case()[1]
    return c, ro.resolve(c['points'], c['P'], c['kps'], c['world'], c['perm'], gt=c['gt'] if gt else None, image_size=S)


# --- Eval.eval_batch: the hm36 scene behind a planted detector
EVAL_Z = (0.0, 0.1, -0.12)                        # normalised depth by (slot - planted slot) mod 3: 0, 200 and -240 mm


@functools.lru_cache(maxsize=None)
def eval_case():
    """-> (x, the case).  Two samples of the hm36 scene; every camera's detections are the labels + 0.001 in the slot that
    rotates with the joint, the same (x, y) with another depth in the other slots; then exchanges, some in camera 0."""
    from oracle import evalpath as ev
    from oracle import geometry as og
    cams, _, x, _ = scene('hm36_best')
    x = {k: v[:2].clone() for k, v in x.items()}
    B, K, V, Hy = 2, 18, len(cams), 3
    pts, P, kps, world = [], [], [], []
    for c in cams:
        m = 'cam_%d' % c
        g = ev.normalise_gt(x[m + '_joints']) + 0.001
        det = g[:, None].repeat(1, Hy, 1, 1)
        for k in range(K):
            for h in range(Hy):
                det[:, h, k, 2] += EVAL_Z[(h - k) % Hy]
        cam = [x[m + s] for s in ('_trans_image', '_k_mat', '_pelvis', '_rot_world', '_trans_world')]
        kps.append(det)
        pts.append(ev.patch_to_image(det[:, 0], cam[0], cam[2]))
        world.append(torch.stack([og.patch_to_world(det[:, h], *cam) for h in range(Hy)], 1))
        P.append(cam[1] @ torch.cat([cam[3], cam[4].unsqueeze(-1)], -1))
    st = lambda ts: torch.stack(ts, 1).numpy().astype(np.float32).copy()
    gt = np.stack([x['cam_%d_joints' % c].numpy() for c in cams], 1)
    case_ = dict(points=st(pts), P=st(P), kps=st(kps), world=st(world), gt=gt, wp=x['world'].numpy(), pairs=PAIRS18,
                 perm=perm_of(K, PAIRS18), planted=np.zeros((B, K), np.uint8), slot=np.arange(K) % Hy)
    plant(case_, anchor=lambda b, a: b == 1 and a <= 3, every=0)          # the legs of sample 1 also in camera 0
    return x, case_


# ------------------------------------------------------------------------------------------------ the device side
def run(c, gt=False, want=('xyzw', 'swap', 'hyp', 'named')):
    from xas_amd import ops_eval
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = ops_eval.multiview_resolve(d(c['points']), d(c['P']), d(c['kps']), d(c['world']), pairs=c['pairs'],
                                     gt=d(c['gt']) if gt else None, image_size=S, want=want)
    return {k: v.cpu() for k, v in out.items()}


def dlt_of(points, P):
    from xas_amd import ops_eval
    return ops_eval.triangulate_dlt(torch.from_numpy(np.ascontiguousarray(points)).cuda(), torch.from_numpy(P).cuda()).cpu()


def resolved_points(c, swap):
    """The points with the exchanges of `swap` [B,K] applied: what stage 1 triangulated."""
    pts = c['points'].copy()
    B, V, K, _ = pts.shape
    for b in range(B):
        for k in range(K):
            for v in range(V):
                if int(swap[b, k]) >> v & 1:
                    pts[b, v, k] = c['points'][b, v, c['perm'][k]]
    return pts


def check_vs_oracle(name, gt=False):
    """What every case asserts: the oracle's swap, hyp, named and sel exactly (integers and gathered values), its float64
    solution within 2e-3 mm (the bound test_gpu_tri_robust.py holds xas_triangulate_robust to against the same DLT oracle:
    fp32 output rounding at |X| ~ 1e3), its mean weight."""
    c, o = case(name, gt)
    got = run(c, gt)
    assert set(got) == {'sel', 'xyzw', 'swap', 'hyp'} | ({'named'} if gt else set())
    for key in ('swap', 'hyp') + (('named',) if gt else ()):
        assert got[key].dtype == torch.uint8 and got[key].shape == o[key].shape
        assert np.array_equal(got[key].numpy(), o[key]), (name, key, got[key].numpy(), o[key])
    assert np.array_equal(got['sel'].numpy(), o['sel']), name
    xyz = got['xyzw'][..., :3].double().numpy()
    nan = np.isnan(o['xyz'])
    assert np.array_equal(np.isnan(xyz), nan)
    err = np.linalg.norm(np.where(nan, 0.0, xyz - o['xyz']), axis=-1).max()
    print('%s%s: |xyz - oracle| max %.3g mm, cost gap %.3g px^2 (rel %.3g), hypothesis margin %.3g mm' % (
        name, ' +gt' if gt else '', err, o['cost_gap'].min(), o['cost_rel'].min(), o['hyp_margin'].min()))
    assert err < 2e-3, (name, err)
    np.testing.assert_allclose(got['xyzw'][..., 3].numpy(), o['w'], rtol=1e-6, equal_nan=True)
    return c, o, got


def truth(c):
    """sel of a fully resolved case under the labels' naming: every joint's own kps in its planted slot.  The exchanges
    moved the data, so it is read back from where they put it."""
    B, V, Hy, K, _ = c['kps'].shape
    out = np.zeros((B, V, K, 3), np.float32)
    for b in range(B):
        for v in range(V):
            for k in range(K):
                s = c['perm'][k] if int(c['planted'][b, k]) >> v & 1 else k
                out[b, v, k] = c['kps'][b, v, c['slot'][k], s]
    return out


@pytest.mark.parametrize('name', CLEAN)
def test_nothing_exchanged(name):
    c, o, got = check_vs_oracle(name)
    assert (got['swap'] == 0).all()
    assert np.array_equal(got['hyp'].numpy(), np.broadcast_to(c['slot'], got['hyp'].shape))
    assert np.array_equal(got['sel'].numpy(), truth(c))
    assert torch.equal(got['xyzw'], dlt_of(c['points'], c['P']))
    assert np.linalg.norm(got['xyzw'][..., :3].numpy() - c['wp'], axis=-1).max() < WORLD_TOL_MM


@pytest.mark.parametrize('name', PLANTED)
def test_planted_exchanges_are_found(name):
    c, o, got = check_vs_oracle(name)
    assert np.array_equal(got['swap'].numpy(), c['planted']), (got['swap'].numpy(), c['planted'])
    assert np.array_equal(got['hyp'].numpy(), np.broadcast_to(c['slot'], got['hyp'].shape))
    assert np.array_equal(got['sel'].numpy(), truth(c))
    assert torch.equal(got['xyzw'], dlt_of(resolved_points(c, c['planted']), c['P']))        # bit for bit, mean weight included
    assert np.linalg.norm(got['xyzw'][..., :3].numpy() - c['wp'], axis=-1).max() < WORLD_TOL_MM
    hit = c['planted'] != 0
    off = np.linalg.norm(dlt_of(c['points'], c['P'])[..., :3].numpy() - c['wp'], axis=-1)
    assert off[hit].min() > 5.0, off[hit].min()                                               # unresolved, the DLT is pulled away


def test_anchor_exchanged_gives_the_mirror_naming_and_labels_name_it():
    c, o, got = check_vs_oracle('anchor')
    V = c['points'].shape[1]
    full = (1 << V) - 1
    paired = c['planted'] != 0
    assert paired.sum() == 2 * 2 * len(c['pairs']) and (c['planted'][paired] & 1).all()
    assert np.array_equal(got['swap'].numpy()[paired], c['planted'][paired] ^ full)           # view 0 kept its (wrong) naming
    mirror = truth(c)[:, :, c['perm']]
    assert np.array_equal(got['sel'].numpy(), mirror)
    assert np.linalg.norm(got['xyzw'][..., :3].numpy() - c['wp'][:, c['perm']], axis=-1).max() < WORLD_TOL_MM
    c, o, named = check_vs_oracle('anchor', gt=True)
    assert np.array_equal(named['named'].numpy(), paired.astype(np.uint8))
    assert np.array_equal(named['swap'].numpy(), c['planted'])
    assert np.array_equal(named['sel'].numpy(), truth(c))
    assert np.array_equal(named['hyp'].numpy(), np.broadcast_to(c['slot'], named['hyp'].shape))
    assert torch.equal(named['xyzw'], got['xyzw'][:, c['perm']])                              # the same two points, renamed


@pytest.mark.parametrize('name', ['clean_hand', 'ex_v4'])
def test_labels_leave_a_right_naming_alone(name):
    c, o, got = check_vs_oracle(name, gt=True)
    bare = run(c)
    assert (got['named'] == 0).all()
    for key in bare:
        assert torch.equal(got[key].view(torch.uint8), bare[key].view(torch.uint8)), key


def test_coincident_pair_is_mask_zero_by_the_tie_rule():
    c, o, got = check_vs_oracle('coincident')
    assert (got['swap'] == 0).all()
    assert torch.equal(got['xyzw'][:, 1], got['xyzw'][:, 4])
    assert np.array_equal(got['sel'].numpy()[:, :, [1, 4]], c['kps'][:, :, c['slot'][1]][:, :, [1, 4]])


def test_dead_views_are_never_exchanged_or_used_but_get_a_hypothesis():
    c, o, got = check_vs_oracle('dead_view')
    assert ((got['swap'] & 0b0100) == 0).all()
    assert np.array_equal(got['swap'].numpy(), c['planted']) and c['planted'][1, 0] == 0b1000 and (c['planted'][:, [0, 1]] != 0).all()
    hyp, live = np.broadcast_to(c['slot'], got['hyp'].shape), np.ones(got['hyp'].shape, bool)
    live[0, 2, [1, 4]] = False                     # the dead view's own exchange: there each joint gets the nearest slot of the other
    assert np.array_equal(got['hyp'].numpy()[live], hyp[live])
    assert np.linalg.norm(got['xyzw'][..., :3].numpy() - c['wp'], axis=-1).max() < WORLD_TOL_MM
    w = c['points'][..., 2]
    np.testing.assert_allclose(got['xyzw'][0, 3, 3], (w[0, 0, 3] + w[0, 1, 3] + w[0, 3, 3]) / 3, rtol=1e-6)
    c, o, named = check_vs_oracle('dead_view', gt=True)
    assert (named['named'] == 0).all() and torch.equal(named['sel'], got['sel'])


def test_fewer_than_two_valid_views_is_the_fallback():
    for gt in (False, True):
        c, o, got = check_vs_oracle('one_valid', gt)
        assert torch.isnan(got['xyzw'][..., :3]).all() and (got['swap'] == 0).all() and (got['hyp'] == 0).all()
        assert np.array_equal(got['sel'].numpy(), c['kps'][:, :, 0])
        assert got['xyzw'][0, 0, 3] == float(c['points'][0, 0, 0, 2]) and torch.isnan(got['xyzw'][1, 3, 3])
        assert not gt or (got['named'] == 0).all()


def test_unpaired_joints_are_the_plain_dlt():
    c, o, got = check_vs_oracle('identity')
    assert (got['swap'] == 0).all() and torch.equal(got['xyzw'], dlt_of(c['points'], c['P']))
    for name in ('ex_v3', 'ex_v6'):                # joint 5 of PAIRS7 stands alone among exchanged pairs
        c, _ = case(name)
        assert torch.equal(run(c)['xyzw'][:, 5], dlt_of(c['points'], c['P'])[:, 5])


@pytest.mark.parametrize('name', ['k64', 'k1', 'hy1'])
def test_lane_and_slot_bounds(name):
    c, o, got = check_vs_oracle(name)
    assert np.array_equal(got['swap'].numpy(), c['planted'])
    assert np.array_equal(got['sel'].numpy(), truth(c))
    assert torch.equal(got['xyzw'], dlt_of(resolved_points(c, c['planted']), c['P']))


def test_optional_outputs_and_two_launches():
    c, _ = case('ex_v6')
    full, again, bare = run(c), run(c), run(c, want=())
    assert set(bare) == {'sel'}
    for k in full:
        assert torch.equal(full[k].view(torch.uint8), again[k].view(torch.uint8)), k
    assert torch.equal(bare['sel'], full['sel'])
    only = run(c, want=('hyp',))
    assert set(only) == {'sel', 'hyp'} and torch.equal(only['hyp'], full['hyp'])


def test_refusals_name_the_limit():
    from xas_amd import ops_eval
    t = lambda *s: torch.ones(*s).cuda()
    args = lambda V, K=3, Hy=2: (t(1, V, K, 3), t(1, V, 3, 4), t(1, V, Hy, K, 3), t(1, V, Hy, K, 3))
    with pytest.raises(RuntimeError, match=r'V=1 views \(needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6\)'):
        ops_eval.multiview_resolve(*args(1), pairs=())
    with pytest.raises(RuntimeError, match=r'V=7 views \(needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6\)'):
        ops_eval.multiview_resolve(*args(7), pairs=())
    with pytest.raises(RuntimeError, match=r'K=65 joints \(needs 1 <= K <= 64\)'):
        ops_eval.multiview_resolve(*args(3, K=65), pairs=())
    p, P, k, w = args(3)
    with pytest.raises(RuntimeError, match='do not match points'):
        ops_eval.multiview_resolve(p, t(1, 4, 3, 4), k, w)
    with pytest.raises(RuntimeError, match='world .* and kps .* differ'):
        ops_eval.multiview_resolve(p, P, k, t(1, 3, 3, 3, 3), pairs=())
    with pytest.raises(RuntimeError, match='labels .* do not match'):
        ops_eval.multiview_resolve(p, P, k, w, pairs=(), gt=t(1, 3, 4, 3))


def test_eval_select_no_switch_keeps_every_joint():
    from xas_amd import ops_eval
    cams, mode, x, kps = scene('hm36_best')
    k, j = kps['cam_0'][:, :1].cuda(), x['cam_0_joints'].cuda()
    plain = ops_eval.eval_select(k, j)
    kept = ops_eval.eval_select(k, j, no_switch=True)
    assert plain['swapped'].any() and not kept['swapped'].any()
    assert torch.equal(kept['sel3d'], k[:, 0]) and not torch.equal(plain['sel3d'], k[:, 0])
    from oracle import evalpath as ev
    want = ev.per_act_mse(kps['cam_0'][:, 0, :, :2], ev.normalise_gt(x['cam_0_joints'])[..., :2])
    torch.testing.assert_close(kept['err2d'].cpu(), want, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------ Eval
def _eval_setup():
    x, c = eval_case()
    cams = [0, 1, 2, 3]
    xd = {k: v.cuda() for k, v in x.items()}
    for cam in cams:
        xd['cam_%d_img' % cam] = torch.zeros(1, 3, 256, 256, device='cuda')
    return cams, xd, {'cam_%d' % cam: torch.from_numpy(c['kps'][:, i].copy()).cuda() for i, cam in enumerate(cams)}, c


def _today_keys(cams):
    names = ['tri'] + ['view_cam_%d' % c for c in cams]
    return {'err2d_cam_%d' % c for c in cams} | {'ambiguity', 'world_gt', 'world_tri'} | {
        '%s_%s' % (m, n) for m in ('mpjpe', 'n-mpjpe', 'p-mpjpe', 'pck', 'auc') for n in names}


def test_eval_batch_views_agrees_with_the_labels_choice(tmp_path):
    import eval as xeval
    from modules import util as mu
    from xas_amd import ops_eval
    cams, xd, kps, c = _eval_setup()
    _, o = case('eval', True)
    sel, r = mu.resolve_views(kps, xd, cams, ops_eval.SWITCH_PAIRS)
    assert np.array_equal(r['swap'].cpu().numpy(), c['planted']) and np.array_equal(r['named'].cpu().numpy(), o['named'])
    assert o['named'][1, [1, 2, 3, 4, 5, 6]].all() and not o['named'][0].any()
    assert np.array_equal(r['hyp'].cpu().numpy(), np.broadcast_to(c['slot'], r['hyp'].shape))
    assert (r['valid'] == 15).all()
    for m in kps:                                                             # the same element of the same tensor, bit for bit
        best = ops_eval.eval_select(kps[m], xd[m + '_joints'], mode='best')['sel3d']
        assert torch.equal(sel[m], best), m
    mk = lambda **kw: xeval.Eval(_cfg(cams), PlantedDetector(), [], str(tmp_path), **kw)
    best = mk().eval_batch(xd, 'best', kps_by_cam=kps)
    conf = mk(resolve='gt').eval_batch(xd, 'confident', kps_by_cam=kps)
    views = mk(resolve='views').eval_batch(xd, 'confident', kps_by_cam=kps)                    # the mode is ignored
    assert set(best) == _today_keys(cams) == set(conf)
    assert set(views) == set(best) | {'resolve_exchanged', 'resolve_hyp0'}
    moved = 0
    for k in best:
        if k.split('_')[0] in ('mpjpe', 'n-mpjpe', 'p-mpjpe'):
            torch.testing.assert_close(views[k], best[k], rtol=1e-5, atol=1e-4)
            moved += int((conf[k] - best[k]).abs().max() > 1.0)
    assert moved >= 3 * len(cams), moved                                      # the control: hypothesis 0 is not the answer
    for m in kps:
        torch.testing.assert_close(views['err2d_' + m], best['err2d_' + m], rtol=1e-6, atol=1e-9)
    bits = lambda a: np.array([[bin(int(t)).count('1') for t in row] for row in a])
    before = np.where(o['named'] == 1, bits(o['valid']) - bits(o['swap']), bits(o['swap']))
    paired = np.array(c['perm']) != np.arange(18)
    assert abs(float(views['resolve_exchanged']) - before[:, paired].mean() / 4) < 1e-6 and float(views['resolve_exchanged']) > 0.1
    assert abs(float(views['resolve_hyp0']) - (o['hyp'] == 0).mean()) < 1e-6
    trans = torch.from_numpy(bits(o['swap'])).float()
    assert abs(float(views['ambiguity']) - float(torch.minimum(trans, 4 - trans).mean())) < 1e-6


def test_result_file_gains_one_line_with_views_only(tmp_path):
    import eval as xeval
    cams, xd, kps, c = _eval_setup()
    det = PlantedDetector()
    det.kps = {0: kps['cam_0'], 1: kps['cam_1'], 2: kps['cam_2'], 3: kps['cam_3']}
    for i, cam in enumerate(cams):
        xd['cam_%d_img' % cam] = torch.full((1, 3, 256, 256), float(i), device='cuda')
    texts = {}
    for tag, kw in (('none', {}), ('gt', dict(resolve='gt')), ('views', dict(resolve='views'))):
        e = xeval.Eval(_cfg(cams), det, [dict(xd), dict(xd)], str(tmp_path / tag), **kw)
        lines = e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt', 'rb').read()
        assert texts[tag].decode().strip().split('\n') == lines
    assert texts['gt'] == texts['none']
    old, new = texts['none'].decode().strip().split('\n'), texts['views'].decode().strip().split('\n')
    assert len(new) == len(old) + 1 and new[-1].startswith('RESOLVE views: exchanged 0.') and ', hypothesis 0 kept 0.3' in new[-1]
    assert new[:-1] == old                                                    # the same figures from the same joints, digit for digit
    with pytest.raises(ValueError, match='Unknown resolve mode'):
        xeval.Eval(_cfg(cams), det, [], str(tmp_path), resolve='labels')
    with pytest.raises(ValueError, match="needs 2 to 6 of them; cam_id_list has 1"):
        xeval.Eval(_cfg([0]), det, [], str(tmp_path), resolve='views')
