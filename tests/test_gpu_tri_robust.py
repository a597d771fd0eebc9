"""xas_triangulate_robust on the MI355X against its float64 restatement (tests/_tri_oracle.py), from the kernel up to
Eval.eval_batch and the result file.

Every input is built on the CPU (CASES, eval_case): exact projections of planted world points through float32 projection
matrices, then outliers, dead views and noise on top.  tests/test_tri_robust_abi.py runs the oracle's decidability condition
over all of them without a GPU.  Where outliers are planted, the (joint, view) choices are SEARCHED with the oracle alone: the
joints are walked in order, the view rotates with the joint index, and the first choice whose every residual keeps 1 px from
the threshold is taken (for a fixed choice about two in three joints have some residual of some subset in that 2-px window).
"""
import functools

import numpy as np
import pytest
import torch

import _tri_oracle as to
import inputs as gi
from test_oracle_evalpath import scene

pytestmark = pytest.mark.gpu
SHIFTS = ((60.0, -45.0), (-45.0, -60.0))          # px; the second one only where two views are corrupted
THR = 20.0


# ------------------------------------------------------------------------------------------------ inputs (CPU only)
def project(P, world, weight=None):
    """Exact (u, v) of world [B,K,3] in float64 through the float32 P [B,V,3,4]; weight = depth (what the reference uses)."""
    wh = np.concatenate([world.astype(np.float64), np.ones(world.shape[:2] + (1,))], -1)
    h = np.einsum('bvij,bkj->bvki', P.astype(np.float64), wh)
    w = h[..., 2] if weight is None else np.broadcast_to(weight, h[..., 2].shape)
    return np.stack([h[..., 0] / h[..., 2], h[..., 1] / h[..., 2], w], -1).astype(np.float32)


def scene_rig(tag):
    cams, _, x, _ = scene(tag)
    P = torch.stack([x['cam_%d_k_mat' % c] @ torch.cat([x['cam_%d_rot_world' % c], x['cam_%d_trans_world' % c].unsqueeze(-1)], -1)
                     for c in cams], 1).numpy()
    world = x['world'].numpy()
    return project(P, world), P, world


def hand_rig(B, V, K, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    world = rng.normal(0.0, 350.0, (B, K, 3)).astype(np.float32)
    P = np.zeros((B, V, 3, 4), np.float32)
    for b in range(B):
        for v in range(V):
            R = gi.random_rotation(rng)
            t = np.array([rng.uniform(-300, 300), rng.uniform(-300, 300), rng.uniform(4500, 5500)])
            fx, fy, cx, cy = rng.uniform(1100, 1200), rng.uniform(1100, 1200), rng.uniform(480, 540), rng.uniform(480, 540)
            P[b, v] = (np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]) @ np.concatenate([R, t[:, None]], 1)).astype(np.float32)
    return project(P, world), P, world


def plant(pts, P, n_views, total, thr=THR, scale=1.0, cover=True):
    """Shift (u, v) of `n_views` views by scale * SHIFTS for `total` joints of the batch -> (points, planted [B,K] bit masks).
    `cover`: every view must carry an outlier somewhere."""
    pts = pts.copy()
    B, V, K, _ = pts.shape
    planted = np.zeros((B, K), np.uint8)
    for b in range(B):
        for k in range(K):
            if np.count_nonzero(planted) >= total:
                break
            choices = [((k + r) % V,) for r in range(V)] if n_views == 1 else \
                [((k + r) % V, (k + r + 1 + s) % V) for r in range(V) for s in range(V - 1)]
            for views in choices:
                p = pts[b, :, k].copy()
                for v, (du, dv) in zip(views, SHIFTS):
                    p[v, 0] += np.float32(scale * du)
                    p[v, 1] += np.float32(scale * dv)
                if to.decidable_one(p, P[b], thr):
                    pts[b, :, k] = p
                    planted[b, k] = sum(1 << v for v in views)
                    break
    assert np.count_nonzero(planted) == total, 'only %d decidable outlier joints' % np.count_nonzero(planted)
    assert not cover or np.bitwise_or.reduce(planted.ravel()) == (1 << V) - 1, 'not every view carries an outlier somewhere'
    return pts, planted


def _case(pts, P, world, thr=THR, planted=None):
    return dict(points=pts, P=P, world=world, thr=thr, planted=planted)


def _clean(rig):
    return _case(*rig)


def _outliers(rig, n_views, total, **kw):
    pts, P, world = rig
    pts, planted = plant(pts, P, n_views, total, **kw)
    return _case(pts, P, world, planted=planted)


def _dead_view():
    pts, P, world = hand_rig(2, 4, 5, 21)
    pts[:, 2, :, :2] += 300.0                      # garbage in a view whose weight says so: never scored, never used
    pts[:, 2, :, 2] = 0.0
    pts[1, 0, 3, 2] = np.nan                       # and one joint with a second dead view (weight not finite)
    return _case(pts, P, world)


def _one_valid():
    pts, P, world = hand_rig(2, 3, 5, 22)
    pts[:, 1:, :, 2] = 0.0                         # only view 0 is valid ...
    pts[1, 0, 2, 2] = -1.0                         # ... and for one joint not even that
    return _case(pts, P, world)


def _behind():
    pts, P, world = hand_rig(2, 4, 5, 23)
    P[:, 1, 2, :] = -P[:, 1, 2, :]                 # view 1 looks the other way: every point is behind it.  Its exact (u, v)
    pts = project(P, world)                        # still satisfy the DLT equations, so only the depth sign can exclude it
    pts[..., 2] = np.abs(pts[..., 2])
    return _case(pts, P, world)


def _inconsistent():
    """Pixel noise far above a 0.5-px threshold: no subset has two inliers, so the result falls back to the DLT of all views."""
    pts, P, world = hand_rig(2, 3, 5, 24)
    rng = np.random.Generator(np.random.PCG64(25))
    for b in range(2):
        for k in range(5):
            for _ in range(200):
                p = pts[b, :, k].copy()
                p[:, :2] += rng.normal(0, 40.0, (3, 2)).astype(np.float32)
                if to.decidable_one(p, P[b], 0.5):
                    pts[b, :, k] = p
                    break
            else:
                raise AssertionError('no decidable noise for joint %d.%d' % (b, k))
    return _case(pts, P, world, thr=0.5)


CASES = {
    'hm36_clean': lambda: _clean(scene_rig('hm36_best')),
    'mpi_clean': lambda: _clean(scene_rig('mpi_confident')),
    'hand_clean': lambda: _clean(hand_rig(2, 4, 5, 11)),
    'hm36_one': lambda: _outliers(scene_rig('hm36_best'), 1, 24),        # a third of the 4 x 18 joints
    'mpi_one': lambda: _outliers(scene_rig('mpi_confident'), 1, 16),
    'hand_one': lambda: _outliers(hand_rig(2, 4, 5, 12), 1, 3, cover=False),
    'mpi_two': lambda: _outliers(scene_rig('mpi_confident'), 2, 12),     # V = 5, two corrupted views: 3 of 5 still agree
    'v2': lambda: _clean(hand_rig(2, 2, 5, 13)),                         # the single subset
    'v6': lambda: _clean(hand_rig(2, 6, 5, 14)),                         # all 57 subsets
    'v6_one': lambda: _outliers(hand_rig(2, 6, 12, 15), 1, 8, scale=8.0),     # 57 subsets: a far outlier keeps their residuals off the threshold
    'k1': lambda: _clean(hand_rig(2, 4, 1, 16)),
    'b3k7': lambda: _outliers(hand_rig(3, 4, 7, 17), 1, 7, cover=False),
    'dead_view': _dead_view,
    'one_valid': _one_valid,
    'behind': _behind,
    'inconsistent': _inconsistent,
}
CLEAN = ('hm36_clean', 'mpi_clean', 'hand_clean', 'v2', 'v6', 'k1')
PLANTED = ('hm36_one', 'mpi_one', 'hand_one', 'mpi_two', 'v6_one', 'b3k7')


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, oracle result) of one case, computed once per process and shared; treat both as read-only."""
    c = CASES[name]() if name != 'eval' else eval_case()[2]
    return c, to.robust(c['points'], c['P'], c['thr'])


# --- Eval.eval_batch: the hm36 scene behind a planted detector, one corrupted camera per sample
EVAL_OFFSETS = (0.001, 0.05, -0.05)               # hypothesis 0 is the ground truth + 0.001 (an eighth of a patch pixel)
EVAL_SHIFT = (0.16, -0.12)                        # normalised patch units: about (20, -15) patch px, (70, -55) image px


@functools.lru_cache(maxsize=None)
def eval_case():
    """-> (x, {cam: (clean kps, corrupted kps)} [B,3,K,3], the triangulation inputs of the corrupted run as a case).
    Sample b's camera b % V is the corrupted one, in every joint for which the oracle finds the outcome decidable and whose
    shifted detection the left/right switch in front of the triangulation leaves in place."""
    from oracle import evalpath as ev
    cams, _, x, _ = scene('hm36_best')
    B, K, V = 4, 18, len(cams)
    g = {c: ev.normalise_gt(x['cam_%d_joints' % c]) for c in cams}
    P = torch.stack([x['cam_%d_k_mat' % c] @ torch.cat([x['cam_%d_rot_world' % c], x['cam_%d_trans_world' % c].unsqueeze(-1)], -1)
                     for c in cams], 1).numpy()
    img = lambda c, sel: ev.patch_to_image(sel, x['cam_%d_trans_image' % c], x['cam_%d_pelvis' % c]).numpy()
    pts = np.stack([img(c, g[c] + EVAL_OFFSETS[0]) for c in cams], 1)
    bad = {c: g[c].clone() for c in cams}
    hyp = lambda t: torch.stack([t + o for o in EVAL_OFFSETS], 1)
    n = 0
    for b in range(B):
        c = cams[b % V]
        shifted = g[c][b] + torch.tensor(EVAL_SHIFT + (0.0,))
        alt = ev.patch_to_image((shifted + EVAL_OFFSETS[0])[None], x['cam_%d_trans_image' % c][b:b + 1], x['cam_%d_pelvis' % c][b:b + 1]).numpy()[0]
        for k in range(K):
            p = pts[b, :, k].copy()
            p[b % V] = alt[k]
            if to.decidable_one(p, P[b], THR):
                keep = pts[b, :, k].copy()
                pts[b, :, k] = p
                bad[c][b, k] = shifted[k]
                if (ev.select_hypothesis(hyp(bad[c]), x['cam_%d_joints' % c], 'best')[0][b] == bad[c][b] + EVAL_OFFSETS[0]).all():
                    n += 1
                else:                             # the switch would trade it for its mirror joint: leave this one alone
                    pts[b, :, k] = keep
                    bad[c][b, k] = g[c][b, k]
    assert n >= B * K // 4, 'only %d corrupted joints' % n
    for i, c in enumerate(cams):                  # what the selection in front of the triangulation makes of the hypotheses
        sel = ev.select_hypothesis(hyp(bad[c]), x['cam_%d_joints' % c], 'best')[0]
        assert np.abs(img(c, sel) - pts[:, i]).max() < 1e-2, 'cam_%d: the selection did not return hypothesis 0 everywhere' % c
    return x, {c: (hyp(g[c]), hyp(bad[c])) for c in cams}, _case(pts, P, x['world'].numpy())


# ------------------------------------------------------------------------------------------------ the device side
def run(c, want=('inliers', 'resid'), thr=None):
    from xas_amd import ops_eval
    out = ops_eval.triangulate_robust(torch.from_numpy(c['points']).cuda(), torch.from_numpy(c['P']).cuda(),
                                      threshold_px=c['thr'] if thr is None else thr, want=want)
    return {k: v.cpu() for k, v in out.items()}


def dlt(c):
    from xas_amd import ops_eval
    return ops_eval.triangulate_dlt(torch.from_numpy(c['points']).cuda(), torch.from_numpy(c['P']).cuda()).cpu()


def check_vs_oracle(name):
    """What every case asserts: the oracle's mask exactly, its float64 solution of the chosen system within 2e-3 mm (the bound of
    test_gpu_eval.test_triangulation_vs_oracle_and_fp64: fp32 output rounding at |X| ~ 1e3), its mean weight and residual."""
    c, o = case(name)
    got = run(c)
    assert got['inliers'].dtype == torch.uint8 and got['inliers'].shape == o['mask'].shape
    assert np.array_equal(got['inliers'].numpy(), o['mask']), (name, got['inliers'].numpy(), o['mask'])
    xyz = got['xyzw'][..., :3].double().numpy()
    nan = np.isnan(o['xyz'])
    assert np.array_equal(np.isnan(xyz), nan)
    err = np.linalg.norm(np.where(nan, 0.0, xyz - o['xyz']), axis=-1).max()
    print('%s: |xyz - oracle| max %.3g mm, threshold margin %.3g px' % (name, err, o['thr_margin'].min()))
    assert err < 2e-3, (name, err)
    np.testing.assert_allclose(got['xyzw'][..., 3].numpy(), o['w'], rtol=1e-6, equal_nan=True)
    # residuals: double arithmetic on both sides from the same fp32 inputs; the two null vectors differ by ~1e-12 relative, the
    # fp32 result by 6e-8 relative
    np.testing.assert_allclose(got['resid'].numpy(), o['resid'], rtol=1e-5, atol=1e-4, equal_nan=True)
    return c, o, got


@pytest.mark.parametrize('name', CLEAN)
def test_no_outliers_is_the_plain_dlt(name):
    c, o, got = check_vs_oracle(name)
    V = c['points'].shape[1]
    assert (got['inliers'] == (1 << V) - 1).all()
    assert torch.equal(got['xyzw'], dlt(c))                                   # bit for bit, mean weight included
    assert float(got['resid'].max()) < 0.05
    assert np.linalg.norm(got['xyzw'][..., :3].numpy() - c['world'], axis=-1).max() < 0.5


@pytest.mark.parametrize('name', PLANTED)
def test_planted_outliers_are_left_out(name):
    c, o, got = check_vs_oracle(name)
    V = c['points'].shape[1]
    assert np.array_equal(got['inliers'].numpy(), ((1 << V) - 1) & ~c['planted'])     # exactly the corrupted views are dropped
    assert np.linalg.norm(got['xyzw'][..., :3].numpy() - c['world'], axis=-1).max() < 0.5
    hit = c['planted'] != 0
    off = np.linalg.norm(dlt(c)[..., :3].numpy() - c['world'], axis=-1)
    assert off[hit].min() > 5.0, off[hit].min()                               # the plain DLT is pulled away: the case has teeth
    assert torch.equal(got['xyzw'][torch.from_numpy(~hit)], dlt(c)[torch.from_numpy(~hit)])


def test_dead_views_are_never_used():
    c, o, got = check_vs_oracle('dead_view')
    assert ((got['inliers'] & 4) == 0).all() and got['inliers'][1, 3] == 0b1010 and got['inliers'][0, 0] == 0b1011
    w = torch.from_numpy(c['points'][..., 2])
    assert torch.allclose(got['xyzw'][0, :, 3], (w[0, 0] + w[0, 1] + w[0, 3]) / 3, rtol=1e-6)
    assert np.linalg.norm(got['xyzw'][..., :3].numpy() - c['world'], axis=-1).max() < 0.5


def test_fewer_than_two_valid_views_is_nan():
    c, o, got = check_vs_oracle('one_valid')
    assert torch.isnan(got['xyzw'][..., :3]).all() and torch.isnan(got['resid']).all() and (got['inliers'] == 0).all()
    assert got['xyzw'][0, 0, 3] == float(c['points'][0, 0, 0, 2]) and torch.isnan(got['xyzw'][1, 2, 3])


def test_a_view_behind_which_the_point_lies_is_excluded():
    c, o, got = check_vs_oracle('behind')
    assert (got['inliers'] == 0b1101).all()
    assert np.linalg.norm(got['xyzw'][..., :3].numpy() - c['world'], axis=-1).max() < 0.5


def test_no_consensus_falls_back_to_all_views():
    c, o, got = check_vs_oracle('inconsistent')
    assert (got['inliers'] == 0).all() and float(got['resid'].min()) > 1.5
    assert torch.equal(got['xyzw'], dlt(c))


def test_optional_outputs_may_be_left_out():
    c, o = case('hm36_one')
    full, bare = run(c), run(c, want=())
    assert set(bare) == {'xyzw'} and torch.equal(bare['xyzw'], full['xyzw'])
    only = run(c, want=('resid',))
    assert set(only) == {'xyzw', 'resid'} and torch.equal(only['resid'], full['resid'])


@pytest.mark.parametrize('name', ['hm36_clean', 'mpi_two', 'v6_one', 'inconsistent'])
def test_two_launches_are_bit_identical(name):
    """hm36_clean: all eleven candidates have the same inlier set and costs that differ in the last bits only - whichever wins,
    the views used are the same, and so must the result be."""
    c, _ = case(name)
    a, b = run(c), run(c)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


def test_refusals_name_the_limit():
    from xas_amd import ops_eval
    pts, P = lambda v: torch.ones(1, v, 3, 3).cuda(), lambda v: torch.ones(1, v, 3, 4).cuda()
    with pytest.raises(RuntimeError, match=r'V=1 views \(needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6\)'):
        ops_eval.triangulate_robust(pts(1), P(1))
    with pytest.raises(RuntimeError, match=r'V=7 views \(needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6\)'):
        ops_eval.triangulate_robust(pts(7), P(7))
    for bad in (0.0, -3.0, float('nan')):
        with pytest.raises(RuntimeError, match=r'needs a threshold > 0 px'):
            ops_eval.triangulate_robust(pts(3), P(3), threshold_px=bad)
    with pytest.raises(RuntimeError, match='do not match points'):
        ops_eval.triangulate_robust(pts(3), P(4))


def test_util_signatures_keep_the_reference_call():
    from modules import util as mu
    c, o = case('hm36_one')
    pts, P = torch.from_numpy(c['points']).cuda(), torch.from_numpy(c['P']).cuda()
    assert torch.equal(mu.batch_triangulate(pts, P).cpu(), dlt(c))
    assert torch.equal(mu.batch_triangulate(pts, P, robust_px=THR).cpu(), run(c)['xyzw'])


# ------------------------------------------------------------------------------------------------ Eval
def _cfg(cams):
    return {'model_params': {'cam_id_list': list(cams)}, 'dataset_params': {'dataset': {'name': 'mpi_inf_3dhp'}}}


class PlantedDetector(torch.nn.Module):
    """Returns the hypotheses planted for the image whose first pixel carries their key."""
    def forward(self, img):
        return self.kps[int(img[0, 0, 0, 0].item())], None


def _eval_setup(which):
    x, kps, _ = eval_case()
    cams = [0, 1, 2, 3]
    xd = {k: v.cuda() for k, v in x.items()}
    det = PlantedDetector()
    det.kps = {}
    for i, c in enumerate(cams):
        xd['cam_%d_img' % c] = torch.full((1, 3, 256, 256), float(i), device='cuda')
        det.kps[i] = kps[c][which].cuda()
    return cams, xd, det


def test_eval_batch_robust_recovers_the_uncorrupted_figure(tmp_path):
    import eval as xeval
    cams, xd, det = _eval_setup(0)
    clean = xeval.Eval(_cfg(cams), det, [], str(tmp_path)).eval_batch(xd, 'best')
    cams, xd, det = _eval_setup(1)
    today = xeval.Eval(_cfg(cams), det, [], str(tmp_path)).eval_batch(xd, 'best')
    plain = xeval.Eval(_cfg(cams), det, [], str(tmp_path), tri='dlt').eval_batch(xd, 'best')
    robust = xeval.Eval(_cfg(cams), det, [], str(tmp_path), tri='robust').eval_batch(xd, 'best')
    assert set(plain) == set(today) and all(torch.equal(plain[k], today[k]) for k in today)      # tensor for tensor
    assert set(robust) == set(today) | {'tri_inlier_views'}
    d = (robust['mpjpe_tri'] - clean['mpjpe_tri']).abs().cpu()
    print('mpjpe_tri clean', clean['mpjpe_tri'].cpu(), 'dlt', plain['mpjpe_tri'].cpu(), 'robust', robust['mpjpe_tri'].cpu())
    assert float(d.max()) < 1.0, d
    assert float((plain['mpjpe_tri'] - clean['mpjpe_tri']).min()) > 1.0       # the corruption does hurt the plain DLT
    n = robust['tri_inlier_views']
    assert n.dim() == 0 and n.is_cuda and len(cams) - 1 < float(n) <= len(cams)
    _, o = case('eval')
    used = np.array([[bin(m).count('1') for m in row] for row in o['used']])
    assert abs(float(n) - used.mean()) < 1e-6
    for k in today:                                                           # nothing but the triangulated pose moves
        if 'tri' not in k:
            assert torch.equal(robust[k], today[k]), k


def test_result_file_is_unchanged_with_tri_dlt(tmp_path):
    import eval as xeval
    cams, xd, det = _eval_setup(1)
    texts = {}
    for tag, kw in (('none', {}), ('dlt', dict(tri='dlt')), ('robust', dict(tri='robust'))):
        e = xeval.Eval(_cfg(cams), det, [dict(xd), dict(xd)], str(tmp_path / tag), **kw)
        lines = e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt', 'rb').read()
        assert texts[tag].decode().strip().split('\n') == lines
    assert texts['dlt'] == texts['none']
    extra = texts['robust'].decode().strip().split('\n')
    assert len(extra) == len(texts['none'].decode().strip().split('\n')) + 1
    assert extra[-1].startswith('TRI inlier views (20.0 px): 3.') and extra[-1].endswith(' of 4')
    with pytest.raises(ValueError, match='Unknown triangulation'):
        xeval.Eval(_cfg(cams), det, [], str(tmp_path), tri='ransac')
