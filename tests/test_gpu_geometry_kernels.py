"""The kernels between the detector and the loss alone, against the float64 run of the oracle on the same fp32 inputs:
patch_to_world fwd/bwd (csrc/geometry.hip) on skewed cameras and every flag combination, the one-block-per-sample reduction
of world_to_patch's backward past its 256 threads, draw_lines_max fwd/bwd at every launch edge (store tail, ragged last block,
L = 1, L = 32, many lines per joint, strides, fine bits, NaN / infinite joints) and the mask-loss kernels of csrc/losses.hip
around their block boundaries and at the clip threshold.

Bounds.  Every case runs the oracle twice on the CPU, in float64 (the reference) and in float32, and takes
max(floor, 4 x |fp32 oracle - float64|) as its bound: the floors are what the suite already asks of these ops (3e-6 forward /
value, 2e-5 patch_to_world backward, 2e-4 line gradient), the factor 4 allows for another but equally valid operation order
(closed-form inverses, fused exponent, block sums).  Nothing in a bound comes from the kernel.  Errors are relative to the
largest reference entry of the case, except the masks (absolute, values in [0, 1]).  Every test prints its figures.

Measured on an MI355X, worst over the shapes / sizes of each case (`kernel` and `fp32 oracle` are distances from float64):

  case                                            kernel     fp32 oracle   bound (smallest .. largest over the shapes)
  patch_to_world fwd  norm patch  world           1.65e-07   1.58e-07      3.00e-06
  patch_to_world bwd  norm patch  world           1.76e-07   2.81e-07      2.00e-05
  patch_to_world fwd  px   patch  world           1.16e-07   1.38e-07      3.00e-06
  patch_to_world bwd  px   patch  world           1.65e-07   2.15e-07      2.00e-05
  patch_to_world fwd  no patch    world           9.53e-08   1.09e-07      3.00e-06
  patch_to_world bwd  no patch    world           1.25e-07   1.04e-07      2.00e-05
  patch_to_world fwd  norm patch  mono            4.75e-08   4.78e-08      3.00e-06
  patch_to_world bwd  norm patch  mono            7.65e-08   7.65e-08      2.00e-05
  patch_to_world fwd  px   patch  mono            4.88e-08   4.83e-08      3.00e-06
  patch_to_world bwd  px   patch  mono            7.86e-08   8.59e-08      2.00e-05
  patch_to_world fwd  no patch    mono            3.54e-08   3.54e-08      3.00e-06
  patch_to_world bwd  no patch    mono            0          0             2.00e-05
  patch_to_image      norm / px                   4.14e-08   4.88e-08      3.00e-06
  world_to_patch bwd  grad_points                 1.63e-07   1.63e-07      2.00e-05
  world_to_patch bwd  grad_pre_rot                1.17e-07   4.82e-07      2.00e-05
  draw_lines mask     one                         9.04e-07   9.10e-07      3.00e-06 .. 3.64e-06
  draw_lines mask     h36m17                      1.51e-06   1.67e-06      3.00e-06 .. 6.69e-06
  draw_lines mask     h36m25                      1.56e-06   1.97e-06      3.00e-06 .. 7.89e-06
  draw_lines mask     chain32                     1.45e-06   1.76e-06      3.00e-06 .. 7.03e-06
  draw_lines mask     chain32_k64                 1.66e-06   1.87e-06      3.00e-06 .. 7.48e-06
  draw_lines mask     star8                       1.27e-06   1.27e-06      3.00e-06 .. 5.07e-06
  draw_lines mask     strided / fine bits / stack 1.48e-06   1.84e-06      3.00e-06 .. 7.35e-06
  draw_lines mask     clean sample beside a NaN   1.56e-06   1.56e-06      3.00e-06 .. 6.24e-06
  draw_lines grad     one                         1.36e-06   1.97e-06      2.00e-04
  draw_lines grad     h36m17                      1.09e-06   1.12e-06      2.00e-04
  draw_lines grad     h36m25                      2.88e-06   2.97e-06      2.00e-04
  draw_lines grad     chain32                     3.57e-06   3.53e-06      2.00e-04
  draw_lines grad     chain32_k64                 2.83e-06   2.81e-06      2.00e-04
  draw_lines grad     star8                       4.23e-06   4.10e-06      2.00e-04
  mask_loss value     four modes, n < 2^20 + 1    1.02e-07   (floor only)  3.00e-06
  mask_loss grad      four modes, n < 2^20 + 1    1.26e-07   (floor only)  3.00e-06
  mask_loss value     four modes, n = 2^20 + 1    8.35e-08   8.01e-08      3.00e-06
  mask_loss grad      four modes, n = 2^20 + 1    8.89e-08   1.30e-07      3.00e-06

The fast exponential of the forward stays at the fp32 oracle's own distance at every S: no finding there.

Line-mask backward: pixels whose float64 winner is not safe to call (mask > 1e-6 and 0 < gap < 1e-3 max(1, |best|) between
the best and the second exponent) get grad_mask = 0 on both sides; exact ties stay in.  Their share of the live pixels is
asserted <= 2 % per case.  Shares (S = 2, 3, 5 leave nothing out at any link set; `one` nothing at any S):

  link set       S = 31    32        33        64
  h36m17         0.68 %    0.82 %    0.43 %    0.51 %
  h36m25         0.74 %    0.87 %    0.73 %    0.55 %
  chain32        0.51 %    0.79 %    1.04 %    0.87 %
  chain32_k64    0.80 %    0.75 %    0.56 %    1.10 %
  star8          0         0.12 %    0.11 %    0.03 %

Non-finite joints: the eight cases of test_draw_lines_non_finite_joint fail on the kernels before the shared winner rule (the
mask of the poisoned sample came out finite, and exactly 0 with one line) and pass with it; the masks and gradients of the
existing goldens are bit-identical before and after.
"""
import functools

import numpy as np
import pytest
import torch

import inputs as gi

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')
FWD_FLOOR, BWD_FLOOR, LINE_GRAD_FLOOR = 3e-6, 2e-5, 2e-4
MODE = 'cam_0'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def relmax(a, ref):
    """max |a - ref| relative to the largest reference entry"""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def absmax(a, ref):
    return float((a.detach().cpu().double() - ref.detach().cpu().double()).abs().max())


def check(what, err, oracle_err, floor):
    """bound = max(floor, 4 x the fp32 oracle's own distance from float64)"""
    bound = max(floor, 4 * oracle_err)
    print('%s: kernel %.3g, fp32 oracle %.3g, bound %.3g' % (what, err, oracle_err, bound))
    assert err <= bound, '%s: error %.3g above the bound %.3g (fp32 oracle %.3g)' % (what, err, bound, oracle_err)


def leaf(t, dt=None, device=None):
    """a fresh autograd leaf (never the caller's tensor itself: the cached inputs stay as they are)"""
    return t.detach().to(device=device, dtype=dt or t.dtype).clone().requires_grad_(True)


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device='cuda')


# ------------------------------------------------------------------------------------------------------------ patch_to_world
def skew_cameras(B, seed):
    """Cameras for which no inverse is a transpose: crop affine diag(sx, sy) . shear . rotation with sx != sy in [0.2, 0.4]
    and a negative determinant for every second sample, fx != fy, rot_world = rotation . diag(0.8, 1, 1.3) + off-diagonal shear;
    pelvis and translations at the magnitudes of inputs.camera_params.  fp32 arrays in the order of the entry points."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ti, km, rot = np.zeros((B, 2, 3)), np.zeros((B, 3, 3)), np.zeros((B, 3, 3))
    for b in range(B):
        sx, sy = rng.uniform(0.2, 0.28), rng.uniform(0.32, 0.4)
        if rng.uniform() < 0.5:
            sx, sy = sy, sx
        if b % 2:
            sx = -sx                                                   # a flipped crop
        th, k = rng.uniform(-0.6, 0.6), rng.uniform(0.1, 0.3) * (1 if rng.uniform() < 0.5 else -1)
        rot2 = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        ti[b, :, :2] = np.diag([sx, sy]) @ np.array([[1.0, k], [0.0, 1.0]]) @ rot2
        ti[b, :, 2] = rng.uniform(-40, 40, 2)
        km[b] = np.diag([rng.uniform(1100, 1140), rng.uniform(1160, 1200), 1.0])
        km[b, 0, 2], km[b, 1, 2] = rng.uniform(480, 540, 2)
        shear = 0.05 * rng.standard_normal((3, 3))
        np.fill_diagonal(shear, 0.0)
        rot[b] = gi.random_rotation(rng) @ np.diag([0.8, 1.0, 1.3]) + shear
    pelvis = np.stack([rng.uniform(-500, 500, B), rng.uniform(-500, 500, B), rng.uniform(4000, 6000, B)], 1)
    tw = rng.uniform(-3000, 3000, (B, 3))
    return tuple(T(a.astype(np.float32)) for a in (ti, km, pelvis, rot, tw))


def test_skew_cameras_are_skewed():
    """the generator does what the cases below rely on (no GPU work; kept here with the generator)"""
    ti, km, pv, rw, tw = [a.double() for a in skew_cameras(6, 3)]
    A = ti[:, :, :2]
    det = torch.linalg.det(A)
    assert (det[0::2] > 0).all() and (det[1::2] < 0).all()
    for M in (A, rw):                                                  # inverse far from any multiple of the transpose
        inv, tr = torch.linalg.inv(M), M.transpose(1, 2)
        scale = (inv * tr).sum((1, 2), keepdim=True) / (tr * tr).sum((1, 2), keepdim=True)
        assert (((inv - scale * tr).norm(dim=(1, 2)) / inv.norm(dim=(1, 2))) > 0.1).all()
    assert ((km[:, 0, 0] - km[:, 1, 1]).abs() > 10).all()


P2W_SHAPES = [(1, 1, 1), (1, 1, 128), (1, 1, 129), (3, 2, 43), (5, 3, 18)]
P2W_FLAGS = [(n, p, m) for n in (True, False) for p in (True, False) for m in (True, False)]
S_IMG, RECT = 256, 2000.0


def _p2w_points(B, Hy, K, is_norm, patch):
    """Points at the magnitudes the stage they enter expects: normalised patch coordinates, patch pixels, or - without the
    patch stage - image pixels and a depth in mm."""
    rng = np.random.Generator(np.random.PCG64(1000 * B + 10 * Hy + K))
    p = rng.uniform(-0.9, 0.9, (B, Hy, K, 3))
    if not patch:
        p = np.stack([500 + 500 * p[..., 0], 500 + 500 * p[..., 1], 5000 + 2000 * p[..., 2]], -1)
    elif not is_norm:
        p = np.stack([(p[..., 0] + 1) / 2 * (S_IMG - 1), (p[..., 1] + 1) / 2 * (S_IMG - 1), p[..., 2] * (S_IMG - 1)], -1)
    return T(p.astype(np.float32)), T(rng.standard_normal((B, Hy, K, 3)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _p2w_reference(B, Hy, K, is_norm, patch, mono, dt):
    """-> points, grad_world (fp32) and the oracle's world points and d/d points in `dt`"""
    from oracle import geometry as geo
    kps, gw = _p2w_points(B, Hy, K, is_norm, patch)
    cam = [a.to(dt) for a in skew_cameras(B, 7 + B)]
    x = leaf(kps.reshape(B, Hy * K, 3), dt)
    w = geo.patch_to_world(x, *cam, image_size=S_IMG, rect_width=RECT, is_norm=is_norm, mono=mono, patch=patch)
    (g,) = torch.autograd.grad(w, x, gw.to(dt).reshape(B, Hy * K, 3))
    return kps, gw, w.detach().reshape(B, Hy, K, 3), g.reshape(B, Hy, K, 3)


def _p2w_hip(kps, gw, cam, is_norm, patch, mono):
    from xas_amd import ops_head
    x = leaf(kps, device='cuda')
    w = ops_head.patch_to_world(x, *cam, image_size=S_IMG, rect_width=RECT, is_norm=is_norm, mono=mono, patch=patch)
    w.backward(gw.cuda())
    return w.detach(), x.grad


@pytest.mark.parametrize('is_norm,patch,mono', P2W_FLAGS, ids=lambda v: 'TF'[not v])
@pytest.mark.parametrize('B,Hy,K', P2W_SHAPES)
def test_patch_to_world(B, Hy, K, is_norm, patch, mono):
    """(1,1,128) / (1,1,129): either side of the 128-thread block; (3,2,43): blocks straddle samples, b = i / HK changes inside
    a block; every flag combination the Python entry can form, forward and backward with a random grad_world."""
    kps, gw, ref, gref = _p2w_reference(B, Hy, K, is_norm, patch, mono, torch.float64)
    _, _, o32, g32 = _p2w_reference(B, Hy, K, is_norm, patch, mono, torch.float32)
    cam = [a.cuda() for a in skew_cameras(B, 7 + B)]
    w, g = _p2w_hip(kps, gw, cam, is_norm, patch, mono)
    assert w.shape == g.shape == (B, Hy, K, 3)
    tag = 'patch_to_world (%d,%d,%d) norm=%d patch=%d mono=%d' % (B, Hy, K, is_norm, patch, mono)
    check(tag + ' fwd', relmax(w, ref), relmax(o32, ref), FWD_FLOOR)
    check(tag + ' bwd', relmax(g, gref), relmax(g32, gref), BWD_FLOOR)


@pytest.mark.parametrize('is_norm', [True, False], ids=['norm', 'px'])
@pytest.mark.parametrize('B,Hy,K', P2W_SHAPES)
def test_patch_to_image(B, Hy, K, is_norm):
    """XAS_GEO_IMAGE (forward only) through ops_eval.patch_to_image against the oracle's patch stage"""
    from oracle import evalpath
    from xas_amd import ops_eval
    kps, _ = _p2w_points(B, Hy, K, is_norm, True)
    kps = kps.reshape(B, Hy * K, 3)
    ti, _, pv, _, _ = skew_cameras(B, 7 + B)
    ref = evalpath.patch_to_image(kps.double(), ti.double(), pv.double(), float(S_IMG), RECT, is_norm)
    o32 = evalpath.patch_to_image(kps, ti, pv, float(S_IMG), RECT, is_norm)
    out = ops_eval.patch_to_image(kps.cuda(), ti.cuda(), pv.cuda(), float(S_IMG), RECT, is_norm)
    check('patch_to_image (%d,%d,%d) norm=%d' % (B, Hy, K, is_norm), relmax(out, ref), relmax(o32, ref), FWD_FLOOR)


@pytest.mark.parametrize('B,Hy,K', [(3, 2, 43), (5, 3, 18)])
def test_patch_to_world_hypotheses_at_once_equal_separate_calls(B, Hy, K):
    for is_norm, patch, mono in ((True, True, False), (False, True, True), (True, False, False)):
        kps, gw = _p2w_points(B, Hy, K, is_norm, patch)
        cam = [a.cuda() for a in skew_cameras(B, 7 + B)]
        w, g = _p2w_hip(kps, gw, cam, is_norm, patch, mono)
        for h in range(Hy):
            wh, gh = _p2w_hip(kps[:, h].contiguous(), gw[:, h].contiguous(), cam, is_norm, patch, mono)
            assert torch.equal(w[:, h], wh) and torch.equal(g[:, h], gh)


# ------------------------------------------------------------------------------- world_to_patch backward: the block reduction
def _w2p_inputs(HK):
    rng = np.random.Generator(np.random.PCG64(500 + HK))
    Hy = 3 if HK % 3 == 0 else 1
    pts = (0.3 * rng.standard_normal((2, Hy, HK // Hy, 3))).astype(np.float32)          # metres about the pelvis
    rot = np.stack([gi.random_rotation(rng) + 0.05 * rng.standard_normal((3, 3)) for _ in range(2)]).astype(np.float32)
    return T(pts), T(rot), T(rng.standard_normal(pts.shape).astype(np.float32))


def _cam_dict(cam, device, dt):
    names = ('trans_image', 'k_mat', 'pelvis', 'rot_world', 'trans_world')
    out = {'%s_%s' % (MODE, k): v.to(device=device, dtype=dt) for k, v in zip(names, cam)}
    out[MODE + '_img'] = torch.zeros(1, 3, S_IMG, S_IMG)                # only .shape is read
    return out


def _w2p_oracle(HK, dt):
    from test_gpu_reproject import f64_project
    pts, rot, gw = _w2p_inputs(HK)
    x = {k: v for k, v in _cam_dict(skew_cameras(2, 21), 'cpu', dt).items() if not k.endswith('_img')}
    p, r = leaf(pts, dt), leaf(rot, dt)
    out = f64_project(p, x, is_norm=False, pre_rot=r, pre_scale=1000.0, pelvis_origin=True, size=S_IMG, rect=RECT)
    return torch.autograd.grad(out, (p, r), gw.to(dt))


def _w2p_hip(HK):
    from xas_amd import ops_head
    pts, rot, gw = _w2p_inputs(HK)
    p, r = leaf(pts, device='cuda'), leaf(rot, device='cuda')
    out = ops_head.world_to_patch(p, _cam_dict(skew_cameras(2, 21), 'cuda', torch.float32), MODE, is_norm=False, pre_rot=r,
                                  pre_scale=1000.0, pelvis_origin=True)
    out.backward(gw.cuda())
    return p.grad, r.grad


@pytest.mark.parametrize('HK', [1, 255, 256, 257, 600])
def test_world_to_patch_backward_reduction(HK):
    """More points per sample than the 256 threads of the one-block-per-sample backward (257, 600: the strided loop), exactly
    as many, one fewer, and a single point; rotated + shifted path, skewed camera."""
    gp, gr = _w2p_hip(HK)
    ref_p, ref_r = _w2p_oracle(HK, torch.float64)
    o_p, o_r = _w2p_oracle(HK, torch.float32)
    check('world_to_patch bwd HK=%d grad_points' % HK, relmax(gp, ref_p), relmax(o_p, ref_p), BWD_FLOOR)
    check('world_to_patch bwd HK=%d grad_pre_rot' % HK, relmax(gr, ref_r), relmax(o_r, ref_r), BWD_FLOOR)
    gp2, gr2 = _w2p_hip(HK)
    assert torch.equal(gp, gp2) and torch.equal(gr, gr2)


# ------------------------------------------------------------------------------------------------------------ draw_lines_max
LINE_S = [2, 3, 5, 31, 32, 33, 64]
WIDTH = {2: 2.0, 3: 0.5, 5: 0.12}       # S -> body_width that keeps pixels of the coarse grids alive; else the workload's
WORK_WIDTH = 3.0e-3
# link set -> seed of inputs.skeleton_2d, chosen on the CPU so that the float64 reference alone meets the 2 % cap at every S
SEEDS = {'one': 5, 'h36m17': 10, 'h36m25': 31, 'chain32': 25, 'chain32_k64': 14, 'star8': 5}


@functools.lru_cache(maxsize=None)
def link_sets():
    """name -> (K, parents, children)"""
    from oracle import geometry as geo
    p17, c17 = geo.skeleton_links(gi.HM36_PARENTS, gi.LINE_SELECT, False, False)
    p25, c25 = geo.skeleton_links(gi.HM36_PARENTS, gi.LINE_SELECT, False, True)
    return {'one': (2, (0,), (1,)),
            'h36m17': (18, tuple(p17), tuple(c17)),
            'h36m25': (18, tuple(p25), tuple(c25)),                                      # >= 21 lines: the fine lines
            'chain32': (33, tuple(range(32)), tuple(range(1, 33))),                      # L = kMaxLines
            'chain32_k64': (64, tuple(range(31, 63)), tuple(range(32, 64))),             # up to the last joint; 0..30 unused
            'star8': (9, (0,) * 8, tuple(range(1, 9)))}                                  # eight lines into one joint


def _width(S):
    return WIDTH.get(S, WORK_WIDTH)


def _line_kps(name, B=2):
    return T(gi.skeleton_2d(B, seed=SEEDS[name], K=link_sets()[name][0]))


def _heat(kp, S, name, dt, width=None):
    """per-line heat-maps of the oracle [B,L,S,S] in dt"""
    from oracle import geometry as geo
    _, p, c = link_sets()[name]
    return geo.line_heatmaps(kp.to(dt), S, list(p), list(c), _width(S) if width is None else width)


def _unsafe_pixels(heat64):
    """[B,L,S,S] float64 -> (live, unsafe) [B,1,S,S]: pixels with mask > 1e-6, and those of them whose winner fp32 and float64
    may call differently: 0 < gap < 1e-3 max(1, |best|) between the best and the second exponent.  Exact ties stay in."""
    e = heat64.log()
    top = e.topk(min(2, e.shape[1]), dim=1).values
    best = top[:, :1]
    live = best.exp() > 1e-6
    if e.shape[1] == 1:
        return live, torch.zeros_like(live)
    gap = best - top[:, 1:2]
    return live, live & (gap > 0) & (gap < 1e-3 * best.abs().clamp_min(1.0))


@functools.lru_cache(maxsize=None)
def _lines_reference(name, S):
    """Inputs and the float64 / float32 oracle: masks, the masked grad_mask, d/d joints.  Computed once, never modified."""
    kp = _line_kps(name)
    heat = _heat(kp, S, name, torch.float64)
    live, unsafe = _unsafe_pixels(heat)
    share = float(unsafe.sum()) / max(1, int(live.sum()))
    gm = torch.rand(2, 1, S, S, generator=torch.Generator().manual_seed(S)) + 0.1
    gm = torch.where(unsafe, torch.zeros_like(gm), gm)
    out = {'kp': kp, 'gm': gm, 'share': share, 'live': int(live.sum())}
    for dt in (torch.float64, torch.float32):
        k = leaf(kp, dt)
        m = _heat(k, S, name, dt).max(dim=1, keepdim=True)[0]
        (g,) = torch.autograd.grad(m, k, gm.to(dt))
        out[dt] = (m.detach(), g)
    return out


def _lines_hip(kp, S, name, gm, width=None):
    from xas_amd import ops_head
    _, p, c = link_sets()[name]
    k = leaf(kp, device='cuda')
    m = ops_head.draw_lines_max(k, S, list(p), list(c), _width(S) if width is None else width)
    m.backward(gm.cuda())
    return m.detach().cpu(), k.grad.cpu()


@pytest.mark.parametrize('name', list(SEEDS))
@pytest.mark.parametrize('S', LINE_S)
def test_draw_lines_max(S, name):
    """S = 2: one float4, one working thread; 3, 5, 31, 33: S*S odd, every store through the tail loop and a ragged last block;
    32: exactly one block; 33: a second block with 65 pixels; 64: four blocks, the cross-block sums of the backward."""
    r = _lines_reference(name, S)
    print('draw_lines %s S=%d: %d live pixels, share left out of the backward %.4f' % (name, S, r['live'], r['share']))
    assert r['share'] <= 0.02
    (ref, gref), (o32, g32) = r[torch.float64], r[torch.float32]
    m, g = _lines_hip(r['kp'], S, name, r['gm'])
    assert m.shape == (2, 1, S, S) and g.shape == r['kp'].shape
    check('draw_lines %s S=%d mask' % (name, S), absmax(m, ref), absmax(o32, ref), FWD_FLOOR)
    check('draw_lines %s S=%d grad' % (name, S), relmax(g, gref), relmax(g32, gref), LINE_GRAD_FLOOR)
    used = set(link_sets()[name][1]) | set(link_sets()[name][2])
    for j in range(r['kp'].shape[1]):
        if j not in used:
            assert (g[:, j] == 0).all()


def test_draw_lines_stack_of_the_public_wrapper():
    """modules.util.draw_lines: one launch per line (L = 1), fine lines by a halved width, against line_heatmaps"""
    from modules.util import draw_lines
    S, name = 33, 'h36m25'
    _, p, c = link_sets()[name]
    kp = _line_kps(name)
    ref, o32 = _heat(kp, S, name, torch.float64), _heat(kp, S, name, torch.float32)
    out = draw_lines(kp.cuda(), S, list(p), list(c), WORK_WIDTH)
    assert out.shape == (2, 25, S, S)
    check('draw_lines stack S=33', absmax(out, ref), absmax(o32, ref), FWD_FLOOR)


def _raw_lines(kps_ptr, sb, sj, B, K, p, c, fine, width, S, gm):
    """xas_draw_lines_max_fwd/_bwd on a raw pointer; every output filled with NaN first, the mask with eight floats of slack
    behind it that must stay untouched"""
    from xas_amd._lib import call, query
    par = torch.tensor(list(p), dtype=torch.int32, device='cuda')
    chi = torch.tensor(list(c), dtype=torch.int32, device='cuda')
    L = len(p)
    buf = nans(B * S * S + 8)
    call('xas_draw_lines_max_fwd', kps_ptr, sb, sj, B, K, par.data_ptr(), chi.data_ptr(), L, fine, float(width), S, buf.data_ptr())
    assert torch.isnan(buf[B * S * S:]).all(), 'the forward wrote past its mask'
    nblk = query('xas_lines_nblk', S)
    partial, g = nans(B * nblk * K * 2), nans(B, K, 2)
    call('xas_draw_lines_max_bwd', kps_ptr, sb, sj, B, K, par.data_ptr(), chi.data_ptr(), L, fine, float(width), S,
         gm.data_ptr(), partial.data_ptr(), g.data_ptr())
    torch.cuda.synchronize()
    return buf[:B * S * S].view(B, 1, S, S).clone(), g


@pytest.mark.parametrize('S', LINE_S)
def test_draw_lines_strides(S):
    """The (x, y) columns of hypothesis 1 of a [B,Hy,K,3] tensor, read in place through kp_stride_b / kp_stride_j, give the
    bits of the contiguous call; nothing is written behind the mask at any S."""
    B, Hy, name = 2, 3, 'h36m25'
    K, p, c = link_sets()[name]
    fine = sum(1 << l for l in (11, 12, 14, 15))
    full = (torch.rand(B, Hy, K, 3, generator=torch.Generator().manual_seed(S)) * 1.6 - 0.8).cuda()
    gm = torch.rand(B, 1, S, S, generator=torch.Generator().manual_seed(S + 1)).cuda()
    view = full[:, 1, :, :2]
    assert view.data_ptr() == full.data_ptr() + 4 * K * 3 and not view.is_contiguous()
    m1, g1 = _raw_lines(view.data_ptr(), Hy * K * 3, 3, B, K, p, c, fine, _width(S), S, gm)
    flat = view.contiguous()
    m2, g2 = _raw_lines(flat.data_ptr(), K * 2, 2, B, K, p, c, fine, _width(S), S, gm)
    assert torch.equal(m1, m2) and torch.equal(g1, g2)
    assert torch.isfinite(m1).all() and torch.isfinite(g1).all()
    ref = _heat(flat.cpu(), S, name, torch.float64).max(dim=1, keepdim=True)[0]
    o32 = _heat(flat.cpu(), S, name, torch.float32).max(dim=1, keepdim=True)[0]
    check('draw_lines strided S=%d mask' % S, absmax(m1, ref), absmax(o32, ref), FWD_FLOOR)


@pytest.mark.parametrize('bits', [(0, 7, 31), tuple(range(32)), ()], ids=['0-7-31', 'all', 'none'])
def test_draw_lines_fine_mask_bits(bits):
    """fine_mask patterns the Python entry never forms, on L = 32 (bit 31 included): exponent x2 is the heat-map squared.  The
    oracle switches its fixed pattern on from 21 lines, so the per-line maps come from two calls of 16 lines."""
    from oracle import geometry as geo
    S, name = 33, 'chain32'
    K, p, c = link_sets()[name]
    kp = _line_kps(name)
    scale = torch.ones(32, dtype=torch.float64)
    scale[list(bits)] = 2.0

    def masks(dt):
        heat = torch.cat([geo.line_heatmaps(kp.to(dt), S, list(p[h:h + 16]), list(c[h:h + 16]), WORK_WIDTH) for h in (0, 16)], 1)
        return heat.pow(scale.to(dt).view(1, -1, 1, 1)).max(dim=1, keepdim=True)[0]
    gm, kg = torch.zeros(2, 1, S, S, device='cuda'), kp.cuda()
    m, _ = _raw_lines(kg.data_ptr(), K * 2, 2, 2, K, p, c, sum(1 << l for l in bits), WORK_WIDTH, S, gm)
    ref = masks(torch.float64)
    check('draw_lines fine bits %s' % (bits,), absmax(m, ref), absmax(masks(torch.float32), ref), FWD_FLOOR)


@pytest.mark.parametrize('bad', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('name,joint', [('one', 0), ('h36m25', 7)])
@pytest.mark.parametrize('S', [33, 64])
def test_draw_lines_non_finite_joint(S, name, joint, bad):
    """One NaN / +inf coordinate in sample 0: its whole mask is NaN, as exp and torch.max give (so that the guarded optimizer
    step sees it), and its gradient is non-finite at least at the joints where autograd's is; sample 1 does not notice."""
    r = _lines_reference(name, S)
    kp = r['kp'].clone()
    kp[0, joint, 1] = bad
    k64 = leaf(kp, torch.float64)
    ref = _heat(k64, S, name, torch.float64).max(dim=1, keepdim=True)[0]
    (gref,) = torch.autograd.grad(ref, k64, r['gm'].double())
    ref = ref.detach()
    assert torch.isnan(ref[0]).all() and not torch.isnan(ref[1]).any()          # what the oracle does
    m, g = _lines_hip(kp, S, name, r['gm'])
    assert torch.equal(torch.isnan(m), torch.isnan(ref))
    o32 = r[torch.float32][0]
    check('draw_lines %s S=%d %s: mask of the clean sample' % (name, S, bad), absmax(m[1], ref[1]), absmax(o32[1], ref[1]), FWD_FLOOR)
    bad_ref = ~torch.isfinite(gref[0]).all(dim=-1)
    assert bad_ref[joint]
    bad_hip = ~torch.isfinite(g[0]).all(dim=-1)
    assert (bad_hip | ~bad_ref).all(), 'finite gradient at joints %s' % (bad_ref & ~bad_hip).nonzero().flatten().tolist()
    m_clean, g_clean = _lines_hip(r['kp'], S, name, r['gm'])
    assert torch.equal(m[1], m_clean[1]) and torch.equal(g[1], g_clean[1])
    assert torch.isfinite(g[1]).all()


# ----------------------------------------------------------------------------------------------------------------- mask loss
LOSS_N = [1, 255, 256, 257, 4095, 4096, 4097, 4096 * 256 + 1]
LOSS_MODES = [(False, False), (True, False), (False, True), (True, True)]             # (weighted, clip)
# The clip is `mask > 0.1` on float32 data, so the threshold is float32(0.1) = 0.100000001490116..., not the double 0.1: a
# mask value of exactly float32(0.1) is above the double 0.1 and NOT above the threshold of the fp32 reference program.  The
# float64 run of the oracle is therefore given the float32 value, or it would itself disagree with that program there.
CLIP_AT = float(np.float32(0.1))


@functools.lru_cache(maxsize=None)
def _loss_inputs(n):
    """mask in [0, 1] with the threshold itself and its two fp32 neighbours planted, gt, weight"""
    gen = torch.Generator().manual_seed(n)
    m = torch.rand(n, generator=gen)
    t = np.float32(0.1)
    edge = torch.tensor([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))], dtype=torch.float32)
    at = (torch.arange(12) * 7919 + n // 2) % n                                          # spread over blocks and lanes
    m[at] = edge.repeat(4)
    assert n < 3 or all(bool((m == v).any()) for v in edge)
    return m, (torch.rand(n, generator=gen) > 0.5).float(), 0.5 + 1.5 * torch.rand(n, generator=gen)


def _loss_oracle(m, gt, w, weighted, clip, dt):
    from oracle import losses
    x = leaf(m, dt)
    v = losses.mask_recon(x, gt.to(dt), w.to(dt) if weighted else None, clip, clip_at=CLIP_AT).mean()
    (g,) = torch.autograd.grad(v, x)
    return v.detach(), g


def _loss_hip(m, gt, w, weighted, clip, shape=None):
    from xas_amd import ops_misc
    shape = shape or (m.numel(),)
    x = leaf(m.reshape(shape), device='cuda')
    v = ops_misc.mask_loss(x, gt.cuda().reshape(shape), w.cuda().reshape(shape) if weighted else None, clip)
    v.backward()
    return v.detach().cpu(), x.grad.cpu().reshape(-1)


@pytest.mark.parametrize('weighted,clip', LOSS_MODES, ids=['plain', 'weighted', 'clip', 'weighted+clip'])
@pytest.mark.parametrize('n', LOSS_N)
def test_mask_loss(n, weighted, clip):
    """n below one block of 4096, around 256 (one element per thread) and 4096, and 257 partial blocks for the 256 threads of
    the finalize kernel; value and d/dmask.  Only the largest n takes its bound from the fp32 oracle; the others keep 3e-6."""
    m, gt, w = _loss_inputs(n)
    ref, gref = _loss_oracle(m, gt, w, weighted, clip, torch.float64)
    o32, g32 = _loss_oracle(m, gt, w, weighted, clip, torch.float32)
    big = n == max(LOSS_N)
    v, g = _loss_hip(m, gt, w, weighted, clip, (1, 1, 1, n) if n % 2 else None)
    tag = 'mask_loss n=%d weighted=%d clip=%d' % (n, weighted, clip)
    check(tag + ' value', relmax(v, ref), relmax(o32, ref) if big else 0.0, FWD_FLOOR)
    check(tag + ' grad', relmax(g, gref), relmax(g32, gref) if big else 0.0, FWD_FLOOR)
    if clip and weighted:                                # the planted values: at and below the threshold clipped, above not
        t = np.float32(0.1)
        assert (g[m <= float(t)] == 0).all() and (g[m == float(np.nextafter(t, np.float32(1)))] != 0).all()


@pytest.mark.parametrize('weighted', [False, True], ids=['clip', 'weighted+clip'])
@pytest.mark.parametrize('n', [257, 4097])
def test_mask_loss_all_clipped_is_exactly_zero(n, weighted):
    m, gt, w = _loss_inputs(n)
    m = (m * CLIP_AT).clamp(max=CLIP_AT)
    m[n // 3] = CLIP_AT
    assert (m <= CLIP_AT).all() and (m == CLIP_AT).any()
    v, g = _loss_hip(m, gt, w, weighted, True)
    assert float(v) == 0.0 and (g == 0).all()
    assert float(_loss_oracle(m, gt, w, weighted, True, torch.float64)[0]) == 0.0


@pytest.mark.parametrize('weighted,clip', LOSS_MODES, ids=['plain', 'weighted', 'clip', 'weighted+clip'])
@pytest.mark.parametrize('n', [257, 4097])
def test_mask_loss_nan_reaches_the_value(n, weighted, clip):
    m, gt, w = _loss_inputs(n)
    m = m.clone()
    m[n - 2] = NAN
    assert torch.isnan(_loss_oracle(m, gt, w, weighted, clip, torch.float64)[0])
    v, _ = _loss_hip(m, gt, w, weighted, clip)
    assert torch.isnan(v)
