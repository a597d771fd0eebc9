"""World -> patch projection (xas_world_to_patch_fwd/bwd, ops_head.world_to_patch) and the SMPL side of modules.util
(project_smpl_to_patch_kps, convert_pelvis_to_world, flip_3D) on the GPU, against the reference-generated golden
`reproject.npz` (tests/golden/make_golden_reproject.py) and against float64 autograd through the restatement below.

Tolerances.  The generator runs the reference's own float32 functions and this file's float64 restatement on the same
inputs and stores, per output group, the reference's maximum absolute deviation from float64 (`dev_*`).  The bar of the
HIP result against float64 is 4 x that deviation (the factor covers the other operation order of a fused closed-form
inverse against LU); against the float32 golden it is that bar plus the golden's own deviation, 5 x in all.  Measured
deviations of the reference (float32 on the CPU) and the resulting bars against float64:

    group                                   reference dev   bar (4 x)
    norm        normalised patch coords       5.00e-07       2.00e-06
    px          patch pixels                  1.30e-04       5.20e-04
    image_uv    image pixels                  9.55e-05       3.82e-04
    image_z     camera depth, mm              8.52e-04       3.41e-03
    rot_px      rotated + shifted, patch px   1.45e-04       5.79e-04
    pelvis_w    pelvis in world, mm           3.32e-04       1.33e-03
    smpl_kps    SMPL joints, patch px         1.50e-04       6.00e-04
    smpl300_kps the same at V = 300           1.65e-04       6.59e-04
    smpl_verts  SMPL vertices, world mm       1.38e-03       5.53e-03
    rt_patch    patch->world->patch, norm     5.36e-07       2.15e-06   (reference's own float32 round trip)
    rt_world    world->patch->world, mm       9.77e-04       3.91e-03   (reference's own float32 round trip)
    g_pts_norm  d/d points, normalised        1.75e-10       7.01e-10
    g_pts_image d/d points, world -> image    2.76e-07       1.10e-06
    g_pts_rot   d/d points, rotated path      5.99e-05       2.39e-04
    g_rot_*     d/d pre_rot, per point count  0.98 .. 2.21e-04   3.93 .. 8.85e-04
    g_smpl_rot / _pose / _shape (V = 300)     1.47e-05 / 1.07e-05 / 1.11e-06   5.90e-05 / 4.27e-05 / 4.43e-06

The float64 restatement is this file's own statement of the pin-hole / crop-affine algebra and of SMPL linear blend skinning
(public formulation: shape blend, joint regression, pose blend, kinematic chain, skinning); it imports nothing but torch.
"""
import functools
import os

import numpy as np
import pytest
import torch

import inputs as gi
from conftest import golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
MODE = 'cam_0'
S, RECT = 256, 2000.0
CAM_SEED, SMPL_CAM_SEED, SMPL_BUF_SEED, SMPL_SMALL_V = 131, 137, 171, 300
# slices (batch, hypothesis, joint) of the [4,3,18,3] fixture: every point count the per-sample reduction of grad_pre_rot
# meets - 54 and 17 (no multiple of 64), 51, 18, and a batch of one
CASES = {'full': (slice(0, 4), slice(0, 3), slice(0, 18)), 'k17': (slice(0, 4), slice(0, 3), slice(0, 17)),
         'h1k17': (slice(0, 4), slice(1, 2), slice(0, 17)), 'b1': (slice(2, 3), slice(0, 3), slice(0, 18)),
         'h1': (slice(0, 4), slice(0, 1), slice(0, 18))}
SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)


# ------------------------------------------------------------------ inputs (seeds only; shared with the golden generator)
def camera_dict(B, seed, device='cpu', dtype=torch.float32):
    ti, km, pv, rw, tw = gi.camera_params(B, seed=seed)
    x = {'trans_image': ti, 'k_mat': km, 'pelvis': pv, 'rot_world': rw, 'trans_world': tw}
    out = {'%s_%s' % (MODE, k): T(v).to(device=device, dtype=dtype) for k, v in x.items()}
    out[MODE + '_img'] = torch.zeros(B, 3, S, S)                      # only .shape is read
    return out


def patch_points():
    """[4,3,18,3] normalised patch points, uniform(-0.9, 0.9)."""
    return np.random.Generator(np.random.PCG64(132)).uniform(-0.9, 0.9, (4, 3, 18, 3)).astype(np.float32)


def grad_weights():
    return np.random.Generator(np.random.PCG64(133)).standard_normal((4, 3, 18, 3)).astype(np.float32)


def pre_rotation(B, seed):
    """[B,3,3]: a rotation plus a small perturbation (not orthonormal: the gradient w.r.t. every entry is exercised)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.stack([gi.random_rotation(rng) + 0.05 * rng.standard_normal((3, 3)) for _ in range(B)]).astype(np.float32)


def smpl_params(B, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return ((0.4 * rng.standard_normal((B, 69))).astype(np.float32), rng.standard_normal((B, 10)).astype(np.float32),
            rng.standard_normal((B, 18, 3)).astype(np.float32))


# ------------------------------------------------------------------ float64 restatement
def cams64(x):
    return {k: v.double() for k, v in x.items() if not k.endswith('_img')}


def f64_pelvis_world(x):
    d = (x[MODE + '_pelvis'] - x[MODE + '_trans_world']).unsqueeze(-1)
    return torch.linalg.solve(x[MODE + '_rot_world'], d).squeeze(-1).unsqueeze(1)           # [B,1,3]


def f64_project(p, x, is_norm=True, pre_rot=None, pre_scale=1.0, pelvis_origin=False, stop=None, size=S, rect=RECT):
    """p [B,N,3] or [B,Hy,K,3] (float64), x: float64 camera dict -> the same shape."""
    shape = p.shape
    p = p.reshape(shape[0], -1, 3)
    if pre_rot is not None:
        p = torch.einsum('bni,bij->bnj', p, pre_rot) * pre_scale
    if pelvis_origin:
        p = p + f64_pelvis_world(x)
    if stop == 'world':
        return p.reshape(shape)
    km, pv, ti = x[MODE + '_k_mat'], x[MODE + '_pelvis'], x[MODE + '_trans_image']
    c = torch.einsum('bij,bnj->bni', x[MODE + '_rot_world'], p) + x[MODE + '_trans_world'].unsqueeze(1)
    u = c[..., 0] / c[..., 2] * km[:, 0, 0, None] + km[:, 0, 2, None]
    v = c[..., 1] / c[..., 2] * km[:, 1, 1, None] + km[:, 1, 2, None]
    if stop == 'image':
        return torch.stack([u, v, c[..., 2]], dim=-1).reshape(shape)
    z = (c[..., 2] - pv[:, 2, None]) / (rect / size)
    px = ti[:, 0, 0, None] * u + ti[:, 0, 1, None] * v + ti[:, 0, 2, None]
    py = ti[:, 1, 0, None] * u + ti[:, 1, 1, None] * v + ti[:, 1, 2, None]
    if is_norm:
        px, py, z = px / (size - 1) * 2 - 1, py / (size - 1) * 2 - 1, z / (size - 1)
    return torch.stack([px, py, z], dim=-1).reshape(shape)


def f64_rotations(axisang):
    """[N,3] axis-angle -> [N,3,3] through the unit quaternion; the angle is |axisang + 1e-8| as in the SMPL layer, which
    keeps the zero root rotation of this path finite."""
    angle = (axisang + 1e-8).norm(dim=1, keepdim=True)
    q = torch.cat([torch.cos(angle / 2), torch.sin(angle / 2) * axisang / angle], dim=1)
    w, a, b, c = (q / q.norm(dim=1, keepdim=True)).unbind(1)
    return torch.stack([w * w + a * a - b * b - c * c, 2 * (a * b - w * c), 2 * (w * b + a * c),
                        2 * (w * c + a * b), w * w - a * a + b * b - c * c, 2 * (b * c - w * a),
                        2 * (a * c - w * b), 2 * (w * a + b * c), w * w - a * a - b * b + c * c], dim=1).view(-1, 3, 3)


def f64_smpl_verts(pose, betas, buf):
    """pose [B,72], betas [B,10], buf: float64 SMPL arrays -> vertices [B,V,3] in metres, minus the root joint."""
    B = pose.shape[0]
    R = f64_rotations(pose.reshape(-1, 3)).view(B, 24, 3, 3)
    shaped = buf['v_template'].reshape(1, -1, 3) + torch.einsum('vcs,bs->bvc', buf['shapedirs'], betas)
    rest = torch.einsum('jv,bvc->bjc', buf['J_regressor'], shaped)
    feature = (R[:, 1:] - torch.eye(3, dtype=pose.dtype)).reshape(B, 207)
    posed = shaped + torch.einsum('vcp,bp->bvc', buf['posedirs'], feature)
    rot, pos = [R[:, 0]], [rest[:, 0]]                                  # global rotation / position of every joint
    for i in range(1, 24):
        par = SMPL_PARENTS[i]
        rot.append(rot[par] @ R[:, i])
        pos.append(pos[par] + torch.einsum('brc,bc->br', rot[par], rest[:, i] - rest[:, par]))
    rot, pos = torch.stack(rot, 1), torch.stack(pos, 1)
    shift = pos - torch.einsum('bjrc,bjc->bjr', rot, rest)               # takes the rest pose out
    blend_r = torch.einsum('vj,bjrc->bvrc', buf['weights'], rot)
    blend_t = torch.einsum('vj,bjr->bvr', buf['weights'], shift)
    return torch.einsum('bvrc,bvc->bvr', blend_r, posed) + blend_t - pos[:, 0:1]


def f64_h36m(verts, regressor):
    j = torch.einsum('bvc,lv->blc', verts, regressor)
    j = j[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13]]
    j = torch.cat([j, (j[:, 11:12] + j[:, 14:15]) / 2], dim=1)
    return j - j[:, 0:1]


def f64_project_smpl(grot, pose, betas, buf, x, convert_verts=False):
    full = torch.cat([torch.zeros(pose.shape[0], 3, dtype=pose.dtype), pose], dim=1)
    verts = f64_smpl_verts(full, betas, buf)
    if convert_verts:
        return f64_project(verts, x, pre_rot=grot, pre_scale=1000.0, pelvis_origin=True, stop='world')
    return f64_project(f64_h36m(verts, buf['h36m_regressor']), x, is_norm=False, pre_rot=grot, pre_scale=1000.0,
                       pelvis_origin=True)


def smpl_buffers64(V):
    return {k: T(v).double() for k, v in gi.smpl_buffers(seed=SMPL_BUF_SEED, V=V).items()}


# ------------------------------------------------------------------ shared state of the GPU tests
@functools.lru_cache(maxsize=None)
def G():
    return golden('reproject')


def dev(name):
    return float(G()['dev_' + name])


def err(got, ref):
    return float((got.detach().double().cpu() - ref.detach().double().cpu()).abs().max())


def check(got, ref64, name, gold=None, what=''):
    """HIP result against float64 (4 x the reference's deviation) and, when given, against the float32 golden (5 x)."""
    d = dev(name)
    e64 = err(got, ref64)
    eg = err(got, T(gold)) if gold is not None else 0.0
    print('%s %s: |hip - f64| %.3e (bar %.3e)  |hip - golden| %.3e (bar %.3e)' % (what, name, e64, 4 * d, eg, 5 * d))
    assert e64 <= 4 * d, '%s %s: %.3e from float64, bar %.3e' % (what, name, e64, 4 * d)
    assert eg <= 5 * d, '%s %s: %.3e from the golden, bar %.3e' % (what, name, eg, 5 * d)


@functools.lru_cache(maxsize=None)
def fixture():
    """Inputs on the GPU, float64 copies on the CPU (computed once, never modified)."""
    g = G()
    x = camera_dict(4, CAM_SEED, 'cuda')
    return {'x': x, 'x64': cams64(camera_dict(4, CAM_SEED)), 'world': T(g['world']), 'pts_rot': T(g['pts_rot']),
            'rot': T(pre_rotation(4, 134)), 'gw': T(grad_weights())}


def sub(x, sl):
    return {k: (v if k.endswith('_img') else v[sl]) for k, v in x.items()}


gpu = pytest.mark.gpu


# ------------------------------------------------------------------ forward
@gpu
@pytest.mark.parametrize('name,kw,stop', [('norm', dict(is_norm=True), None), ('px', dict(is_norm=False), None)])
def test_forward_vs_golden(name, kw, stop):
    from xas_amd import ops_head
    f = fixture()
    w = f['world'][:, 0]                                               # [B,K,3]
    out = ops_head.world_to_patch(w.cuda(), f['x'], MODE, **kw)
    assert out.shape == (4, 18, 3)
    check(out, f64_project(w.double(), f['x64'], **kw), name, G()['patch_' + name], 'forward')


@gpu
def test_forward_stop_at_image_vs_golden():
    from xas_amd import ops_head
    f = fixture()
    w = f['world'][:, 0]
    out = ops_head.world_to_patch(w.cuda(), f['x'], MODE, stop_at_image=True)
    ref = f64_project(w.double(), f['x64'], stop='image')
    check(out[..., :2], ref[..., :2], 'image_uv', G()['image'][..., :2], 'forward')
    check(out[..., 2], ref[..., 2], 'image_z', G()['image'][..., 2], 'forward')


@gpu
def test_hypothesis_axis_equals_per_hypothesis_calls():
    from xas_amd import ops_head
    f = fixture()
    w = f['world'].cuda()                                              # [B,3,K,3]
    out = ops_head.world_to_patch(w, f['x'], MODE)
    assert out.shape == (4, 3, 18, 3)
    for h in range(3):
        assert torch.equal(out[:, h], ops_head.world_to_patch(w[:, h].contiguous(), f['x'], MODE))
    check(out, f64_project(f['world'].double(), f['x64']), 'norm', what='hypotheses')
    rot = f['rot'].cuda()
    p = f['pts_rot'].cuda()
    kw = dict(is_norm=False, pre_rot=rot, pre_scale=1000.0, pelvis_origin=True)
    out = ops_head.world_to_patch(p, f['x'], MODE, **kw)
    for h in range(3):
        assert torch.equal(out[:, h], ops_head.world_to_patch(p[:, h].contiguous(), f['x'], MODE, **kw))
    ref = f64_project(f['pts_rot'].double(), f['x64'], is_norm=False, pre_rot=f['rot'].double(), pre_scale=1000.0, pelvis_origin=True)
    check(out, ref, 'rot_px', G()['patch_rot_px'], 'rotated')


@gpu
def test_round_trip():
    """patch -> world -> patch and world -> patch -> world on the inputs of geometry.npz.  Bar: 4 x the error of the
    reference's own float32 round trip on the same inputs (stored by the generator)."""
    from xas_amd import ops_head
    from modules.util import convert_patch_to_world
    g = golden('geometry')
    x = camera_dict(4, 31, 'cuda')
    k = T(g['kps']).cuda()
    back = ops_head.world_to_patch(convert_patch_to_world(k, x, MODE), x, MODE)
    e = err(back, k)
    print('round trip patch: %.3e (bar %.3e)' % (e, 4 * dev('rt_patch')))
    assert e <= 4 * dev('rt_patch')
    w = T(g['world']).cuda()
    back = convert_patch_to_world(ops_head.world_to_patch(w, x, MODE), x, MODE)
    e = err(back, w)
    print('round trip world: %.3e (bar %.3e)' % (e, 4 * dev('rt_world')))
    assert e <= 4 * dev('rt_world')


# ------------------------------------------------------------------ backward
def _hip_grads(case, rotated, **kw):
    from xas_amd import ops_head
    f = fixture()
    b, h, k = CASES[case]
    src = f['pts_rot'] if rotated else f['world']
    p = src[b, h, k].contiguous().cuda().requires_grad_(True)
    x = sub(f['x'], b)
    rot = f['rot'][b].contiguous().cuda().requires_grad_(True) if rotated else None
    if rotated:
        kw.update(pre_rot=rot, pre_scale=1000.0, pelvis_origin=True)
    out = ops_head.world_to_patch(p, x, MODE, **kw)
    (out * f['gw'][b, h, k].cuda()).sum().backward()
    return out.detach(), p.grad, (rot.grad if rotated else None)


def _f64_grads(case, rotated, **kw):
    f = fixture()
    b, h, k = CASES[case]
    src = f['pts_rot'] if rotated else f['world']
    p = src[b, h, k].double().requires_grad_(True)
    x = sub(f['x64'], b)
    rot = f['rot'][b].double().requires_grad_(True) if rotated else None
    if rotated:
        kw.update(pre_rot=rot, pre_scale=1000.0, pelvis_origin=True)
    out = f64_project(p, x, **kw)
    (out * f['gw'][b, h, k].double()).sum().backward()
    return out.detach(), p.grad, (rot.grad if rotated else None)


@gpu
@pytest.mark.parametrize('name,kw', [('norm', dict(is_norm=True)), ('image', dict(stop_at_image=True))])
def test_backward_points_vs_golden_and_float64(name, kw):
    _, gp, _ = _hip_grads('full', False, **kw)
    kw64 = dict(stop='image') if name == 'image' else kw
    _, ref, _ = _f64_grads('full', False, **kw64)
    check(gp, ref, 'g_pts_' + name, G()['g_pts_' + name], 'backward')


@gpu
@pytest.mark.parametrize('case', list(CASES))
def test_backward_pre_rot_vs_golden_and_float64(case):
    """grad_pts and grad_pre_rot of the rotated / shifted path for every point count of CASES (54, 51, 17 points per sample:
    no multiple of the wave; one sample alone), against the reference's autograd (golden) and float64 autograd."""
    out, gp, gr = _hip_grads(case, True, is_norm=False)
    ref_out, ref_gp, ref_gr = _f64_grads(case, True, is_norm=False)
    b, h, k = CASES[case]
    assert gr.shape == (b.stop - b.start, 3, 3)
    check(out, ref_out, 'rot_px', what=case)
    check(gp, ref_gp, 'g_pts_rot', G()['g_pts_rot'][b, h, k], case)
    check(gr, ref_gr, 'g_rot_' + case, G()['g_rot_' + case], case)


@gpu
@pytest.mark.selfcheck
def test_forward_and_backward_are_bit_reproducible():
    runs = [_hip_grads('full', True, is_norm=False) + _hip_grads('k17', True, is_norm=True)[1:] for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ SMPL path
def _smpl_inputs(B=2):
    pose, betas, gw = smpl_params(B, 136)
    return T(pre_rotation(B, 135)), T(pose), T(betas), T(gw)


@gpu
def test_project_smpl_vs_golden():
    from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer
    from modules.util import project_smpl_to_patch_kps
    buf = gi.smpl_buffers(seed=SMPL_BUF_SEED)
    lay = SMPL_Layer.from_arrays(buf, center_idx=0).cuda()
    reg = T(buf['h36m_regressor']).cuda()
    x = camera_dict(2, SMPL_CAM_SEED, 'cuda')
    x64 = cams64(camera_dict(2, SMPL_CAM_SEED))
    grot, pose, betas, _ = _smpl_inputs()
    b64 = smpl_buffers64(6890)
    kps = project_smpl_to_patch_kps(grot.cuda(), pose.cuda(), betas.cuda(), lay, reg, x, MODE)
    assert kps.shape == (2, 18, 3)
    check(kps, f64_project_smpl(grot.double(), pose.double(), betas.double(), b64, x64), 'smpl_kps', G()['smpl_kps'], 'smpl')
    verts = project_smpl_to_patch_kps(grot.cuda(), pose.cuda(), betas.cuda(), lay, reg, x, MODE, convert_verts=True)
    assert verts.shape == (2, 6890, 3)
    ref = f64_project_smpl(grot.double(), pose.double(), betas.double(), b64, x64, convert_verts=True)
    check(verts[:, ::10], ref[:, ::10], 'smpl_verts', G()['smpl_verts_sub'], 'smpl')
    check(verts, ref, 'smpl_verts', what='smpl (all vertices)')


@gpu
def test_project_smpl_gradients_vs_float64():
    """d/d(global_rot_params, pose_params, shape_params) of a random-weighted sum of the patch joints, at the reduced vertex
    count V = 300 (three vertex blocks, the last one ragged), against float64 autograd of the restatement and against the
    reference's own float32 autograd (golden)."""
    from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer
    from modules.util import project_smpl_to_patch_kps
    buf = gi.smpl_buffers(seed=SMPL_BUF_SEED, V=SMPL_SMALL_V)
    lay = SMPL_Layer.from_arrays(buf, center_idx=0).cuda()
    x = camera_dict(2, SMPL_CAM_SEED, 'cuda')
    grot, pose, betas, gw = _smpl_inputs()
    leaves = [t.cuda().requires_grad_(True) for t in (grot, pose, betas)]
    kps = project_smpl_to_patch_kps(*leaves, lay, T(buf['h36m_regressor']).cuda(), x, MODE)
    grads = torch.autograd.grad((kps * gw.cuda()).sum(), leaves)
    l64 = [t.double().requires_grad_(True) for t in (grot, pose, betas)]
    k64 = f64_project_smpl(*l64, smpl_buffers64(SMPL_SMALL_V), cams64(camera_dict(2, SMPL_CAM_SEED)))
    g64 = torch.autograd.grad((k64 * gw.double()).sum(), l64)
    check(kps, k64, 'smpl300_kps', G()['smpl300_kps'], 'smpl V=300')
    for name, got, ref in zip(('g_smpl_rot', 'g_smpl_pose', 'g_smpl_shape'), grads, g64):
        check(got, ref, name, G()[name], 'smpl V=300')


# ------------------------------------------------------------------ small helpers
@gpu
def test_convert_pelvis_to_world_vs_golden():
    from modules.util import convert_pelvis_to_world
    f = fixture()
    out = convert_pelvis_to_world(f['x'], MODE)
    assert out.shape == (4, 1, 3)
    check(out, f64_pelvis_world(f['x64']), 'pelvis_w', G()['pelvis_world'], 'pelvis')


@gpu
def test_flip_3d_swaps_one_group_by_the_seeded_draw():
    from modules.util import flip_3D
    k = T(grad_weights()[:, 0]).cuda()
    legs, arms = list(range(18)), list(range(18))
    legs[1:7] = [4, 5, 6, 1, 2, 3]
    arms[11:17] = [14, 15, 16, 11, 12, 13]
    seen = set()
    for seed in range(8):
        torch.manual_seed(seed)
        draw = float(torch.rand(1))
        torch.manual_seed(seed)
        out = flip_3D(k)
        follow = float(torch.rand(1))
        torch.manual_seed(seed)
        torch.rand(1)
        assert follow == float(torch.rand(1))                        # exactly one draw was consumed
        assert torch.equal(out, k[:, legs if draw < 0.5 else arms])
        assert not torch.equal(out, k)
        seen.add(draw < 0.5)
    assert seen == {True, False}
    assert torch.equal(k, T(grad_weights()[:, 0]).cuda())             # the input is left alone
