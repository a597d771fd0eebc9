#!/usr/bin/env python3
"""Generate tests/golden/reproject.npz: the reference's own world -> patch functions and its
project_smpl_to_patch_kps on seeded inputs, IMPORTED from a checkout of the reference (as make_golden.py does; none of
its text is stored).  Run:  XAS_REFERENCE=<checkout> python tests/golden/make_golden_reproject.py

Inputs come from seeds (tests/golden/inputs.py and the helpers at the top of tests/test_gpu_reproject.py); the file
holds outputs only:

* `world` [4,3,18,3]: convert_patch_to_world of patch points drawn from uniform(-0.9, 0.9), and `pts_rot`: the same
  points expressed in metres about the pelvis and turned back through the test's pre-rotation (float64), so that the
  rotated / shifted path lands on the same world points;
* the reference's float32 results and autograd gradients on them;
* `dev_<group>`: the reference's maximum absolute deviation from the float64 restatement of tests/test_gpu_reproject.py
  per output group - the tests' bars are multiples of these;
* `rt_*`: the error of the reference's own float32 round trip on the inputs of geometry.npz.

Every camera-space depth of every fixture is asserted to be above 1000 mm (no near-singular perspective divide)."""
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('XAS_REFERENCE') or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REF or not os.path.isdir(os.path.join(REF, 'modules')):
    sys.exit('set XAS_REFERENCE (or pass the path) to a checkout of the reference project')
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

import numpy as np                                                        # noqa: E402
import torch                                                              # noqa: E402
import torch.nn as nn                                                     # noqa: E402

from modules import util as ref_util                                      # noqa: E402  (before tests/conftest.py puts the mirror in front)
from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer             # noqa: E402
import inputs as gi                                                       # noqa: E402
import test_gpu_reproject as tr                                           # noqa: E402  (input helpers + float64 restatement)

assert os.path.realpath(ref_util.__file__).startswith(os.path.realpath(REF) + os.sep)
torch.set_num_threads(8)
T, MODE = tr.T, tr.MODE
out, devs = {}, {}


def dev(name, got32, ref64):
    d = float((got32.detach().double() - ref64.detach()).abs().max())
    devs[name] = max(devs.get(name, 0.0), d)
    return d


def depth_ok(world, x):
    """camera-space depth of world points [B,N,3] under the float32 camera dict x."""
    c = torch.einsum('bij,bnj->bni', x[MODE + '_rot_world'].double(), world.double().reshape(world.shape[0], -1, 3))
    z = c[..., 2] + x[MODE + '_trans_world'].double()[:, 2, None]
    assert float(z.min()) > 1000.0, 'camera-space depth %.1f mm: pick another seed' % float(z.min())
    return float(z.min())


def ref_smpl_layer(buf):
    """The reference layer built the way make_golden.py's SMPL golden builds it (no licensed pickle)."""
    lay = SMPL_Layer.__new__(SMPL_Layer)
    nn.Module.__init__(lay)
    lay.center_idx, lay.gender, lay.num_joints = 0, 'neutral', 24
    lay.kintree_parents = [4294967295] + list(tr.SMPL_PARENTS[1:])
    lay.register_buffer('th_betas', torch.zeros(1, 10))
    for k in ('shapedirs', 'posedirs', 'v_template', 'J_regressor', 'weights'):
        lay.register_buffer('th_' + k, T(buf[k]))
    return lay


# ------------------------------------------------------------------ plain world -> patch
x = tr.camera_dict(4, tr.CAM_SEED)
x64 = tr.cams64(x)
patch = T(tr.patch_points())
world = torch.stack([ref_util.convert_patch_to_world(patch[:, h], x, MODE, is_norm=True) for h in range(3)], dim=1)
depth_ok(world, x)
gw = T(tr.grad_weights())
out['world'] = world

w0 = world[:, 0].clone().requires_grad_(True)
for name, kw in (('norm', dict(is_norm=True)), ('px', dict(is_norm=False))):
    r = ref_util.convert_world_to_patch(w0, x, MODE, **kw)
    out['patch_' + name] = r
    for h in range(3):
        dev(name, ref_util.convert_world_to_patch(world[:, h], x, MODE, **kw), tr.f64_project(world[:, h].double(), x64, **kw))
km = x[MODE + '_k_mat']
image = lambda p: ref_util.convert_world_to_image(p, km[..., 0, [0]], km[..., 1, [1]], km[..., 0, [2]], km[..., 1, [2]],
                                                  x[MODE + '_trans_world'], x[MODE + '_rot_world'])
img = image(w0)
out['image'] = img
i64 = tr.f64_project(world[:, 0].double(), x64, stop='image')
dev('image_uv', img[..., :2], i64[..., :2])
dev('image_z', img[..., 2], i64[..., 2])
# the gradient tests feed the FULL [4,3,18,3] set to one launch; their plain-path gradients per hypothesis:
for name, fn32, kw64 in (('norm', lambda p: ref_util.convert_world_to_patch(p, x, MODE), {}), ('image', image, dict(stop='image'))):
    gs = []
    for h in range(3):
        p = world[:, h].clone().requires_grad_(True)
        g, = torch.autograd.grad((fn32(p) * gw[:, h]).sum(), p)
        p64 = world[:, h].double().requires_grad_(True)
        g64, = torch.autograd.grad((tr.f64_project(p64, x64, **kw64) * gw[:, h].double()).sum(), p64)
        dev('g_pts_' + name, g, g64)
        gs.append(g)
    out['g_pts_' + name] = torch.stack(gs, dim=1)

pw = ref_util.convert_pelvis_to_world(x, MODE)
out['pelvis_world'] = pw
dev('pelvis_w', pw, tr.f64_pelvis_world(x64))

# ------------------------------------------------------------------ rotated / scaled / pelvis-shifted path (util.py:376-382)
rot = T(tr.pre_rotation(4, 134))
rel = (world.double() - tr.f64_pelvis_world(x64).unsqueeze(1)) / 1000.0
pts_rot = torch.einsum('bhkj,bji->bhki', rel, torch.linalg.inv(rot.double())).float()
out['pts_rot'] = pts_rot


def ref_rotated(p, g, xs, is_norm=False):
    """[B,Hy,K,3] -> the tail of project_smpl_to_patch_kps, one hypothesis at a time."""
    res = []
    for h in range(p.shape[1]):
        j = torch.bmm(p[:, h], g) * 1000
        j = j + ref_util.convert_pelvis_to_world(xs, MODE)
        res.append(ref_util.convert_world_to_patch(j, xs, MODE, is_norm=is_norm))
    return torch.stack(res, dim=1)


for case, (b, h, k) in tr.CASES.items():
    xs, xs64 = tr.sub(x, b), tr.sub(x64, b)
    p = pts_rot[b, h, k].clone().requires_grad_(True)
    g = rot[b].clone().requires_grad_(True)
    r = ref_rotated(p, g, xs)
    gp, gr = torch.autograd.grad((r * gw[b, h, k]).sum(), (p, g))
    p64, r64 = pts_rot[b, h, k].double().requires_grad_(True), rot[b].double().requires_grad_(True)
    o64 = tr.f64_project(p64, xs64, is_norm=False, pre_rot=r64, pre_scale=1000.0, pelvis_origin=True)
    gp64, gr64 = torch.autograd.grad((o64 * gw[b, h, k].double()).sum(), (p64, r64))
    depth_ok(tr.f64_project(p64.detach(), xs64, pre_rot=r64.detach(), pre_scale=1000.0, pelvis_origin=True, stop='world'), xs)
    dev('rot_px', r, o64)
    dev('g_pts_rot', gp, gp64)
    dev('g_rot_' + case, gr, gr64)
    out['g_rot_' + case] = gr
    if case == 'full':
        out['patch_rot_px'], out['g_pts_rot'] = r, gp

# ------------------------------------------------------------------ project_smpl_to_patch_kps
xs = tr.camera_dict(2, tr.SMPL_CAM_SEED)
xs64 = tr.cams64(xs)
grot, pose, betas, gws = tr._smpl_inputs()
for V, tag in ((6890, 'smpl'), (tr.SMPL_SMALL_V, 'smpl300')):
    buf = gi.smpl_buffers(seed=tr.SMPL_BUF_SEED, V=V)
    lay, reg = ref_smpl_layer(buf), T(buf['h36m_regressor'])
    b64 = tr.smpl_buffers64(V)
    leaves = [t.clone().requires_grad_(True) for t in (grot, pose, betas)]
    kps = ref_util.project_smpl_to_patch_kps(*leaves, lay, reg, xs, MODE)
    l64 = [t.double().requires_grad_(True) for t in (grot, pose, betas)]
    k64 = tr.f64_project_smpl(*l64, b64, xs64)
    out[tag + '_kps'] = kps
    dev(tag + '_kps', kps, k64)
    v64 = tr.f64_project_smpl(*[t.detach() for t in l64], b64, xs64, convert_verts=True)
    depth_ok(tr.f64_project(tr.f64_h36m(tr.f64_smpl_verts(torch.cat([torch.zeros(2, 3, dtype=torch.float64), l64[1].detach()], 1),
                                                          l64[2].detach(), b64), b64['h36m_regressor']), xs64, pre_rot=l64[0].detach(),
                            pre_scale=1000.0, pelvis_origin=True, stop='world'), xs)
    if V == 6890:
        verts = ref_util.project_smpl_to_patch_kps(grot, pose, betas, lay, reg, xs, MODE, convert_verts=True)
        out['smpl_verts_sub'] = verts[:, ::10]
        dev('smpl_verts', verts, v64)
        g32 = torch.autograd.grad((kps * gws).sum(), leaves[0])
        out['g_smpl6890_rot'] = g32[0]
    else:
        g32 = torch.autograd.grad((kps * gws).sum(), leaves)
        g64 = torch.autograd.grad((k64 * gws.double()).sum(), l64)
        for name, a, b in zip(('g_smpl_rot', 'g_smpl_pose', 'g_smpl_shape'), g32, g64):
            out[name] = a
            dev(name, a, b)

# ------------------------------------------------------------------ the reference's own float32 round trip (geometry.npz inputs)
geo = np.load(os.path.join(HERE, 'geometry.npz'))
xg = tr.camera_dict(4, 31)
k = T(geo['kps'])
devs['rt_patch'] = float((ref_util.convert_world_to_patch(ref_util.convert_patch_to_world(k, xg, MODE), xg, MODE) - k).abs().max())
w = T(geo['world'])
depth_ok(w, xg)
devs['rt_world'] = float((ref_util.convert_patch_to_world(ref_util.convert_world_to_patch(w, xg, MODE), xg, MODE) - w).abs().max())

for name, d in sorted(devs.items()):
    assert d > 0.0, name
    out['dev_' + name] = np.float64(d)
    print('dev_%-14s %.3e   bar (4 x) %.3e' % (name, d, 4 * d))
arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
np.savez_compressed(os.path.join(HERE, 'reproject.npz'), **arrays)
print('wrote reproject.npz', {k: v.shape for k, v in arrays.items() if not k.startswith('dev_')},
      os.path.getsize(os.path.join(HERE, 'reproject.npz')), 'bytes')
