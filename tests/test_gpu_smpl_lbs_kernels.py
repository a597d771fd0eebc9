"""The SMPL skinning kernels of csrc/smpl_lbs.hip alone, through the C ABI (xas_smpl_lbs_fwd / xas_smpl_lbs_bwd), against
float64 oracle.smpl.smpl_lbs and its autograd on the CPU, computed from the same fp32 inputs - at the vertex counts where the
tiling changes: V = 1 (one vertex), 127 (one block of the vertex passes with a tail), 128 (an exact block), 129 (a block plus one
vertex) and 300 (more than 256: the block loops of the joint regressor and of the d(betas) pass wrap), for one and two samples and
for no centre joint, the root and the last joint.  Every output buffer is filled with NaN before the launch.

Bars: those of the SMPL tests of test_gpu_model.py, which run the layer at V = 6890 - 3e-5 absolute on vertices and joints
(metres), 2e-4 of the largest reference gradient on d(pose) and d(betas).  The gradient at an exactly zero rotation divides by
the 1e-8 guard of rodrigues_layer.py:41 and is left out of the comparison, as there.

One size has a bar of its own.  At V = 1 the joint regressor puts all 24 joints on the one vertex, so with a centre joint the
vertex minus the centre does not depend on the shape: the reference d(betas) is 1e-9 at the most where it is 0.1 - 0.4 in every
other case, and an error relative to it measures nothing (56 to 218 before this file existed, from an absolute error of
6.7e-8 to 1.63e-7 - the absolute error of every other case lies in 1.8e-8 .. 1.3e-7).  There d(betas) is held absolutely, to
twice the worst error seen: 3.3e-7."""
import functools

import numpy as np
import pytest
import torch

import inputs as gi
from oracle import smpl as osmpl

pytestmark = pytest.mark.gpu

FWD_BAR, GRAD_BAR = 3e-5, 2e-4
BETAS_ABS_BAR_V1_CENTRED = 2 * 1.632e-7          # V = 1 with a centre joint (see above)
BUF_SEED = 71
KEYS = ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights')
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def buffers(V):
    """-> (fp32 CPU tensors in the entry points' order, the same on the GPU); shared by the cases of a size, never written."""
    buf = gi.smpl_buffers(BUF_SEED, V=V)
    cpu = tuple(T(buf[k]) for k in KEYS)
    return cpu, tuple(t.cuda() for t in cpu)


def case_inputs(B, V, seed, zero_pose=False):
    gen = torch.Generator().manual_seed(seed)
    pose = 0.6 * torch.randn(B, 72, generator=gen)
    pose[0, 9:12] = 0.0                                   # identity rotation: angle = |1e-8|
    if zero_pose:
        pose.zero_()
    betas = torch.randn(B, 10, generator=gen)
    gv = torch.randn(B, V, 3, generator=gen) / V ** 0.5
    gj = torch.randn(B, 24, 3, generator=gen)
    return pose, betas, gv, gj


def reference(V, pose, betas, gv, gj, center):
    """float64 oracle and its autograd -> verts, joints, d_pose, d_betas"""
    cpu, _ = buffers(V)
    p, b = pose.double().requires_grad_(True), betas.double().requires_grad_(True)
    verts, joints = osmpl.smpl_lbs(p, b, *(t.double() for t in cpu), center_idx=None if center < 0 else center)
    loss = (verts * gv.double()).sum()
    if gj is not None:
        loss = loss + (joints * gj.double()).sum()
    loss.backward()
    return verts.detach(), joints.detach(), p.grad, b.grad


def run_kernels(V, pose, betas, gv, gj, center):
    """xas_smpl_lbs_fwd then xas_smpl_lbs_bwd on NaN-filled outputs -> verts, joints, d_pose, d_betas (on the CPU)"""
    from xas_amd._lib import call, ptr, query
    _, dev = buffers(V)
    B = pose.shape[0]
    nans = lambda *s: torch.full(s, float('nan'), device='cuda', dtype=torch.float32)
    parents = torch.tensor(osmpl.SMPL_PARENTS, dtype=torch.int32, device='cuda')
    pg, bg = pose.cuda(), betas.cuda()
    verts, joints, ws = nans(B, V, 3), nans(B, 24, 3), nans(B * (24 * 3 + 24 * 16 + 207))
    call('xas_smpl_lbs_fwd', ptr(pg), ptr(bg), *(ptr(t) for t in dev), ptr(parents), B, V, center, ptr(verts), ptr(joints),
         ptr(ws))
    d_pose, d_betas = nans(B, 72), nans(B, 10)
    ws2 = nans(query('xas_smpl_lbs_bwd_workspace_floats', B, V))
    dv, dj = gv.cuda(), (gj.cuda() if gj is not None else None)
    call('xas_smpl_lbs_bwd', ptr(pg), ptr(bg), *(ptr(t) for t in dev), ptr(parents), B, V, center, ptr(ws), ptr(dv), ptr(dj),
         ptr(d_pose), ptr(d_betas), ptr(ws2))
    return verts.cpu(), joints.cpu(), d_pose.cpu(), d_betas.cpu()


def check(got, ref, pose, tag, betas_abs_bar=None):
    verts, joints, d_pose, d_betas = got
    v_ref, j_ref, p_ref, b_ref = ref
    e_v, e_j = float((verts.double() - v_ref).abs().max()), float((joints.double() - j_ref).abs().max())
    mask = (pose.reshape(-1, 24, 3) != 0).any(-1, keepdim=True).expand(-1, -1, 3).reshape(-1, 72)
    e_b = float((d_betas.double() - b_ref).abs().max()) / float(b_ref.abs().max())
    e_p = float((d_pose.double() - p_ref)[mask].abs().max()) / float(p_ref[mask].abs().max()) if mask.any() else 0.0
    print('%s: verts %.2e joints %.2e (bar %.0e)   d_pose %.2e d_betas %.2e (bar %.0e)' % (tag, e_v, e_j, FWD_BAR, e_p, e_b, GRAD_BAR))
    a_b = float((d_betas.double() - b_ref).abs().max())
    print('   d_betas: absolute error %.3e, largest reference %.3e' % (a_b, float(b_ref.abs().max())))
    assert torch.isfinite(verts).all() and torch.isfinite(joints).all() and torch.isfinite(d_betas).all()
    assert torch.isfinite(d_pose[mask]).all()
    assert e_v < FWD_BAR and e_j < FWD_BAR
    assert e_p < GRAD_BAR
    assert e_b < GRAD_BAR if betas_abs_bar is None else a_b < betas_abs_bar


@pytest.mark.parametrize('center', [-1, 0, 23])
@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('V', [1, 127, 128, 129, 300])
def test_smpl_lbs_kernels_vs_float64(V, B, center):
    pose, betas, gv, gj = case_inputs(B, V, seed=1000 * V + 10 * B + center + 1)
    a = run_kernels(V, pose, betas, gv, gj, center)
    b = run_kernels(V, pose, betas, gv, gj, center)
    for x, y in zip(a, b):                                # no atomics: bit for bit run to run, NaN at the zero rotation or not
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    check(a, reference(V, pose, betas, gv, gj, center), pose, 'V=%d B=%d center=%d' % (V, B, center),
          betas_abs_bar=BETAS_ABS_BAR_V1_CENTRED if V == 1 and center >= 0 else None)


@pytest.mark.parametrize('V', [129, 300])
def test_smpl_lbs_bwd_without_joint_gradient(V):
    """d_joints = NULL is a zero joint gradient: only the vertices send gradient back."""
    pose, betas, gv, _ = case_inputs(2, V, seed=V + 7)
    check(run_kernels(V, pose, betas, gv, None, 0), reference(V, pose, betas, gv, None, 0), pose, 'V=%d no d_joints' % V)


@pytest.mark.parametrize('V', [129, 300])
def test_smpl_lbs_all_zero_pose(V):
    """Every rotation is the identity (angle = |1e-8|): the forward and d(betas) are compared, d(pose) is not (see above)."""
    pose, betas, gv, gj = case_inputs(2, V, seed=V + 11, zero_pose=True)
    check(run_kernels(V, pose, betas, gv, gj, 0), reference(V, pose, betas, gv, gj, 0), pose, 'V=%d zero pose' % V)
