"""xas_smpl_fit / xas_smpl_fit_linearise on the GPU against tests/_smplfit_oracle.py (float64 torch on oracle.smpl, autograd
Jacobian, the header's LM step for step), on the synthetic body of tests/_smplfit_inputs.py.

Bounds.  Both sides are double arithmetic on the same fp32 inputs, so they differ by rounding only.  The largest gaps of a
run of this file are recorded in profiles/smpl_fit_check.txt; LIN_BOUND and PARAM_BOUND are 16 x the largest recorded
figure (a margin for other seeds), and LIN_BOUND must stay below 1e-8: above that the arithmetic is not double."""
import numpy as np
import pytest
import torch

import _smplfit_cases as sc
import _smplfit_inputs as si
import _smplfit_oracle as so

pytestmark = pytest.mark.gpu

LIN_BOUND = 16 * 1.252e-15       # max |J - J_oracle| / max |J_oracle| and the same for r (profiles/smpl_fit_check.txt)
PARAM_BOUND = 16 * 9.969e-14     # max |x - x_oracle| / max |x_oracle| of a fit (profiles/smpl_fit_check.txt)
assert LIN_BOUND < 1e-8
WP, WS = sc.POSE_PRIOR, sc.SHAPE_PRIOR
_cache = {}


def layer_of(V, reg='dense'):
    key = (V, reg)
    if key not in _cache:
        from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer
        a = si.arrays(V, reg)
        _cache[key] = (a, SMPL_Layer.from_arrays(a, center_idx=0).cuda(), torch.as_tensor(a['h36m_regressor']).cuda(),
                       so.model_arrays(a))
    return _cache[key]


def split(x):
    """x [B,85] -> the init dict of ops_smplfit (float32, cuda)."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
    return {'pose': torch.cat([x[:, :3], x[:, 6:75]], 1).cuda(), 'trans': x[:, 3:6].contiguous().cuda(), 'betas': x[:, 75:].contiguous().cuda()}


def join(out):
    """fit output -> x [B,85] float64 on the CPU."""
    p = out['pose'].cpu()
    return torch.cat([p[:, :3], out['trans'].cpu(), p[:, 3:], out['betas'].cpu()], 1)


def lin_inputs(V, seed):
    """B = 3: zero body pose and betas; two random poses with angles up to 1 rad.  Joint 3 of every sample and joints 0 and 17
    of sample 2 have weight 0 and a NaN target; the other weights are uneven."""
    x = si.random_params(3, seed, pose_amp=1.0)
    x[0, 6:] = 0
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    tgt = rng.uniform(-800, 800, (3, 18, 3)).astype(np.float32) + x[:, None, 3:6].astype(np.float32)
    w = rng.uniform(0.2, 3.0, (3, 18)).astype(np.float32)
    w[:, 3] = 0
    w[2, 0] = w[2, 17] = 0
    tgt[w == 0] = np.nan
    return x, tgt, w


@pytest.mark.parametrize('reg', si.REGRESSORS)
@pytest.mark.parametrize('V', si.SIZES)
def test_linearise_against_the_oracle(V, reg):
    from xas_amd import ops_smplfit
    a, layer, hreg, m = layer_of(V, reg)
    x, tgt, w = lin_inputs(V, 11 + V)
    r, J = ops_smplfit.linearise_smpl(torch.as_tensor(tgt).cuda(), torch.as_tensor(w).cuda(), layer, hreg, split(x), WP, WS)
    r, J = r.cpu(), J.cpu()
    worst = 0.0
    for b in range(3):
        ro, Jo = so.linearise(torch.as_tensor(x[b]), m, torch.as_tensor(tgt[b]).double(), torch.as_tensor(w[b]).double(), WP, WS)
        gj = float((J[b] - Jo).abs().max() / Jo.abs().max())
        gr = float((r[b] - ro).abs().max() / ro.abs().max())
        print('linearise V=%d %s sample %d: J gap %.3e  r gap %.3e  (max |J| %.3e)' % (V, reg, b, gj, gr, float(Jo.abs().max())))
        worst = max(worst, gj, gr)
        off = [3] + ([0, 17] if b == 2 else [])
        for k in off:                                                     # weight 0: exactly nothing
            assert (J[b, 3 * k:3 * k + 3] == 0).all() and (r[b, 3 * k:3 * k + 3] == 0).all()
    assert torch.isfinite(J).all() and torch.isfinite(r).all()
    assert worst <= LIN_BOUND, 'largest gap %.3e over the bound %.3e' % (worst, LIN_BOUND)


def fitted():
    """The kernel's fits of every planted case, in groups of B = 3 (computed once)."""
    if 'fit' not in _cache:
        from xas_amd import ops_smplfit
        c = sc.load()
        a, layer, hreg, m = layer_of(sc.V, sc.REG)
        n = len(c['index'])
        outs = []
        for s in range(0, n, 3):
            tg = torch.as_tensor(c['targets'][s:s + 3]).cuda()
            outs.append(ops_smplfit.fit_smpl(tg, torch.ones(tg.shape[0], 18, device='cuda'), layer, hreg, init=None, iters=sc.MAX_ITERS,
                                             pose_prior=WP, shape_prior=WS))
        _cache['fit'] = (c, {k: torch.cat([o[k] for o in outs]).cpu() for k in outs[0]})
    return _cache['fit']


def test_fit_reaches_the_oracles_minimum():
    c, out = fitted()
    a, layer, hreg, m = layer_of(sc.V, sc.REG)
    n = len(c['index'])
    assert n >= 8 and (c['gap2'] < sc.KEEP_GAP).all()
    x = join(out)
    w = torch.ones(18, dtype=torch.float64)
    worst = 0.0
    for i in range(n):
        xo, Co = torch.as_tensor(c['x'][i]), float(c['cost'][i, 1])
        tg = torch.as_tensor(c['targets'][i]).double()
        r, J = so.linearise(x[i], m, tg, w, WP, WS)
        g = float((J.T @ r).abs().max())
        gap = float((x[i] - xo).abs().max() / xo.abs().max())
        C0, C1 = float(out['cost'][i, 0]), float(out['cost'][i, 1])
        print('fit case %d: status %d, %d trials (oracle %d), cost %.6f -> %.9f (oracle %.9f), |J^T r| %.3e of %.3e, parameter gap %.3e'
              % (int(c['index'][i]), int(out['status'][i]), int(out['iters'][i]), int(c['iters'][i]), C0, C1, Co, g, float(c['g0'][i]), gap))
        worst = max(worst, gap)
        assert int(out['status'][i]) == 0
        # the linearise gap in cost terms: d C = 2 |r| |dr| <= 2 C LIN_BOUND
        assert C1 <= Co * (1 + 1e-9) + 2 * Co * LIN_BOUND
        assert g <= 1e-6 * float(c['g0'][i])
        assert gap <= PARAM_BOUND, 'case %d: parameter gap %.3e over %.3e' % (i, gap, PARAM_BOUND)
        assert abs(C1 - so.cost_of(r)) <= 1e-9 * C1
    print('fit: largest parameter gap %.3e' % worst)


def test_masking_and_pass_through():
    from xas_amd import ops_smplfit
    c, _ = fitted()
    a, layer, hreg, m = layer_of(sc.V, sc.REG)
    tg = torch.as_tensor(c['targets'][:3]).clone()
    w = torch.ones(3, 18)
    w[:, 5] = 0
    w[1, 9] = 0
    init = split(c['x0'][:3])
    run = lambda t, ww, ini: ops_smplfit.fit_smpl(t.cuda(), ww.cuda(), layer, hreg, init=ini, iters=6, pose_prior=WP, shape_prior=WS)
    fin = run(tg, w, init)
    tn = tg.clone()
    tn[:, 5] = float('nan')
    tn[1, 9] = float('inf')
    nan = run(tn, w, init)
    for k in fin:
        assert torch.equal(fin[k], nan[k]), k                             # a target of weight 0 changes no bit
    assert (fin['status'] != 2).all() and (fin['cost'][:, 1] < fin['cost'][:, 0]).all()
    # five usable joints: passed through
    w5 = torch.zeros(3, 18)
    w5[:, :5] = 1
    w5[2, 5] = 1                                                          # sample 2 has six: it is fitted
    out = run(tg, w5, init)
    assert out['status'].tolist()[:2] == [2, 2] and int(out['status'][2]) != 2
    x0 = torch.as_tensor(c['x0'][:3]).float().double()
    assert torch.equal(join(out)[:2], x0[:2]) and not torch.equal(join(out)[2], x0[2])
    assert torch.equal(out['cost'][:2, 0], out['cost'][:2, 1]) and out['iters'].tolist()[:2] == [0, 0]
    for b in range(2):
        assert float((out['joints'][b].cpu() - so.joints(x0[b], m)).abs().max()) < 1e-6
    # a parameter that is not finite: passed through, the inputs come back
    bad = {k: v.clone() for k, v in init.items()}
    bad['pose'][0, 7] = float('nan')
    bad['trans'][1, 2] = float('inf')
    out = run(tg, torch.ones(3, 18), bad)
    assert out['status'].tolist()[:2] == [2, 2] and int(out['status'][2]) != 2
    assert torch.equal(out['pose'][:2].float().cpu().isnan(), bad['pose'][:2].cpu().isnan())
    keep = ~bad['pose'][:2].cpu().isnan()
    assert torch.equal(out['pose'][:2].cpu()[keep], bad['pose'][:2].cpu().double()[keep])
    assert torch.equal(out['trans'][:2].cpu(), bad['trans'][:2].cpu().double())


def test_zero_iterations_return_the_start():
    from xas_amd import ops_smplfit
    c, _ = fitted()
    a, layer, hreg, m = layer_of(sc.V, sc.REG)
    tg = torch.as_tensor(c['targets'][:3])
    out = ops_smplfit.fit_smpl(tg.cuda(), torch.ones(3, 18).cuda(), layer, hreg, init=split(c['x0'][:3]), iters=0, pose_prior=WP,
                               shape_prior=WS)
    assert torch.equal(out['cost'][:, 0], out['cost'][:, 1]) and out['iters'].tolist() == [0, 0, 0] and out['status'].tolist() == [1, 1, 1]
    assert torch.equal(join(out), torch.as_tensor(c['x0'][:3]).float().double())
    for b in range(3):
        Co = float(c['cost'][b, 0])
        assert abs(float(out['cost'][b, 0]) - Co) <= 2 * Co * LIN_BOUND


def test_determinism_and_batch_independence():
    from xas_amd import ops_smplfit
    c, first = fitted()
    a, layer, hreg, m = layer_of(sc.V, sc.REG)
    tg = torch.as_tensor(c['targets'][:3]).cuda()
    run = lambda t: ops_smplfit.fit_smpl(t, torch.ones(t.shape[0], 18, device='cuda'), layer, hreg, iters=sc.MAX_ITERS, pose_prior=WP,
                                         shape_prior=WS)
    again, one = run(tg), run(tg[1:2])
    for k in again:
        assert torch.equal(again[k].cpu(), first[k][:3]), k
        assert torch.equal(one[k][0], again[k][1]), k


def test_fitted_parameters_through_the_existing_kernels():
    """xas_smpl_lbs_fwd + smpl_to_h36m in fp32, root rotation and translation applied as project_smpl_to_patch_kps applies them
    (row vector times R^T, x 1000), against the fit's own joints: 4 ulp (fp32) of the largest coordinate."""
    from modules.util import smpl_to_h36m
    from xas_amd.pseudo import _rodrigues
    c, out = fitted()
    a, layer, hreg, m = layer_of(sc.V, sc.REG)
    pose, betas, trans = out['pose'].float().cuda(), out['betas'].float().cuda(), out['trans'].float().cuda()
    verts, _ = layer(torch.cat([torch.zeros_like(pose[:, :3]), pose[:, 3:]], 1), betas)
    j = smpl_to_h36m(verts, hreg)
    G = _rodrigues(pose[:, :3].double().cpu()).transpose(1, 2).float().cuda()
    Y = torch.bmm(j, G) * 1000.0 + trans.unsqueeze(1)
    err = float((Y.double().cpu() - out['joints']).abs().max())
    big = float(out['joints'].abs().max())
    print('fit joints vs the fp32 path: %.3e mm at a largest coordinate of %.1f mm' % (err, big))
    assert err <= 4 * np.spacing(np.float32(big))


def test_fit_output_renders_as_a_pseudo_bank(tmp_path):
    from modules import util as mu
    from xas_amd.pseudo import PseudoSynth
    from xas_amd.synthetic import synthetic_batch
    c, out = fitted()
    a, layer, hreg, m = layer_of(sc.V, sc.REG)
    path = str(tmp_path / 'fit.npz')
    np.savez(path, pose=out['pose'].float().numpy(), betas=out['betas'].float().numpy(), trans=out['trans'].float().numpy(),
             cost=out['cost'].float().numpy(), status=out['status'].numpy(), joint_rms_mm=np.zeros(len(out['status']), np.float32))
    x = synthetic_batch(2, [0], torch.device('cuda'), seed=8)
    synth = PseudoSynth(path, layer, hreg, 'shade', seed=5)
    synth.fill(x, ['cam_0'])
    S = x['cam_0_img'].shape[-1]
    assert float((x['cam_0_pseudo_img'] != x['cam_0_pseudo_img'][:, :, :1, :1]).sum()) > 0      # the mask is not empty
    rows, ang = PseudoSynth(path, layer, hreg, 'shade', seed=5).draw(2)
    # the fitted joints, root-centred and turned as the bank row is turned, projected by the existing launch
    from xas_amd.pseudo import _rodrigues
    from xas_amd import ops_head
    J = out['joints'][rows] - out['trans'][rows].unsqueeze(1)                               # R(omega) 1000 j
    turn = _rodrigues(synth.up.unsqueeze(0) * ang.unsqueeze(1))
    world = torch.einsum('bij,bkj->bki', turn, J).float().cuda() / 1000.0
    eye = torch.eye(3, device='cuda').expand(2, 3, 3).contiguous()
    kps = ops_head.world_to_patch(world, x, 'cam_0', is_norm=False, pre_rot=eye, pre_scale=1000.0, pelvis_origin=True)
    expect = mu.normalise_patch_joints(kps, S)
    err = float((x['cam_0_pseudo_joints'] - expect).abs().max())
    print('pseudo joints vs the projection of the fitted joints: %.3e (normalised units)' % err)
    assert err <= 1e-4
