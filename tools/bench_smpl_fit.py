#!/usr/bin/env python3
"""xas_smpl_fit at (B, V) = (32, 6890) on the synthetic body of tests/_smplfit_inputs.py, with its dense H36M regressor and with
one that keeps 10 % of the columns: time per call of ops_smplfit.fit_smpl (compaction of the regressor, workspace and the two
launches) from a given start, with max_iters = 0 (one evaluation), 1 and 10, and of linearise_smpl.  Targets are the model's
own joints at planted parameters (body-pose angles within 0.3 rad), the start is the default one.  Per figure: 3 warm-up calls,
then 5 windows of `--reps` calls back to back with device events around each window, the variants alternating window by window;
the median window is the figure, min and max the spread.  Time per trial = (t(10) - t(0)) / trials made beyond the start.
usage: bench_smpl_fit.py [--out FILE] [--reps N]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
import _smplfit_inputs as si
from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer
from xas_amd import ops_smplfit
argv = sys.argv[1:]
opt = {'--out': None, '--reps': '3'}
for flag in list(opt):
    if flag in argv:
        i = argv.index(flag)
        opt[flag] = argv[i + 1]
        del argv[i:i + 2]
reps, B, V, WINDOWS = int(opt['--reps']), 32, 6890, 5
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


a = si.arrays(V)
layer = SMPL_Layer.from_arrays(a, center_idx=0).cuda()
dense = torch.as_tensor(a['h36m_regressor']).cuda()
keep = torch.zeros(V, dtype=torch.bool)
keep[torch.randperm(V, generator=torch.Generator().manual_seed(1))[:V // 10]] = True
sparse = torch.where(keep.cuda(), dense, torch.zeros_like(dense))
sparse = sparse / sparse.sum(dim=1, keepdim=True)
x = torch.as_tensor(si.random_params(B, 3, pose_amp=0.3), dtype=torch.float32)
planted = {'pose': torch.cat([x[:, :3], x[:, 6:75]], 1).cuda(), 'trans': x[:, 3:6].contiguous().cuda(), 'betas': x[:, 75:].contiguous().cuda()}
ones = torch.ones(B, 18, device='cuda')
say('MI355X, xas_smpl_fit at (B, V) = (%d, %d), synthetic body, priors %g / %g; one workgroup of 256 threads per sample.' % (
    B, V, ops_smplfit.POSE_PRIOR, ops_smplfit.SHAPE_PRIOR))
say('%d windows of %d calls per variant after 3 warm-up calls, device events around each window, variants alternating; ms per call of '
    'ops_smplfit (host preparation + 2 launches): median window (min .. max)' % (WINDOWS, reps))
for tag, reg in (('dense regressor', dense), ('10 % of the columns', sparse)):
    tgt = ops_smplfit.fit_smpl(torch.zeros(B, 18, 3, device='cuda'), ones, layer, reg, init=planted, iters=0)['joints'].float()
    init = ops_smplfit.default_init(tgt, ones, layer, reg)
    fns = (('evaluate (max_iters 0)', lambda: ops_smplfit.fit_smpl(tgt, ones, layer, reg, init=init, iters=0)),
           ('linearise', lambda: ops_smplfit.linearise_smpl(tgt, ones, layer, reg, init)),
           ('fit, max_iters 1', lambda: ops_smplfit.fit_smpl(tgt, ones, layer, reg, init=init, iters=1)),
           ('fit, max_iters 10', lambda: ops_smplfit.fit_smpl(tgt, ones, layer, reg, init=init, iters=10)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _, f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in fns}
    for _ in range(WINDOWS):
        for name, f in fns:
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    say('%s (%d vertices visited)' % (tag, int((reg != 0).any(0).sum())))
    med = {}
    for name, _ in fns:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        say('  %-24s %9.3f  (%.3f .. %.3f)' % (name, med[name], t.min(), t.max()))
    out = fns[3][1]()
    trials = out['iters'].float().mean().item()
    say('  per trial (one solve, one evaluation and, if accepted, one linearisation): %.3f ms at %.1f trials per sample; cost %.4g -> %.4g, '
        'status %s' % ((med['fit, max_iters 10'] - med['evaluate (max_iters 0)']) / max(trials, 1.0), trials, out['cost'][:, 0].mean().item(),
                       out['cost'][:, 1].mean().item(), np.bincount(out['status'].cpu().numpy(), minlength=3).tolist()))
if opt['--out']:
    with open(opt['--out'], 'w') as f:
        f.write('\n'.join(lines) + '\n')
