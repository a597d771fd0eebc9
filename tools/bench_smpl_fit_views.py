#!/usr/bin/env python3
"""xas_smpl_fit_views at (B, V) = (32, 6890) on the synthetic body of tests/_smplfit_inputs.py, with C = 1 (ray anchors) and C = 4
cameras, with the dense H36M regressor and with one that keeps 10 % of the columns: time per call of ops_smplfit (host
preparation, workspace and all the launches) of one linearisation (linearise_smpl_views), of the start alone (max_iters 0), of
one trial (max_iters 1) and of 30 trials, and IN THE SAME RUN of xas_smpl_fit (start, 1 and 30 trials) on the triangulated points
of the same samples (C = 1: the anchors), the yardstick.  The detections are the projected planted joints plus 2 px of noise, the
start is a little off the planted parameters.  Per figure: 1 warm-up call, then 3 windows of `--reps` calls with device events
around each window, the variants alternating window by window; the median window is the figure, min and max the spread.
usage: bench_smpl_fit_views.py [--out FILE] [--reps N] [--batch B]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
import _smplfit_inputs as si
import _smplfit_views_cases as vc
from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer
from xas_amd import ops_smplfit, ops_track
argv = sys.argv[1:]
opt = {'--out': None, '--reps': '1', '--batch': '32'}
for flag in list(opt):
    if flag in argv:
        i = argv.index(flag)
        opt[flag] = argv[i + 1]
        del argv[i:i + 2]
reps, B, V, WINDOWS = int(opt['--reps']), int(opt['--batch']), 6890, 3
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
part = lambda t: {'pose': torch.cat([t[:, :3], t[:, 6:75]], 1).cuda(), 'trans': t[:, 3:6].contiguous().cuda(), 'betas': t[:, 75:].contiguous().cuda()}
planted = part(x)
gen = torch.Generator().manual_seed(4)
off = x.clone()
off[:, :3] += 0.05 * torch.randn(B, 3, generator=gen)
off[:, 3:6] += 20.0 * torch.randn(B, 3, generator=gen)
off[:, 6:75] *= 0.8
off[:, 75:] *= 0.5
init = part(off)
ones = torch.ones(B, 18, device='cuda')
say('MI355X, xas_smpl_fit_views at (B, V) = (%d, %d), synthetic body, priors %g / %g (xas_smpl_fit: %g / %g); workspace %.1f MB.'
    % (B, V, ops_smplfit.VIEWS_POSE_PRIOR, ops_smplfit.VIEWS_SHAPE_PRIOR, ops_smplfit.POSE_PRIOR, ops_smplfit.SHAPE_PRIOR,
       ops_smplfit.views_workspace_bytes(B, V) / 1e6))
say('%d windows of %d calls per variant after 1 warm-up call, device events around each window, variants alternating; ms per call of '
    'ops_smplfit (host preparation + all launches): median window (min .. max)' % (WINDOWS, reps))
for tag, reg in (('dense regressor', dense), ('10 % of the columns', sparse)):
    clean = ops_smplfit.fit_smpl(torch.zeros(B, 18, 3, device='cuda'), ones, layer, reg, init=planted, iters=0)['joints']
    for C in (1, 4):
        Y = clean.cpu().numpy()
        P = np.stack([np.stack([vc.look_at(Y[b].mean(0) + 4000.0 * np.array([np.sin(t), 0.1, -np.cos(t)]), Y[b].mean(0))
                                for t in 2 * np.pi * np.arange(C) / C]) for b in range(B)])
        uv = np.stack([vc.project(P[b], Y[b]) for b in range(B)]) + 2.0 * torch.randn(B, C, 18, 2, generator=gen).numpy()
        points = torch.as_tensor(np.concatenate([uv, np.ones((B, C, 18, 1))], -1), dtype=torch.float32).cuda()
        pmat = torch.as_tensor(P, dtype=torch.float32).cuda()
        tgt = (clean + 5.0 * torch.randn(B, 18, 3, generator=gen).cuda()).float()          # the yardstick's targets: 5 mm of noise
        anchor, info = (tgt, ops_track.ray_information(pmat[:, 0], tgt)) if C == 1 else (None, None)
        views = lambda it: ops_smplfit.fit_smpl_views(points, pmat, layer, reg, init, anchor=anchor, info=info, iters=it)
        joints = lambda it: ops_smplfit.fit_smpl(tgt, ones, layer, reg, init=init, iters=it)
        fns = (('views: one linearisation', lambda: ops_smplfit.linearise_smpl_views(points, pmat, layer, reg, init, anchor=anchor, info=info)),
               ('views: start (max_iters 0)', lambda: views(0)),
               ('views: max_iters 1', lambda: views(1)),
               ('views: max_iters 30', lambda: views(30)),
               ('joints: start (max_iters 0)', lambda: joints(0)),
               ('joints: max_iters 1', lambda: joints(1)),
               ('joints: max_iters 30', lambda: joints(30)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _, f in fns:
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
        say('%s (%d vertices visited), C = %d%s' % (tag, int((reg != 0).any(0).sum()), C, ' with ray anchors' if C == 1 else ''))
        med = {}
        for name, _ in fns:
            t = np.array(times[name])
            med[name] = float(np.median(t))
            say('  %-28s %10.3f  (%.3f .. %.3f)' % (name, med[name], t.min(), t.max()))
        new, old = views(30), joints(30)
        say('  one full trial (max_iters 1 - start): views %.3f ms, joints %.3f ms' % (
            med['views: max_iters 1'] - med['views: start (max_iters 0)'], med['joints: max_iters 1'] - med['joints: start (max_iters 0)']))
        say('  views: trials %s, cost %.4g -> %.4g px^2; joints: trials %s, cost %.4g -> %.4g mm^2' % (
            new['iters'].tolist(), new['cost'][:, 0].sum().item(), new['cost'][:, 1].sum().item(),
            old['iters'].tolist(), old['cost'][:, 0].sum().item(), old['cost'][:, 1].sum().item()))
if opt['--out']:
    with open(opt['--out'], 'w') as f:
        f.write('\n'.join(lines) + '\n')
