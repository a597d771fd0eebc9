#!/usr/bin/env python3
"""xas_smpl_fit_tracks at (S, T, V) = (8, 256, 6890) on the synthetic body of tests/_smplfit_inputs.py, with its dense H36M
regressor and with one that keeps 10 % of the columns: time per call of ops_smplfit (host preparation, workspace and all the
launches) of one linearisation (linearise_smpl_tracks), of the start alone (max_iters 0), of one full trial (max_iters 1) and of
30 trials, and in the same run of xas_smpl_fit (30 trials) on the same samples.  Every track has one planted beta and a planted
pose per frame (angles within 0.3 rad); targets are the model's own joints plus 5 mm of noise, the start is the default one; the
samples lie shuffled in N.  Per figure: 1 warm-up call, then 3 windows of `--reps` calls with device events around each window,
the variants alternating window by window; the median window is the figure, min and max the spread.
usage: bench_smpl_fit_tracks.py [--out FILE] [--reps N] [--tracks S] [--frames T]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
import _smplfit_inputs as si
from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer
from xas_amd import ops_smplfit
argv = sys.argv[1:]
opt = {'--out': None, '--reps': '1', '--tracks': '8', '--frames': '256'}
for flag in list(opt):
    if flag in argv:
        i = argv.index(flag)
        opt[flag] = argv[i + 1]
        del argv[i:i + 2]
reps, S, T, V, WINDOWS = int(opt['--reps']), int(opt['--tracks']), int(opt['--frames']), 6890, 3
N = S * T
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
x = si.random_params(N, 3, pose_amp=0.3).reshape(S, T, 85)
x[:, :, 75:] = x[:, :1, 75:]                                              # one beta per track
x = torch.as_tensor(x.reshape(N, 85), dtype=torch.float32)
order = torch.randperm(N, generator=torch.Generator().manual_seed(2))
x = x[order]
track, frame = (order // T).numpy(), (order % T).numpy()
planted = {'pose': torch.cat([x[:, :3], x[:, 6:75]], 1).cuda(), 'trans': x[:, 3:6].contiguous().cuda(), 'betas': x[:, 75:].contiguous().cuda()}
ones = torch.ones(N, 18, device='cuda')
noise = 5.0 * torch.randn(N, 18, 3, generator=torch.Generator().manual_seed(4)).cuda()
say('MI355X, xas_smpl_fit_tracks at (S, T, V) = (%d, %d, %d), N = %d samples shuffled, synthetic body, priors %g / %g; workspace %.1f MB '
    '(xas_smpl_fit for as many samples: %.1f MB).' % (S, T, V, N, ops_smplfit.POSE_PRIOR, ops_smplfit.SHAPE_PRIOR,
                                                     ops_smplfit.tracks_workspace_bytes(N, V, S) / 1e6,
                                                     ops_smplfit.query('xas_smpl_fit_workspace_bytes', N, V) / 1e6))
say('%d windows of %d calls per variant after 1 warm-up call, device events around each window, variants alternating; ms per call of '
    'ops_smplfit (host preparation + all launches): median window (min .. max)' % (WINDOWS, reps))
for tag, reg in (('dense regressor', dense), ('10 % of the columns', sparse)):
    tgt = (ops_smplfit.fit_smpl(torch.zeros(N, 18, 3, device='cuda'), ones, layer, reg, init=planted, iters=0)['joints'] + noise).float()
    init = ops_smplfit.default_init(tgt, ones, layer, reg)
    tracks = lambda it: ops_smplfit.fit_smpl_tracks(tgt, ones, track, frame, layer, reg, init=init, iters=it)
    fns = (('tracks: one linearisation', lambda: ops_smplfit.linearise_smpl_tracks(tgt, ones, track, frame, layer, reg, init=init)),
           ('tracks: start (max_iters 0)', lambda: tracks(0)),
           ('tracks: max_iters 1', lambda: tracks(1)),
           ('tracks: max_iters 30', lambda: tracks(30)),
           ('xas_smpl_fit, max_iters 30', lambda: ops_smplfit.fit_smpl(tgt, ones, layer, reg, init=init, iters=30)))
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
    say('%s (%d vertices visited)' % (tag, int((reg != 0).any(0).sum())))
    med = {}
    for name, _ in fns:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        say('  %-28s %10.3f  (%.3f .. %.3f)' % (name, med[name], t.min(), t.max()))
    out, per = tracks(30), fns[4][1]()
    say('  one full trial (max_iters 1 - start): %.3f ms' % (med['tracks: max_iters 1'] - med['tracks: start (max_iters 0)']))
    say('  tracks: trials %s, status %s, cost %.4g -> %.4g; per sample: %.1f trials, status %s, cost %.4g -> %.4g' % (
        out['track_trials'].tolist(), out['track_status'].tolist(), out['track_cost'][:, 0].sum().item(), out['track_cost'][:, 1].sum().item(),
        per['iters'].float().mean().item(), np.bincount(per['status'].cpu().numpy(), minlength=3).tolist(), per['cost'][:, 0].sum().item(),
        per['cost'][:, 1].sum().item()))
if opt['--out']:
    with open(opt['--out'], 'w') as f:
        f.write('\n'.join(lines) + '\n')
