#!/usr/bin/env python3
"""xas_smpl_fit_tracks_smooth at (S, T, V) = (8, 256, 6890) on the synthetic body of tests/_smplfit_inputs.py, with its dense H36M
regressor and with one that keeps 10 % of the columns: time per call of ops_smplfit (host preparation, workspace and all the
launches) of one linearisation with its trial solve (linearise_smpl_tracks_smooth), of the start alone (max_iters 0), of one
trial (max_iters 1) and of 30 trials, and IN THE SAME RUN of xas_smpl_fit_tracks (start, 1 and 30 trials) on the same samples, the
yardstick.  Every track has one planted beta and planted parameters that are a quadratic in the frame number; targets are the
model's own joints plus 5 mm of noise, the start is the default one; the samples lie shuffled in N.  Per figure: 1 warm-up call,
then 3 windows of `--reps` calls with device events around each window, the variants alternating window by window; the median
window is the figure, min and max the spread.  The per-track recurrence is not timed by itself: the line `recurrence` is the
difference of the two trials divided by T, a LOWER estimate (the yardstick's trial holds a per-frame elimination this one lacks).
usage: bench_smpl_fit_smooth.py [--out FILE] [--reps N] [--tracks S] [--frames T]"""
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
rng = np.random.Generator(np.random.PCG64(5))
base = si.random_params(S, 3, pose_amp=0.3)[:, None]                      # [S,1,85]
scale = np.concatenate([np.full(3, 0.01), np.full(3, 5.0), np.full(69, 0.003), np.zeros(10)])
tt = np.arange(T, dtype=np.float64)[None, :, None]
x = base + scale * rng.standard_normal((S, 1, 85)) * tt + 0.5 * (0.02 * scale) * rng.standard_normal((S, 1, 85)) * tt ** 2
x = torch.as_tensor(x.reshape(N, 85), dtype=torch.float32)
order = torch.randperm(N, generator=torch.Generator().manual_seed(2))
x = x[order]
track, frame = (order // T).numpy(), (order % T).numpy()
planted = {'pose': torch.cat([x[:, :3], x[:, 6:75]], 1).cuda(), 'trans': x[:, 3:6].contiguous().cuda(), 'betas': x[:, 75:].contiguous().cuda()}
ones = torch.ones(N, 18, device='cuda')
noise = 5.0 * torch.randn(N, 18, 3, generator=torch.Generator().manual_seed(4)).cuda()
say('MI355X, xas_smpl_fit_tracks_smooth at (S, T, V) = (%d, %d, %d), N = %d samples shuffled, synthetic body, priors %g / %g, weights %g / '
    '%g; workspace %.1f MB (xas_smpl_fit_tracks: %.1f MB).' % (S, T, V, N, ops_smplfit.POSE_PRIOR, ops_smplfit.SHAPE_PRIOR,
                                                               ops_smplfit.FIT_SMOOTH_ROT, ops_smplfit.FIT_SMOOTH_TRANS,
                                                               ops_smplfit.tracks_smooth_workspace_bytes(N, V, S) / 1e6,
                                                               ops_smplfit.tracks_workspace_bytes(N, V, S) / 1e6))
say('%d windows of %d calls per variant after 1 warm-up call, device events around each window, variants alternating; ms per call of '
    'ops_smplfit (host preparation + all launches): median window (min .. max)' % (WINDOWS, reps))
for tag, reg in (('dense regressor', dense), ('10 % of the columns', sparse)):
    tgt = (ops_smplfit.fit_smpl(torch.zeros(N, 18, 3, device='cuda'), ones, layer, reg, init=planted, iters=0)['joints'] + noise).float()
    init = ops_smplfit.default_init(tgt, ones, layer, reg)
    smooth = lambda it: ops_smplfit.fit_smpl_tracks_smooth(tgt, ones, track, frame, layer, reg, init=init, iters=it)
    tracks = lambda it: ops_smplfit.fit_smpl_tracks(tgt, ones, track, frame, layer, reg, init=init, iters=it)
    fns = (('smooth: one linearisation', lambda: ops_smplfit.linearise_smpl_tracks_smooth(tgt, ones, track, frame, layer, reg, init=init)),
           ('smooth: start (max_iters 0)', lambda: smooth(0)),
           ('smooth: max_iters 1', lambda: smooth(1)),
           ('smooth: max_iters 30', lambda: smooth(30)),
           ('tracks: start (max_iters 0)', lambda: tracks(0)),
           ('tracks: max_iters 1', lambda: tracks(1)),
           ('tracks: max_iters 30', lambda: tracks(30)))
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
    new, old = smooth(30), tracks(30)
    t_new = med['smooth: max_iters 1'] - med['smooth: start (max_iters 0)']
    t_old = med['tracks: max_iters 1'] - med['tracks: start (max_iters 0)']
    say('  one full trial (max_iters 1 - start): smooth %.3f ms, tracks %.3f ms' % (t_new, t_old))
    say('  recurrence (difference of the two trials / T, a lower estimate): %.1f us per frame' % (1e3 * (t_new - t_old) / T))
    say('  smooth: trials %s, status %s, cost %.4g -> %.4g; tracks: trials %s, status %s, cost %.4g -> %.4g' % (
        new['track_trials'].tolist(), new['track_status'].tolist(), new['track_cost'][:, 0].sum().item(), new['track_cost'][:, 1].sum().item(),
        old['track_trials'].tolist(), old['track_status'].tolist(), old['track_cost'][:, 0].sum().item(), old['track_cost'][:, 1].sum().item()))
if opt['--out']:
    with open(opt['--out'], 'w') as f:
        f.write('\n'.join(lines) + '\n')
