#!/usr/bin/env python3
"""xas_track_smooth (30 trials), with 1 trial, and xas_track_linearise at (S, T, V, K) = (60, 2048, 4, 18), with
xas_triangulate_refine on the same points in the same run as the yardstick: time per call over the C ABI, buffers allocated once,
device events around back-to-back calls, median (min - max) over alternating rounds.  Inputs: the seeded tracks of
tests/_track_inputs.py (one ring rig per track, sinusoidal joints, 2 px of noise, consecutive frames), init from the device DLT.
usage: bench_track_smooth.py [S] [T] [--rounds R]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from xas_amd._lib import call, ptr, query
import _refine_inputs as ri
import _track_inputs as ti
argv = sys.argv[1:]
rounds = 3
if '--rounds' in argv:
    i = argv.index('--rounds')
    rounds = int(argv[i + 1])
    del argv[i:i + 2]
S, T = (int(argv[0]) if argv else 60), (int(argv[1]) if len(argv) > 1 else 2048)
V, K, ITERS, ACC = 4, 18, 30, ti.ACC_W
N = S * T
rng = np.random.Generator(np.random.PCG64(7))
pts, P = np.zeros((N, V, K, 3), np.float32), np.zeros((N, V, 3, 4), np.float32)
fr = np.arange(T)
for s in range(S):
    _, Ps, _ = ri.ring_rig(1, V, K, 7000 + s)
    Pt = np.repeat(Ps, T, 0)
    world = ti.trajectory(fr, K, rng)
    pts[s * T:(s + 1) * T], P[s * T:(s + 1) * T], _ = ri.noisy((ri.project(Pt, world), Pt, world), 7500 + s)
pts, P = torch.from_numpy(pts).cuda(), torch.from_numpy(P).cuda()
frame = torch.from_numpy(np.tile(fr, S).astype(np.int32)).cuda()
init, out, ref = (torch.empty(N, K, 4, device='cuda') for _ in range(3))
call('xas_triangulate_dlt', ptr(pts), ptr(P), N, V, K, ptr(init))
table = (ctypes.c_int * (S + 1))(*[s * T for s in range(S + 1)])
nbytes = query('xas_track_smooth_workspace_bytes', N, K)
ws = torch.empty(nbytes, device='cuda', dtype=torch.uint8)
status, resid = torch.empty(N, K, device='cuda', dtype=torch.uint8), torch.empty(N, K, 2, device='cuda')
tstat, cost = torch.empty(S, K, device='cuda', dtype=torch.uint8), torch.zeros(S, K, 2, device='cuda', dtype=torch.float64)
trials = torch.empty(S, K, device='cuda', dtype=torch.int32)
band, g = torch.empty(N, K, 27, device='cuda', dtype=torch.float64), torch.empty(N, K, 3, device='cuda', dtype=torch.float64)
C = torch.empty(S, K, device='cuda', dtype=torch.float64)
smooth = lambda it: call('xas_track_smooth', ptr(pts), ptr(P), ptr(init), None, table, ptr(frame), N, V, K, S, 0, 0.0, ACC, it,
                         ptr(out), ptr(status), ptr(resid), ptr(tstat), ptr(cost), ptr(trials), ptr(ws))
lin = lambda: call('xas_track_linearise', ptr(pts), ptr(P), ptr(init), None, table, ptr(frame), N, V, K, S, 0, 0.0, ACC, 1e-3,
                   ptr(band), ptr(g), ptr(C), ptr(ws))
refine = lambda: call('xas_triangulate_refine', ptr(pts), ptr(P), ptr(init), None, N, V, K, 0, 0.0, 20, ptr(ref), ptr(resid), None, None)
jobs = (('track_smooth (up to 30 trials)', lambda: smooth(ITERS), 3), ('track_smooth (1 trial)', lambda: smooth(1), 5),
        ('track_linearise', lin, 10), ('triangulate_refine (20 trials)', refine, 20))
a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
print('S=%d T=%d V=%d K=%d (%d samples, %d waves, workspace %.0f MB), %d alternating rounds, device events around back-to-back calls'
      % (S, T, V, K, N, S * K, nbytes / 1e6, rounds), flush=True)
a.record(); smooth(ITERS); e.record()
torch.cuda.synchronize()
print('first call of track_smooth: %.1f ms' % a.elapsed_time(e), flush=True)
made = trials.cpu().numpy()
smoothed = out.clone()
times = {name: [] for name, _, _ in jobs}
for name, f, reps in jobs:
    f()
torch.cuda.synchronize()
for _ in range(rounds):                                                           # alternating: every round times each in turn
    for name, f, reps in jobs:
        a.record()
        for _ in range(reps):
            f()
        e.record()
        torch.cuda.synchronize()
        times[name].append(a.elapsed_time(e) / reps * 1e3)
for name, _, reps in jobs:
    t = sorted(times[name])
    print('%-40s %12.1f us per call, median (%.1f - %.1f), %d calls per round' % (name, t[len(t) // 2], t[0], t[-1], reps))
refine()
move = (smoothed[..., :3] - ref[..., :3]).norm(dim=-1)
print('smooth: trials made per (track, joint) %d - %d (mean %.1f), status counts %s, moved %.2f mm from the per-frame points on average'
      % (made.min(), made.max(), made.mean(), np.bincount(tstat.cpu().numpy().reshape(-1), minlength=3).tolist(), float(move.mean())))
