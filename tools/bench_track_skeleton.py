#!/usr/bin/env python3
"""xas_track_skeleton_smooth (30 trials), with 1 trial, and xas_track_skeleton_linearise (one linearisation and one trial solve)
at (S, T, V, K) = (60, 2048, 4, 18) with the 17 bones of the configs' parent_ids, and xas_track_anchor_smooth (no anchors: the
per-joint smoother) on the same tracks in the same run as the baseline: time per call over the C ABI, buffers allocated once,
device events around back-to-back calls, median (min - max) over alternating rounds.  Inputs: the seeded tracks of
tests/_track_inputs.py (one ring rig per track, sinusoidal joints that move independently, so the bones are not rigid, 2 px of
noise, consecutive frames), the start from the device DLT, the lengths ops_track.track_bone_lengths of that start.
usage: bench_track_skeleton.py [S] [T] [--rounds R] [--out FILE]   (FILE: profiles/track_skeleton_timing.txt)"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from xas_amd._lib import call, ptr, query
from xas_amd.ops_track import TRACK_BONE_W, bones_of, track_bone_lengths
import _refine_inputs as ri
import _track_inputs as ti
import _track_skeleton_inputs as si
argv = sys.argv[1:]
rounds, path = 3, os.path.join(ROOT, 'profiles', 'track_skeleton_timing.txt')
for flag in ('--rounds', '--out'):
    if flag in argv:
        i = argv.index(flag)
        if flag == '--rounds':
            rounds = int(argv[i + 1])
        else:
            path = argv[i + 1]
        del argv[i:i + 2]
S, T = (int(argv[0]) if argv else 60), (int(argv[1]) if len(argv) > 1 else 2048)
V, K, ITERS, ACC = 4, 18, 30, ti.ACC_W
N = S * T
rng = np.random.Generator(np.random.PCG64(7))
pts, P, truth = np.zeros((N, V, K, 3), np.float32), np.zeros((N, V, 3, 4), np.float32), np.zeros((N, K, 3), np.float32)
fr = np.arange(T)
for s in range(S):
    _, Ps, _ = ri.ring_rig(1, V, K, 7000 + s)
    Pt = np.repeat(Ps, T, 0)
    world = ti.trajectory(fr, K, rng)
    pts[s * T:(s + 1) * T], P[s * T:(s + 1) * T], _ = ri.noisy((ri.project(Pt, world), Pt, world), 7500 + s)
    truth[s * T:(s + 1) * T] = world
pts, P = torch.from_numpy(pts).cuda(), torch.from_numpy(P).cuda()
frame = torch.from_numpy(np.tile(fr, S).astype(np.int32)).cuda()
init, out, out1 = (torch.empty(N, K, 4, device='cuda') for _ in range(3))
call('xas_triangulate_dlt', ptr(pts), ptr(P), N, V, K, ptr(init))
bones = bones_of(si.PARENTS18)
Bn = len(bones)
host_bones = (ctypes.c_int * (2 * Bn))(*bones.reshape(-1).tolist())
length = track_bone_lengths(init, np.repeat(np.arange(S), T), None, bones)
table = (ctypes.c_int * (S + 1))(*[s * T for s in range(S + 1)])
nbytes, nbytes1 = query('xas_track_skeleton_workspace_bytes', N, K), query('xas_track_anchor_workspace_bytes', N, K)
ws, ws1 = torch.empty(nbytes, device='cuda', dtype=torch.uint8), torch.empty(nbytes1, device='cuda', dtype=torch.uint8)
status, resid = torch.empty(N, K, device='cuda', dtype=torch.uint8), torch.empty(N, K, 2, device='cuda')
bone = torch.empty(N, Bn, 2, device='cuda')
tstat, cost, trials = torch.empty(S, device='cuda', dtype=torch.uint8), torch.zeros(S, 2, device='cuda', dtype=torch.float64), torch.empty(S, device='cuda', dtype=torch.int32)
tstat1, cost1 = torch.empty(S, K, device='cuda', dtype=torch.uint8), torch.zeros(S, K, 2, device='cuda', dtype=torch.float64)
trials1 = torch.empty(S, K, device='cuda', dtype=torch.int32)
g, d = (torch.empty(N, K, 3, device='cuda', dtype=torch.float64) for _ in range(2))
hdiag, hoff = torch.empty(N, 3 * K, 3 * K, device='cuda', dtype=torch.float64), torch.empty(N, 2, device='cuda', dtype=torch.float64)
C = torch.empty(S, device='cuda', dtype=torch.float64)
head = (ptr(pts), ptr(P), ptr(init), None, None, None)
skeleton = lambda it: call('xas_track_skeleton_smooth', *head, host_bones, ptr(length), table, ptr(frame), N, V, K, S, Bn, 0, 0.0, 0.0,
                           ACC, TRACK_BONE_W, it, ptr(out), ptr(status), ptr(resid), ptr(bone), ptr(tstat), ptr(cost), ptr(trials), ptr(ws))
lin = lambda: call('xas_track_skeleton_linearise', *head, host_bones, ptr(length), table, ptr(frame), N, V, K, S, Bn, 0, 0.0, 0.0, ACC,
                   TRACK_BONE_W, 1e-3, ptr(g), ptr(hdiag), ptr(hoff), ptr(d), ptr(C), ptr(ws))
each = lambda it: call('xas_track_anchor_smooth', *head, table, ptr(frame), N, V, K, S, 0, 0.0, 0.0, ACC, it, ptr(out1), ptr(status),
                       ptr(resid), ptr(tstat1), ptr(cost1), ptr(trials1), ptr(ws1))
jobs = (('track_skeleton_smooth (up to 30 trials)', lambda: skeleton(ITERS), 1), ('track_skeleton_smooth (1 trial)', lambda: skeleton(1), 2),
        ('track_skeleton_linearise (1 linearisation, 1 solve)', lin, 2), ('track_anchor_smooth (up to 30 trials)', lambda: each(ITERS), 3),
        ('track_anchor_smooth (1 trial)', lambda: each(1), 5))
a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
lines = ['S=%d T=%d V=%d K=%d Bn=%d (%d samples, %d workgroups of 256; workspace %.0f MB = %d bytes per frame; the per-joint smoother: %d '
         'waves, %.0f MB), %d alternating rounds, device events around back-to-back calls'
         % (S, T, V, K, Bn, N, S, nbytes / 1e6, nbytes // N, S * K, nbytes1 / 1e6, rounds)]
print(lines[0], flush=True)
for name, f, reps in jobs:
    f()
torch.cuda.synchronize()
skeleton(ITERS); each(ITERS)
torch.cuda.synchronize()
made, made1, errs = trials.cpu().numpy(), trials1.cpu().numpy(), bone.clone()
smoothed, smoothed1 = out.clone(), out1.clone()
times = {name: [] for name, _, _ in jobs}
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
    lines.append('%-52s %14.1f us per call, median (%.1f - %.1f), %d calls per round' % (name, t[len(t) // 2], t[0], t[-1], reps))
med = lambda name: sorted(times[name])[len(times[name]) // 2]
lines.append('full call: %.1f x the per-joint smoother; one trial: %.1f x' % (
    med(jobs[0][0]) / med(jobs[3][0]), med(jobs[1][0]) / med(jobs[4][0])))
truth = torch.from_numpy(truth).cuda()
rms = lambda c: float(torch.sqrt((errs[..., c] ** 2).nanmean()))
lines.append('skeleton: trials made per track %d - %d (mean %.1f); per-joint: per (track, joint) %d - %d (mean %.1f)'
             % (made.min(), made.max(), made.mean(), made1.min(), made1.max(), made1.mean()))
lines.append('skeleton: bone length RMS against the track\'s median %.2f -> %.2f mm (these bones are not rigid); mean distance to the true '
             'points %.2f mm, the per-joint smoother\'s %.2f mm' % (rms(0), rms(1), float((smoothed[..., :3] - truth).norm(dim=-1).mean()),
                                                                  float((smoothed1[..., :3] - truth).norm(dim=-1).mean())))
for l in lines[1:]:
    print(l)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
