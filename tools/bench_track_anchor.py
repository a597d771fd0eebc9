#!/usr/bin/env python3
"""xas_track_anchor_smooth (30 trials), with 1 trial, and xas_track_anchor_linearise at (S, T, V, K) = (60, 2048, 1, 18) with ray
anchors, and xas_track_smooth on tracks of the same size (its own V = 4) in the same run as the yardstick: time per call over the
C ABI, buffers allocated once, device events around back-to-back calls, median (min - max) over alternating rounds.  Inputs: the
seeded tracks of tests/_track_inputs.py (one ring rig per track, sinusoidal joints, 2 px of noise, consecutive frames); the
anchors are the true points moved 30 mm (sigma) along camera 0's ray, information TRACK_DEPTH_W along it
(tests/_track_anchor_inputs.ray_info), the start is the anchor; track_smooth starts from the device DLT.
usage: bench_track_anchor.py [S] [T] [--rounds R] [--out FILE]   (FILE: profiles/track_anchor_timing.txt)"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from xas_amd._lib import call, ptr, query
from xas_amd.ops_track import TRACK_ANCHOR_HUBER, TRACK_DEPTH_W
import _refine_inputs as ri
import _track_anchor_inputs as ai
import _track_inputs as ti
argv = sys.argv[1:]
rounds, path = 3, os.path.join(ROOT, 'profiles', 'track_anchor_timing.txt')
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
ray = truth.astype(np.float64) - ai.centres(P[:, :1])[:, 0][:, None]
ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
anchor = (truth + ray * rng.normal(0.0, 30.0, (N, K, 1))).astype(np.float32)
info = ai.ray_info(P[:, 0], anchor, TRACK_DEPTH_W)
pts1, P1 = torch.from_numpy(np.ascontiguousarray(pts[:, :1])).cuda(), torch.from_numpy(np.ascontiguousarray(P[:, :1])).cuda()
pts, P = torch.from_numpy(pts).cuda(), torch.from_numpy(P).cuda()
anchor, info = torch.from_numpy(anchor).cuda().contiguous(), torch.from_numpy(info).cuda().contiguous()
init1 = torch.cat([anchor, torch.ones_like(anchor[..., :1])], -1).contiguous()
frame = torch.from_numpy(np.tile(fr, S).astype(np.int32)).cuda()
init, out, out1 = (torch.empty(N, K, 4, device='cuda') for _ in range(3))
call('xas_triangulate_dlt', ptr(pts), ptr(P), N, V, K, ptr(init))
table = (ctypes.c_int * (S + 1))(*[s * T for s in range(S + 1)])
nbytes = query('xas_track_anchor_workspace_bytes', N, K)
ws = torch.empty(nbytes, device='cuda', dtype=torch.uint8)
status, resid = torch.empty(N, K, device='cuda', dtype=torch.uint8), torch.empty(N, K, 2, device='cuda')
tstat, cost = torch.empty(S, K, device='cuda', dtype=torch.uint8), torch.zeros(S, K, 2, device='cuda', dtype=torch.float64)
trials, trials1 = (torch.empty(S, K, device='cuda', dtype=torch.int32) for _ in range(2))
band, g = torch.empty(N, K, 27, device='cuda', dtype=torch.float64), torch.empty(N, K, 3, device='cuda', dtype=torch.float64)
C = torch.empty(S, K, device='cuda', dtype=torch.float64)
anchored = lambda it: call('xas_track_anchor_smooth', ptr(pts1), ptr(P1), ptr(init1), None, ptr(anchor), ptr(info), table, ptr(frame),
                           N, 1, K, S, 0, 0.0, TRACK_ANCHOR_HUBER, ACC, it, ptr(out1), ptr(status), ptr(resid), ptr(tstat), ptr(cost),
                           ptr(trials1), ptr(ws))
lin = lambda: call('xas_track_anchor_linearise', ptr(pts1), ptr(P1), ptr(init1), None, ptr(anchor), ptr(info), table, ptr(frame),
                   N, 1, K, S, 0, 0.0, TRACK_ANCHOR_HUBER, ACC, 1e-3, ptr(band), ptr(g), ptr(C), ptr(ws))
smooth = lambda it: call('xas_track_smooth', ptr(pts), ptr(P), ptr(init), None, table, ptr(frame), N, V, K, S, 0, 0.0, ACC, it,
                         ptr(out), ptr(status), ptr(resid), ptr(tstat), ptr(cost), ptr(trials), ptr(ws))
jobs = (('track_anchor_smooth V=1 (up to 30 trials)', lambda: anchored(ITERS), 3), ('track_anchor_smooth V=1 (1 trial)', lambda: anchored(1), 5),
        ('track_anchor_linearise V=1', lin, 10), ('track_smooth V=4 (up to 30 trials)', lambda: smooth(ITERS), 3),
        ('track_smooth V=4 (1 trial)', lambda: smooth(1), 5))
a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
lines = ['S=%d T=%d K=%d (%d samples, %d waves, workspace %.0f MB), %d alternating rounds, device events around back-to-back calls'
         % (S, T, K, N, S * K, nbytes / 1e6, rounds)]
print(lines[0], flush=True)
anchored(ITERS); smooth(ITERS)
torch.cuda.synchronize()
made1, made = trials1.cpu().numpy(), trials.cpu().numpy()
smoothed = out1.clone()
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
    lines.append('%-44s %12.1f us per call, median (%.1f - %.1f), %d calls per round' % (name, t[len(t) // 2], t[0], t[-1], reps))
truth = torch.from_numpy(truth).cuda()
lines.append('anchored: trials made per (track, joint) %d - %d (mean %.1f); track_smooth: %d - %d (mean %.1f)'
             % (made1.min(), made1.max(), made1.mean(), made.min(), made.max(), made.mean()))
lines.append('anchored: mean distance to the true points %.2f mm, the anchors\' %.2f mm' % (
    float((smoothed[..., :3] - truth).norm(dim=-1).mean()), float((anchor - truth).norm(dim=-1).mean())))
for l in lines[1:]:
    print(l)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
