#!/usr/bin/env python3
"""xas_track_resolve at (S, T, K, Hy) = (60, 2048, 18, 3) with the shipped pairs (12 units per track), and at Hy = 5, with
xas_track_smooth (1 trial and up to 30) on tracks of the same S, T and K in the same run as the yardstick: time per call over
the C ABI, buffers allocated once, device events around back-to-back calls, median (min - max) over alternating rounds.
Inputs: the planted scene of tests/_resolve_track_inputs.py; for the yardstick the seeded tracks of tools/bench_track_smooth.py.
usage: bench_track_resolve.py [S] [T] [--rounds R]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from xas_amd._lib import call, ptr, query
import _refine_inputs as fi
import _resolve_track_inputs as ri
import _track_inputs as ti
argv = sys.argv[1:]
rounds = 3
if '--rounds' in argv:
    i = argv.index('--rounds')
    rounds = int(argv[i + 1])
    del argv[i:i + 2]
S, T = (int(argv[0]) if argv else 60), (int(argv[1]) if len(argv) > 1 else 2048)
K, V = 18, 4
N = S * T
table = (ctypes.c_int * (S + 1))(*[s * T for s in range(S + 1)])
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def resolve_job(Hy):
    c = ri.scene(70 + Hy, [T] * S, K=K, Hy=Hy)
    kps, world, frame = dev(c['kps']), dev(c['world']), dev(c['frame'])
    perm = (ctypes.c_int * K)(*c['perm'])
    nbytes = query('xas_track_resolve_workspace_bytes', N, Hy, K)
    ws = torch.empty(nbytes, device='cuda', dtype=torch.uint8)
    sel = torch.empty(N, K, 3, device='cuda')
    hyp, swap, status = (torch.empty(N, K, device='cuda', dtype=torch.uint8) for _ in range(3))
    cost = torch.empty(S, K, device='cuda', dtype=torch.float64)
    f = lambda: call('xas_track_resolve', ptr(kps), ptr(world), None, perm, table, ptr(frame), N, Hy, K, S, c['vel_w'], c['hyp_w'],
                     c['swap_w'], ptr(sel), ptr(hyp), ptr(swap), ptr(status), ptr(cost), ptr(ws))
    f()
    torch.cuda.synchronize()
    right = (hyp.cpu().numpy() == c['truth']['hyp']) & (swap.cpu().numpy() == c['truth']['swap'])
    units = sum(1 for k in range(K) if k <= c['perm'][k])
    print('track_resolve Hy=%d: %d waves (%d units per track, %d states per pair), workspace %.0f MB, in %.0f MB; labels as planted on %.4f of the joints'
          % (Hy, S * units, units, 2 * Hy * Hy, nbytes / 1e6, (kps.numel() + world.numel()) * 4 / 1e6, right.mean()), flush=True)
    return f


def smooth_job():
    rng = np.random.Generator(np.random.PCG64(7))
    pts, P = np.zeros((N, V, K, 3), np.float32), np.zeros((N, V, 3, 4), np.float32)
    fr = np.arange(T)
    for s in range(S):
        _, Ps, _ = fi.ring_rig(1, V, K, 7000 + s)
        Pt = np.repeat(Ps, T, 0)
        world = ti.trajectory(fr, K, rng)
        pts[s * T:(s + 1) * T], P[s * T:(s + 1) * T], _ = fi.noisy((fi.project(Pt, world), Pt, world), 7500 + s)
    pts, P, frame = dev(pts), dev(P), dev(np.tile(fr, S).astype(np.int32))
    init, out = torch.empty(N, K, 4, device='cuda'), torch.empty(N, K, 4, device='cuda')
    call('xas_triangulate_dlt', ptr(pts), ptr(P), N, V, K, ptr(init))
    ws = torch.empty(query('xas_track_smooth_workspace_bytes', N, K), device='cuda', dtype=torch.uint8)
    return lambda it: call('xas_track_smooth', ptr(pts), ptr(P), ptr(init), None, table, ptr(frame), N, V, K, S, 0, 0.0, ti.ACC_W, it,
                           ptr(out), None, None, None, None, None, ptr(ws))


print('S=%d T=%d K=%d (%d samples), %d alternating rounds, device events around back-to-back calls' % (S, T, K, N, rounds), flush=True)
r3, r5, smooth = resolve_job(3), resolve_job(5), smooth_job()
jobs = (('track_resolve Hy=3', r3, 5), ('track_resolve Hy=5', r5, 3), ('track_smooth (1 trial), the yardstick', lambda: smooth(1), 5),
        ('track_smooth (up to 30 trials)', lambda: smooth(30), 2))
a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
