#!/usr/bin/env python3
"""xas_calibrate_bundle (30 trials) and xas_calibrate_linearise at (N, V, K, R) = (4096, 4, 18, 2), with xas_triangulate_refine on
the same points in the same run as the yardstick: time per call over the C ABI, buffers allocated once, device events around
back-to-back calls, median (min - max) over alternating rounds.  Inputs: the seeded ring rigs of tests/_calib_inputs.py (1 px of
noise, cameras bumped by 0.3 degrees and 5 mm), init from the device DLT.
usage: bench_calib.py [N] [--rounds R]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from xas_amd._lib import call, ptr, query
import _calib_inputs as ci
argv = sys.argv[1:]
rounds = 5
if '--rounds' in argv:
    i = argv.index('--rounds')
    rounds = int(argv[i + 1])
    del argv[i:i + 2]
N, V, K, R, ITERS = int(argv[0]) if argv else 4096, 4, 18, 2, 30
rng = np.random.default_rng(11)
start = [0, N // 2 + N // 8, N]                                                   # two rigs of unequal size
pts, P = np.zeros((N, V, K, 3), np.float32), np.zeros((N, V, 3, 4), np.float32)
truth = rng.uniform(-1000, 1000, size=(N, K, 3))
for r in range(R):
    Ks, Rs, ts = ci.ring_cameras(V, rng)
    Pt, Pb = ci.pmats(Ks, Rs, ts), ci.pmats(Ks, *ci.bump(Rs, ts, rng, 0.3, 5.0))
    s = slice(start[r], start[r + 1])
    h = np.einsum('vij,nkj->nvki', Pt, np.concatenate([truth[s], np.ones((start[r + 1] - start[r], K, 1))], -1))
    pts[s, ..., :2] = h[..., :2] / h[..., 2:] + rng.normal(size=h[..., :2].shape)
    pts[s, ..., 2] = 1.0
    P[s] = Pb
pts, P = torch.from_numpy(pts).cuda(), torch.from_numpy(P).cuda()
init, out = torch.empty(N, K, 4, device='cuda'), torch.empty(N, K, 4, device='cuda')
call('xas_triangulate_dlt', ptr(pts), ptr(P), N, V, K, ptr(init))
table = (ctypes.c_int * (R + 1))(*start)
ws = torch.empty(query('xas_calibrate_workspace_bytes', N, V, K, R), device='cuda', dtype=torch.uint8)
f64 = lambda *s: torch.zeros(*s, device='cuda', dtype=torch.float64)
delta, cost, rms, zero = f64(R, V, 6), f64(R, 2), f64(R, 2), f64(R, V, 6)
status, trials = torch.empty(R, device='cuda', dtype=torch.uint8), torch.empty(R, 2, device='cuda', dtype=torch.int32)
n = 6 * (V - 1)
S, b, C = f64(R, n, n), f64(R, n), f64(R)
resid = torch.empty(N, K, 2, device='cuda')
free = ((1 << V) - 1) & ~1


def bundle():
    delta.zero_()
    call('xas_calibrate_bundle', ptr(pts), ptr(P), ptr(init), None, table, N, V, K, R, free, 0, 0.0, 1e4, 1e-2, ITERS, ptr(delta),
         ptr(out), ptr(cost), ptr(rms), None, ptr(status), ptr(trials), ptr(ws))


lin = lambda: call('xas_calibrate_linearise', ptr(pts), ptr(P), ptr(init), None, table, N, V, K, R, free, 0, 0.0, 1e4, 1e-2, 1e-3,
                   ptr(zero), ptr(S), ptr(b), ptr(C), ptr(ws))
refine = lambda: call('xas_triangulate_refine', ptr(pts), ptr(P), ptr(init), None, N, V, K, 0, 0.0, 20, ptr(out), ptr(resid), None, None)
jobs = (('calibrate_bundle (30 trials enqueued)', bundle, 10), ('calibrate_linearise', lin, 50), ('triangulate_refine (20 trials)', refine, 100))
a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
times = {name: [] for name, _, _ in jobs}
for name, f, reps in jobs:
    for _ in range(3):
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
print('N=%d V=%d K=%d R=%d (rigs of %d and %d samples, %d points), %d alternating rounds, device events around back-to-back calls'
      % (N, V, K, R, start[1], N - start[1], N * K, rounds))
for name, _, reps in jobs:
    t = sorted(times[name])
    print('%-40s %10.1f us per call, median (%.1f - %.1f), %d calls per round' % (name, t[len(t) // 2], t[0], t[-1], reps))
print('bundle: trials made / accepted per rig %s, status %s, RMS %s -> %s px' % (
    trials.tolist(), status.tolist(), ['%.3f' % v for v in rms[:, 0].tolist()], ['%.3f' % v for v in rms[:, 1].tolist()]))
