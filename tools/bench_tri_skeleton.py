#!/usr/bin/env python3
"""xas_triangulate_skeleton beside xas_triangulate_refine (--tri-refine lm) and xas_triangulate_dlt at evaluation's shape
(V=4, K=18, the shipped limb table, L=4; max_iter=20; sym_w=0.1; 2 px of pixel noise on a ring of cameras, the noisy case of
tests/test_gpu_tri_skeleton.py scaled up) at B=32 and B=512: time per call over the C ABI, outputs allocated once.  Per kernel
and batch: 20 warm-up calls, then 7 windows of 200 calls back to back with device events around each window, the three kernels
alternating window by window; the median window is the figure, min and max the spread.
usage: bench_tri_skeleton.py [--out FILE] [--reps N]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from xas_amd import ops_eval
from xas_amd._lib import call, ptr
from _refine_inputs import noisy, project, ring_rig      # the seeded rigs of the tests: numpy only
argv = sys.argv[1:]
opt = {'--out': None, '--reps': '200'}
for flag in list(opt):
    if flag in argv:
        i = argv.index(flag)
        opt[flag] = argv[i + 1]
        del argv[i:i + 2]
reps, V, K, WINDOWS = int(opt['--reps']), 4, 18, 7
limbs = ops_eval.SYM_LIMBS
table = (ctypes.c_int * (4 * len(limbs)))(*[j for row in limbs for j in row])
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


say('MI355X, V=%d K=%d L=%d max_iter=20 sym_w=%g, unweighted, no Huber; resid and status written (skeleton: also sym and cost).' % (
    V, K, len(limbs), ops_eval.TRI_SYM_W))
say('%d windows of %d calls back to back per kernel after 20 warm-up calls, device events around each window, kernels alternating; '
    'us per call: median window (min .. max)' % (WINDOWS, reps))
for B in (32, 512):
    _, P, world = ring_rig(B, V, K, 7)
    for dst, src in ((4, 1), (5, 2), (6, 3), (11, 14), (12, 15), (13, 16)):      # the planted skeleton is left/right symmetric
        world[:, dst] = world[:, src] * np.array([-1.0, 1.0, 1.0], np.float32)
    pts, P, _ = noisy((project(P, world), P, world), 8)
    pts, P = torch.from_numpy(pts).cuda(), torch.from_numpy(P).cuda()
    init, out = torch.empty(B, K, 4, device='cuda'), torch.empty(B, K, 4, device='cuda')
    resid, status = torch.empty(B, K, 2, device='cuda'), torch.empty(B, K, device='cuda', dtype=torch.uint8)
    sym, cost = torch.empty(B, len(limbs), 2, device='cuda'), torch.empty(B, 2, device='cuda')
    fns = (('triangulate_dlt', lambda: call('xas_triangulate_dlt', ptr(pts), ptr(P), B, V, K, ptr(init))),
           ('triangulate_refine', lambda: call('xas_triangulate_refine', ptr(pts), ptr(P), ptr(init), None, B, V, K, 0, 0.0, 20, ptr(out),
                                               ptr(resid), None, ptr(status))),
           ('triangulate_skeleton', lambda: call('xas_triangulate_skeleton', ptr(pts), ptr(P), ptr(init), None, table, B, V, K, len(limbs),
                                                 0, 0.0, ops_eval.TRI_SYM_W, 20, ptr(out), ptr(resid), ptr(sym), ptr(cost), ptr(status))))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _, f in fns:
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in fns}
    for _ in range(WINDOWS):
        for name, f in fns:
            a.record()
            for _ in range(reps):
                f()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / reps * 1e3)
    say('B=%d (%d joints, %d waves for the skeleton kernel)' % (B, B * K, B))
    for name, _ in fns:
        t = np.array(times[name])
        say('  %-21s %8.2f  (%.2f .. %.2f)' % (name, np.median(t), t.min(), t.max()))
    fns[0][1]()                                            # leave the skeleton kernel's own outputs in the buffers
    fns[2][1]()
    st = status.cpu().numpy()
    say('  skeleton: %d samples stopped on the step rule, %d out of trials; RMS residual %.3f -> %.3f px, mean |limb a| - |limb b| '
        '%.3f -> %.3f mm, cost %.1f -> %.1f' % ((st[:, 0] == 0).sum(), (st[:, 0] == 1).sum(), float(resid[..., 0].mean()),
                                                float(resid[..., 1].mean()), float(sym[..., 0].abs().mean()), float(sym[..., 1].abs().mean()),
                                                float(cost[:, 0].mean()), float(cost[:, 1].mean())))
if opt['--out']:
    with open(opt['--out'], 'w') as f:
        f.write('\n'.join(lines) + '\n')
