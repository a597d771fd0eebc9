#!/usr/bin/env python3
"""xas_triangulate_refine beside xas_triangulate_dlt at evaluation's shape (B=32, V=4, K=18; max_iter=20; 2 px of pixel noise on a
ring of cameras, the noisy case of tests/test_gpu_tri_refine.py scaled up): time per call over the C ABI, outputs allocated once.
usage: bench_tri_refine.py [B] [--reps N]     under `rocprofv3 --kernel-trace --stats -- python ...` the kernels' own times"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import torch
from xas_amd._lib import call, ptr
from _refine_inputs import noisy, ring_rig      # the seeded rigs of the tests: numpy only
argv = sys.argv[1:]
reps = 200
if '--reps' in argv:
    i = argv.index('--reps')
    reps = int(argv[i + 1])
    del argv[i:i + 2]
B, V, K = int(argv[0]) if argv else 32, 4, 18
pts, P, _ = noisy(ring_rig(B, V, K, 7), 8)
pts, P = torch.from_numpy(pts).cuda(), torch.from_numpy(P).cuda()
init, out = torch.empty(B, K, 4, device='cuda'), torch.empty(B, K, 4, device='cuda')
resid, status = torch.empty(B, K, 2, device='cuda'), torch.empty(B, K, device='cuda', dtype=torch.uint8)
dlt = lambda: call('xas_triangulate_dlt', ptr(pts), ptr(P), B, V, K, ptr(init))
lm = lambda: call('xas_triangulate_refine', ptr(pts), ptr(P), ptr(init), None, B, V, K, 0, 0.0, 20, ptr(out), ptr(resid), None, ptr(status))
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
print('B=%d V=%d K=%d max_iter=20, %d calls back to back after 20 warm-up calls, events around the loop' % (B, V, K, reps))
for name, f in (('triangulate_dlt', dlt), ('triangulate_refine', lm), ('triangulate_dlt', dlt), ('triangulate_refine', lm)):
    for _ in range(20):
        f()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    print('%-20s %.2f us per call' % (name, a.elapsed_time(b) / reps * 1e3))
st = status.cpu().numpy()
print('status: %d stopped on the step rule, %d out of trials, %d passed through; RMS residual %.3f -> %.3f px' % (
    (st == 0).sum(), (st == 1).sum(), (st == 2).sum(), float(resid[..., 0].mean()), float(resid[..., 1].mean())))
