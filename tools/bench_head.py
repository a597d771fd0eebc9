#!/usr/bin/env python3
"""Soft-argmax head kernels and the heat-map spread kernel alone at the BASELINE size (B=32, K=18, D=H=W=64): achieved HBM GB/s.
usage: bench_head.py [B] [--depth D]      D: cube side (64; e.g. 96 for 384^2 patches - the head's general policy)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd')]
import torch
from xas_amd import ops_head
argv = sys.argv[1:]
D = 64
if '--depth' in argv:
    i = argv.index('--depth')
    D = int(argv[i + 1])
    del argv[i:i + 2]
B = int(argv[0]) if argv else 32
reps = 20
lg = torch.randn(B, D, D, 18 * D, device='cuda').permute(0, 3, 1, 2).requires_grad_(True)   # NHWC storage
g = torch.randn(B, 3, 18, 3, device='cuda')
kps, _, _ = ops_head.softargmax_multi(lg, 18, 3, 15)
kps.backward(g)
torch.cuda.synchronize()
a, b, c = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
tf = tb = 0.0
for _ in range(reps):
    lg.grad = None
    a.record()
    kps, _, _ = ops_head.softargmax_multi(lg, 18, 3, 15)
    b.record()
    kps.backward(g)
    c.record()
    torch.cuda.synchronize()
    tf += a.elapsed_time(b); tb += b.elapsed_time(c)
nbytes = B * 18 * D * D * D * 4
print('D=%d B=%d' % (D, B))
print('head fwd  %.1f us  %.0f GB/s (reads %d MB once)' % (tf / reps * 1e3, nbytes / (tf / reps * 1e-3) / 1e9, nbytes >> 20))
print('head bwd  %.1f us  %.0f GB/s (read + write)' % (tb / reps * 1e3, 2 * nbytes / (tb / reps * 1e-3) / 1e9))
lg = lg.detach()
ops_head.heatmap_spread(lg, 18)
ts = 0.0
for _ in range(reps):
    a.record()
    ops_head.heatmap_spread(lg, 18)
    b.record()
    torch.cuda.synchronize()
    ts += a.elapsed_time(b)
print('head spread  %.1f us  %.0f GB/s (reads %d MB once)' % (ts / reps * 1e3, nbytes / (ts / reps * 1e-3) / 1e9, nbytes >> 20))
