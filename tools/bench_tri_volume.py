#!/usr/bin/env python3
"""xas_triangulate_volume (eval.py --tri-volume) beside xas_triangulate_refine (--tri-refine lm) at evaluation's shape:
(B, V, K, D) = (32, 4, 18, 64), G = 16, levels = 2, side 800 mm: time per call over the C ABI, outputs allocated once.  The
cubes are log-Gaussians (sigma 1.5 cells) round every view's cube coordinates of planted joints on the seeded rig of
tests/_volume_inputs.py, built on the device; the start is the planted point moved by 30 mm per axis.  Per kernel: 20 warm-up
calls, then 7 windows of `reps` calls back to back with device events around each window, the kernels alternating window by
window; the median window is the figure, min and max the spread.  The counts beside the times come from the shapes: one
SAMPLE is one voxel looked up in one view (eight logits, four 8-byte loads).
usage: bench_tri_volume.py [--out FILE] [--reps N]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from xas_amd import ops_eval
from xas_amd._lib import call, ptr
import _volume_inputs as vi                              # the seeded rigs of the tests: numpy only
from _refine_inputs import noisy, ring_rig
argv = sys.argv[1:]
opt = {'--out': None, '--reps': '100'}
for flag in list(opt):
    if flag in argv:
        i = argv.index(flag)
        opt[flag] = argv[i + 1]
        del argv[i:i + 2]
reps, WINDOWS = int(opt['--reps']), 7
B, V, K, D, G, LEVELS, SIDE = 32, 4, 18, 64, ops_eval.TRI_VOL_G, ops_eval.TRI_VOL_LEVELS, ops_eval.TRI_VOL_SIDE_MM
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


cams = vi.rig(B, V, 7)
world = vi.planted(B, K, 8, spread_mm=400.0)
coords = torch.from_numpy(vi.cube_coords(cams, world, D).astype(np.float32)).cuda()      # [V,B,K,3] = (w, h, d)
g = torch.arange(D, device='cuda', dtype=torch.float32)
cubes = []
for v in range(V):                                       # [B,H,W,K,D]: the head's NHWC storage
    cw, ch, cd = (coords[v, :, :, n] for n in range(3))
    sq = ((g.view(1, D, 1, 1, 1) - ch.view(B, 1, 1, K, 1)) ** 2 + (g.view(1, 1, D, 1, 1) - cw.view(B, 1, 1, K, 1)) ** 2
          + (g.view(1, 1, 1, 1, D) - cd.view(B, 1, 1, K, 1)) ** 2)
    cubes.append((sq * (-1.0 / (2 * 1.5 ** 2))).reshape(B, D, D, K * D).contiguous())
    del sq
table = (ctypes.c_void_p * V)(*[t.data_ptr() for t in cubes])
cam = [torch.from_numpy(cams[k]).cuda() for k in ('trans_image', 'k_mat', 'pelvis', 'rot_world', 'trans_world')]
init = torch.from_numpy(world + np.float32(30.0)).cuda()
xyz, cov = torch.empty(B, K, 3, device='cuda'), torch.empty(B, K, 6, device='cuda')
status = torch.empty(B, K, device='cuda', dtype=torch.uint8)
pts, P, _ = noisy(ring_rig(B, V, K, 7), 8)
pts, P = torch.from_numpy(pts).cuda(), torch.from_numpy(P).cuda()
init4, out4 = torch.empty(B, K, 4, device='cuda'), torch.empty(B, K, 4, device='cuda')
resid, st4 = torch.empty(B, K, 2, device='cuda'), torch.empty(B, K, device='cuda', dtype=torch.uint8)
call('xas_triangulate_dlt', ptr(pts), ptr(P), B, V, K, ptr(init4))
fns = (('triangulate_refine', lambda: call('xas_triangulate_refine', ptr(pts), ptr(P), ptr(init4), None, B, V, K, 0, 0.0, 20, ptr(out4),
                                           ptr(resid), None, ptr(st4))),
       ('triangulate_volume', lambda: call('xas_triangulate_volume', table, None, *[ptr(t) for t in cam], ptr(init), None, None, B, V, K,
                                           D, G, LEVELS, SIDE, 1.0, 1.0, 256.0, 2000.0, ptr(xyz), ptr(cov), ptr(status))))
say('MI355X, (B, V, K, D) = (%d, %d, %d, %d), G=%d levels=%d side=%g mm, beta=1, out_penalty=1; xyz, cov and status written.' % (
    B, V, K, D, G, LEVELS, SIDE))
say('%d windows of %d calls back to back per kernel after 20 warm-up calls, device events around each window, kernels alternating; '
    'us per call: median window (min .. max)' % (WINDOWS, reps))
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
for name, _ in fns:
    t = np.array(times[name])
    say('  %-21s %8.2f  (%.2f .. %.2f)' % (name, np.median(t), t.min(), t.max()))
t = float(np.median(times['triangulate_volume'])) * 1e-6
samples = B * K * LEVELS * G ** 3 * V
say('  volume: %d workgroups of 256 threads, %.2f M samples per call = %.1f G samples/s; %.0f MB of logits gathered per call (32 B per '
    'sample, before any cache) = %.2f TB/s; %.2f M double-precision exp per call (one per voxel) = %.1f G exp/s' % (
        B * K, samples / 1e6, samples / t / 1e9, samples * 32 / 1e6, samples * 32 / t / 1e12, samples / V / 1e6, samples / V / t / 1e9))
s = status.cpu().numpy()
err = (xyz.cpu().numpy() - world).astype(np.float64)
say('  volume: status 0/1/2/3 on %d/%d/%d/%d joints; fused point %.2f mm (mean) from the planted one, start %.2f mm; sqrt(trace cov) %.1f mm' % (
    (s == 0).sum(), (s == 1).sum(), (s == 2).sum(), (s == 3).sum(), np.linalg.norm(err, axis=-1).mean(), 30.0 * 3 ** 0.5,
    float((cov[..., 0] + cov[..., 3] + cov[..., 5]).sqrt().mean())))
if opt['--out']:
    with open(opt['--out'], 'w') as f:
        f.write('\n'.join(lines) + '\n')
