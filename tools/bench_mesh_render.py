#!/usr/bin/env python3
"""xas_mesh_render (train.py --pseudo-online) alone at the shipped size: (B, Nv, F, S) = (32, 6890, 13776, 256), the vertex and
face counts of the SMPL template, on a synthetic body: a closed latitude-longitude mesh of exactly that many vertices and faces
(84 x 82 rings), 0.36 x 0.26 x 1.7 m with a sinusoidal bend, turned by another seeded rotation per sample and scaled as a
2000 mm box on a 256-pixel patch.  Time per call over the C ABI, outputs and workspace allocated once: 20 warm-up calls, then 7
windows of `reps` calls back to back with device events around each window; the median window is the figure, min and max the
spread.  Both looks are timed, alternating window by window: white faces with ambient 0.35, and face colours with ambient 1.
The counts beside the times come from the faces' pixel boxes, computed here as the set-up kernel computes them.
usage: bench_mesh_render.py [--out FILE] [--reps N]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from xas_amd._lib import call, ptr, query
import _render_inputs as ri                              # the seeded mesh builders of the tests: numpy only
argv = sys.argv[1:]
opt = {'--out': None, '--reps': '50'}
for flag in list(opt):
    if flag in argv:
        i = argv.index(flag)
        opt[flag] = argv[i + 1]
        del argv[i:i + 2]
reps, WINDOWS = int(opt['--reps']), 7
B, S, TILE = 32, 256, ri.TILE
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


rng = np.random.Generator(np.random.PCG64(17))
v, f = ri._ellipsoid(83, 84, (0.18, 0.13, 0.85))         # metres
Nv, F = len(v), len(f)
assert (Nv, F) == (6890, 13776)
v[:, 0] += 0.12 * np.sin(3.0 * v[:, 2])                 # a bend: the silhouette is no ellipse and faces overlap in depth
verts = []
for b in range(B):
    R = ri._rot(rng)
    R = R if b % 4 else np.eye(3)[[0, 2, 1]] * [1, -1, 1]            # every fourth sample upright, the others anywhere
    p = v @ R.T * 1000.0 / (2000.0 / S)                               # mm -> patch units, depth relative to the pelvis
    verts.append(p + [S / 2 + rng.uniform(-10, 10), S / 2 + rng.uniform(-10, 10), 0.0])
verts = torch.from_numpy(np.stack(verts).astype(np.float32)).cuda()
faces = torch.from_numpy(f).cuda()
rgb = torch.from_numpy(rng.uniform(0.1, 1.0, (F, 3)).astype(np.float32)).cuda()
img, mask = torch.empty(B, 3, S, S, device='cuda'), torch.empty(B, 1, S, S, device='cuda')
zbuf, fid = torch.empty(B, S, S, device='cuda'), torch.empty(B, S, S, device='cuda', dtype=torch.int32)
nbytes = query('xas_mesh_render_workspace_bytes', B, F, S)
ws = torch.empty(nbytes, device='cuda', dtype=torch.uint8)
fns = (('shade (img, mask)', lambda: call('xas_mesh_render', ptr(verts), ptr(faces), None, None, 0.35, 1.0, 0.0, B, Nv, F, S, ptr(img),
                                          ptr(mask), None, None, ptr(ws))),
       ('parts (all outputs)', lambda: call('xas_mesh_render', ptr(verts), ptr(faces), ptr(rgb), None, 1.0, 1.0, 0.0, B, Nv, F, S, ptr(img),
                                            ptr(mask), ptr(zbuf), ptr(fid), ptr(ws))))
say('MI355X, xas_mesh_render at (B, Nv, F, S) = (%d, %d, %d, %d), synthetic closed body mesh, workspace %.1f MB.' % (B, Nv, F, S, nbytes / 1e6))
say('%d windows of %d calls back to back per look after 20 warm-up calls, device events around each window, looks alternating; '
    'us per call (set-up + raster launch): median window (min .. max)' % (WINDOWS, reps))
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _, fn in fns:
    for _ in range(20):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in fns}
for _ in range(WINDOWS):
    for name, fn in fns:
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times[name].append(a.elapsed_time(b) / reps * 1e3)
for name, _ in fns:
    t = np.array(times[name])
    say('  %-21s %8.2f  (%.2f .. %.2f)' % (name, np.median(t), t.min(), t.max()))
# the faces' pixel boxes as the set-up kernel forms them -> tiles met per face
tri = verts[:, faces.long()]                             # [B,F,3,3]
lo = tri[..., :2].amin(2).ceil().clamp(min=0)
hi = tri[..., :2].amax(2).floor().clamp(max=S - 1)
live = (lo <= hi).all(-1)
span = ((hi / TILE).floor() - (lo / TILE).floor() + 1).clamp(min=0)
pairs = int((span[..., 0] * span[..., 1] * live).sum())
tiles = B * (S // TILE) ** 2
t = float(np.median(times['shade (img, mask)'])) * 1e-6
say('  raster: %d workgroups of 256 threads (one per sample and %dx%d tile) after %d set-up workgroups; %d of %d faces have a pixel in '
    'their box; %.1f faces per tile after compaction on average (%d face-tile pairs); per call %.1f MB of boxes scanned (8 B per face '
    'and tile) and %.1f MB of 64-byte records read, before any cache = %.2f TB/s at the shade time' % (
        tiles, TILE, TILE, -(-B * F // 256), int(live.sum()), B * F, pairs / tiles, pairs, tiles * F * 8 / 1e6, pairs * 64 / 1e6,
        (tiles * F * 8 + pairs * 64) / t / 1e12))
say('  result: %.1f %% of the pixels covered; %d distinct faces visible' % (100.0 * float(mask.mean()), int((torch.bincount(fid[fid >= 0].flatten() + 0, minlength=F) > 0).sum())))
if opt['--out']:
    with open(opt['--out'], 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
