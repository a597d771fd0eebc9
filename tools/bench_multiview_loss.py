#!/usr/bin/env python3
"""xas_multiview_consistency_fwd / _bwd alone at the training step's shape (B=32, V=4, Hy=3, K=18; 2 px of pixel noise on a ring
of cameras, the noisy case of tests/test_gpu_multiview.py scaled up): time per call over the C ABI, outputs allocated once.  Then
the full training step of a workload without and with loss_config.multiview_loss, interleaved so that both see the same clocks.
usage: bench_multiview_loss.py [B] [--reps N] [--steps N] [--workload NAME]
under `rocprofv3 --kernel-trace --stats -- python ...` the kernels' own times"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'x-as-supervision_amd'), os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from xas_amd._lib import call, ptr
from _refine_inputs import noisy, ring_rig      # the seeded rigs of the tests: numpy only
argv = sys.argv[1:]


def opt(flag, default, kind=int):
    if flag in argv:
        i = argv.index(flag)
        v = kind(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


reps, steps, workload = opt('--reps', 200), opt('--steps', 10), opt('--workload', 'HM36_Multi_SurS1', str)
B, V, Hy, K = int(argv[0]) if argv else 32, 4, 3, 18
from _multiview_inputs import patch_case        # crop affines and hypotheses along the rays, as the tests build them
c = patch_case(noisy(ring_rig(B, V, K, 7), 8), 9)
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
kps, ti, world, P = d(c['kps_xy']), d(c['ti']), d(c['world']), d(c['P'])
reproj, depth, xyz = torch.empty(B, K, device='cuda'), torch.empty(B, K, device='cuda'), torch.empty(B, K, 3, device='cuda')
hsel, status = torch.empty(B, V, K, device='cuda', dtype=torch.int32), torch.empty(B, K, device='cuda', dtype=torch.uint8)
g = torch.ones(B, K, device='cuda')
gk, gw = torch.empty_like(kps), torch.empty_like(world)
fwd = lambda: call('xas_multiview_consistency_fwd', ptr(kps), ptr(ti), ptr(world), ptr(P), None, B, V, Hy, K, 256.0, 0.0, 0,
                   ptr(reproj), ptr(depth), ptr(xyz), ptr(hsel), ptr(status))
bwd = lambda flags: call('xas_multiview_consistency_bwd', ptr(kps), ptr(ti), ptr(world), ptr(P), None, ptr(g), ptr(g), B, V, Hy, K,
                         256.0, 0.0, flags, ptr(gk), ptr(gw))
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
print('B=%d V=%d Hy=%d K=%d, %d calls back to back after 20 warm-up calls, events around the loop' % (B, V, Hy, K, reps))
for name, f in (('fwd', fwd), ('bwd through X', lambda: bwd(0)), ('bwd detached', lambda: bwd(1))) * 2:
    for _ in range(20):
        f()
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    print('%-16s %.2f us per call' % (name, a.elapsed_time(b) / reps * 1e3))
print('status: %d solved, %d passed through; mean reproj %.3f px^2, mean depth %.3f mm^2' % (
    (status == 0).sum(), (status == 2).sum(), float(reproj.mean()), float(depth.mean())))

if steps > 0:
    from xas_amd import engine
    from xas_amd.synthetic import model_config, synthetic_batch
    runs = {}
    for tag, key in (('without the key', None), ('with the key', dict(weight_2d=1e-3, weight_3d=1e-6))):
        cfg = model_config(workload)
        if key is not None:
            cfg['model_params']['loss_config']['multiview_loss'] = key
        torch.manual_seed(1234)
        model, disc, opt_det, opt_disc = engine.prepare_model(cfg)
        model.cuda().train()
        disc.cuda().train()
        runs[tag] = (engine.TrainStep(cfg, model, disc, opt_det, opt_disc), synthetic_batch(B, cfg['model_params']['cam_id_list'],
                                                                                             torch.device('cuda'), seed=100))
    for step, x in runs.values():
        for _ in range(2):
            step(x)
    torch.cuda.synchronize()
    times = {tag: [] for tag in runs}
    for _ in range(steps):                                            # interleaved: A B A B ...
        for tag, (step, x) in runs.items():
            t0 = time.perf_counter()
            step(x)
            torch.cuda.synchronize()
            times[tag].append((time.perf_counter() - t0) * 1e3)
    print('%s B=%d, %d steps each, interleaved, after 2 warm-up steps; wall clock around a synchronised step' % (workload, B, steps))
    for tag, ms in times.items():
        ms = np.array(ms)
        print('step %-16s median %.2f ms, min %.2f, max %.2f' % (tag, np.median(ms), ms.min(), ms.max()))
