"""The pass-through rule of the four multi-view solvers is one rule (csrc/multiview.h: point_startable and the fit at the
start): the same (points, pmat, init, views) goes through triangulate_refine, triangulate_skeleton, calibrate_bundle and
track_smooth, and all four refine the same set of points.

The inputs: N = 4 samples that are also the 4 frames of one track and one rig, V = 3, K = 4.  Every way a point can fail the
rule is planted once, and the refined set is written down here from the planting, not read from a kernel:
    (0, 0)  one valid view only (the other two weights are 0), views byte 0
    (2, 0)  a views byte that leaves one view
    (1, 1)  NaN in init, with payloads, one of them negative
    (3, 1)  -inf in init
    (0, 2)  a start behind camera 1
Joint 3 has the zero views byte in every frame (it stands for all valid views: refined); the other ordinary points name their
views, (3, 2) only two of the three.  Every joint keeps at least two ordinary frames, so every track is smoothed.

What "not refined" means differs in one of the four, by include/xas_hip.h: triangulate_refine, triangulate_skeleton and
calibrate_bundle pass such a point through, init bit for bit, and that is asserted on the raw 32-bit patterns, NaN payloads
included.  track_smooth passes a whole track through only where it has fewer than two data frames; in a smoothed track a frame
without data is a GAP frame, which it fills from its neighbours (status 1).  So for track_smooth the test asserts status 0
exactly on the refined set and status 1 on the rest, a finite filled point there, and init's fourth entry bit for bit."""
import numpy as np
import pytest
import torch

import _refine_oracle as ro
from _refine_inputs import noisy, project, ring_rig

pytestmark = pytest.mark.gpu
N, V, K = 4, 3, 4
NOT_REFINED = ((0, 0), (2, 0), (1, 1), (3, 1), (0, 2))


def _f32_bits(pattern):
    return np.array([pattern], np.uint32).view(np.float32)[0]


def _inputs():
    _, P1, world1 = ring_rig(1, V, K, 71)
    P = np.repeat(P1, N, 0)
    world = (world1 + np.arange(N, dtype=np.float32)[:, None, None] * np.array([5.0, -3.0, 2.0], np.float32)).astype(np.float32)
    pts, _, _ = noisy((project(P, world), P, world), 171)
    init = ro.dlt_start(pts, P)
    init[..., :3] += np.array([1.0, -0.5, 0.7], np.float32)               # off the DLT point: a refined point moves
    assert np.isfinite(init).all()
    views = np.full((N, K), 0b111, np.uint8)
    views[:, 3] = 0                                                       # the zero byte: all valid views
    views[3, 2] = 0b101
    pts[0, 1:, 0, 2] = 0.0                                                # (0, 0): one valid view
    views[0, 0] = 0
    views[2, 0] = 0b010                                                   # (2, 0): the byte leaves one view
    init[1, 1, 0] = _f32_bits(0x7fc12345)                                 # (1, 1): NaN with payloads
    init[1, 1, 1] = _f32_bits(0xffc00001)
    init[3, 1, 2] = -np.inf                                               # (3, 1)
    centre = -np.linalg.solve(P[0, 1, :, :3].astype(np.float64), P[0, 1, :, 3].astype(np.float64))
    init[0, 2, :3] = (centre + 0.5 * (centre - world[0, 2])).astype(np.float32)   # (0, 2): behind camera 1
    refined = np.ones((N, K), bool)
    for n, k in NOT_REFINED:
        refined[n, k] = False
    assert (refined.sum(0) >= 2).all()
    return pts, P, init, views, refined


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def test_the_four_solvers_refine_the_same_points():
    from xas_amd import ops_calib, ops_eval, ops_track
    pts, P, init, views, refined = _inputs()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = (d(pts), d(P), d(init))
    want = torch.from_numpy(refined)
    start = _bits(args[2])
    assert torch.equal(start, torch.from_numpy(init.view(np.int32)))     # the payloads reached the device

    def passed_through(name, xyzw):
        got = _bits(xyzw)
        same = (got == start).all(-1)
        assert bool(same[~want].all()), '%s: a point outside the refined set is not init bit for bit' % name
        return ~same

    ref = ops_eval.triangulate_refine(*args, views=d(views), want=('status',))
    assert torch.equal(ref['status'].cpu() != 2, want), 'triangulate_refine: status %s' % ref['status'].cpu()
    moved = passed_through('triangulate_refine', ref['xyzw'])
    assert torch.equal(moved, want), 'triangulate_refine left a refined point where it started'

    sk = ops_eval.triangulate_skeleton(*args, views=d(views), limbs=(), want=('status',))
    assert torch.equal(sk['status'].cpu() != 2, want), 'triangulate_skeleton: status %s' % sk['status'].cpu()
    passed_through('triangulate_skeleton', sk['xyzw'])

    cal = ops_calib.calibrate_bundle(*args, torch.zeros(N, dtype=torch.int64), views=d(views), free=0, want=('status',))
    cal_moved = passed_through('calibrate_bundle', cal['xyzw'])
    assert torch.equal(cal_moved[moved], want[moved]), 'calibrate_bundle: moved %s' % cal_moved

    ts = ops_track.track_smooth(*args, np.zeros(N, np.int64), np.arange(N, dtype=np.int64), views=d(views),
                                want=('status', 'track_status'))
    assert bool((ts['track_status'].cpu() != 2).all()), 'track_smooth passed a whole track through'
    assert torch.equal(ts['status'].cpu() == 0, want), 'track_smooth: status %s' % ts['status'].cpu()
    assert bool((ts['status'].cpu()[~want] == 1).all())
    assert bool(torch.isfinite(ts['xyzw'].cpu()[~want][:, :3]).all())
    assert torch.equal(_bits(ts['xyzw'])[..., 3], start[..., 3])
