"""eval.py --smooth OUT.npz --smooth-data anchor on the planted batch of tests/test_gpu_eval_all_options.py as three frames with
image paths: once with one camera together with --resolve-track (whose choice is the anchor), once with four cameras and
--tri-volume (the fused points with the inverse of their covariance).  The file's columns, finite outputs, the two lines."""
import numpy as np
import pytest
import torch

from test_eval_fit_cli import _cfg
from test_gpu_eval_all_options import D, PlantedAllDetector

pytestmark = pytest.mark.gpu
ITERS, FRAMES, K = 8, 3, 18
COLUMNS = ['anchored', 'cost', 'frame', 'joints', 'status', 'track', 'track_status', 'trials']


def planted():
    import _volume_inputs as vi
    from test_eval_calib_cli import _setup
    cams, xd, base = _setup()
    det = PlantedAllDetector()
    det.kps, det.cubes = base.kps, {}
    B = xd['cam_0_joints'].shape[0]
    rng = np.random.Generator(np.random.PCG64(5))
    for i in range(len(cams)):
        centre = det.kps[i][:, 0].double().cpu().numpy()
        L = np.zeros((B, D, D, K * D), np.float32)
        for b in range(B):
            for k in range(K):
                L[b, :, :, k * D:(k + 1) * D] = vi.log_gaussian((centre[b, k] + 1.0) / 2.0 * D, D, 1.0) + 0.02 * rng.normal(size=(D, D, D))
        det.cubes[i] = torch.from_numpy(L).cuda().permute(0, 3, 1, 2)
    batches = [dict(xd, cam_0_img_path=['img/seq_%s_%06d.jpg' % ('abcdefgh'[b], 10 + 2 * f) for b in range(B)]) for f in range(FRAMES)]
    return cams, det, batches, B


def run(tmp_path, cams, det, batches, **keys):
    import eval as xeval
    e = xeval.Eval(_cfg(cams, smooth=str(tmp_path / 'out' / 'smooth.npz'), smooth_data='anchor', smooth_iters=ITERS, **keys), det,
                   [dict(b) for b in batches], str(tmp_path))
    e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
    with np.load(str(tmp_path / 'out' / 'smooth.npz')) as z:
        file = {k: z[k] for k in z.files}
    lines = open(tmp_path / 'eval' / 'eval_result.txt').read().strip().split('\n')
    return e, file, [l for l in lines if l.startswith('SMOOTH')], lines


def check_file(file, B):
    N = B * FRAMES
    assert sorted(file) == COLUMNS
    assert file['joints'].shape == (N, K, 3) and file['status'].shape == (N, K) and file['anchored'].shape == (N, K)
    assert file['anchored'].dtype == np.uint8 and file['track'].shape == (N,) and file['frame'].shape == (N,)
    assert file['track_status'].shape == (B, K) and file['cost'].shape == (B, K, 2) and file['trials'].shape == (B, K)
    assert (file['cost'][..., 1] <= file['cost'][..., 0]).all()
    assert np.isfinite(file['joints'][file['anchored'] == 1]).all()
    assert (file['status'][file['anchored'] == 1] == 0).all()          # a usable anchor makes a data frame


def test_one_camera_smooths_the_choice_of_resolve_track(tmp_path):
    from xas_amd import ops_track
    cams, det, batches, B = planted()
    e, file, smooth, lines = run(tmp_path, cams[:1], det, batches, resolve_track=str(tmp_path / 'out' / 'rt.npz'))
    check_file(file, B)
    with np.load(str(tmp_path / 'out' / 'rt.npz')) as z:
        chosen = z['cam_0_joints']
    assert np.array_equal(file['anchored'] == 1, np.isfinite(chosen).all(-1)) and file['anchored'].any()
    assert np.isfinite(file['joints']).all() and (file['status'] == 0).all() and (file['trials'] >= 1).all()
    for l in smooth:
        print(l)
    assert len(smooth) == 2 and lines[-1].startswith('RESOLVE track cam_0')                      # the track lines stay last
    assert smooth[0].startswith('SMOOTH anchor (one camera, depth %s, huber %s) %d tracks of mean length %s (acc %s, gap %d, %d trials): '
                                'VIEW MPJPE ' % (ops_track.TRACK_DEPTH_W, ops_track.TRACK_ANCHOR_HUBER, B, float(FRAMES),
                                                 ops_track.TRACK_ACC_W, ops_track.TRACK_MAX_GAP, ITERS))
    assert ' mm, reprojection RMS ' in smooth[0] and ' px, anchored 1.0 , gaps filled 0.0 , passed through 0.0' in smooth[0]
    assert smooth[1].startswith('SMOOTH filled gap joints (anchor): MPJPE ')
    # the file is a direct call on what the batches kept, anchored on the other option's file
    rows = e.smooth_rows
    cat = lambda k: torch.cat([r[k] for r in rows])
    assert rows[0]['points'].shape[1] == 1 and rows[0]['views'] is None
    track, frame = ops_track.tracks_of([p for r in rows for p in r['paths']], ops_track.TRACK_MAX_GAP)
    anchor = torch.as_tensor(chosen).cuda()
    init = torch.cat([anchor, torch.ones_like(anchor[..., :1])], -1)
    direct = ops_track.track_anchor_smooth(cat('points'), cat('pmat'), init, track, frame, anchor=anchor,
                                           info=ops_track.ray_information(cat('pmat')[:, 0], anchor), max_iter=ITERS)
    assert np.array_equal(direct['xyzw'][..., :3].cpu().numpy().view(np.uint32), file['joints'].view(np.uint32))


def test_one_camera_without_resolve_track_anchors_on_its_own_selection(tmp_path):
    cams, det, batches, B = planted()
    e, file, smooth, lines = run(tmp_path, cams[:1], det, batches)
    check_file(file, B)
    assert np.isfinite(file['joints']).all() and file['anchored'].all() and len(smooth) == 2 and lines[-1] == smooth[1]
    assert torch.equal(e.smooth_rows[0]['anchor'], e.smooth_rows[0]['init'][..., :3])


def test_four_cameras_smooth_the_fused_points(tmp_path):
    cams, det, batches, B = planted()
    e, file, smooth, lines = run(tmp_path, cams, det, batches, tri_volume=True, tri_vol_side=2000.0, tri_vol_grid=8, tri_vol_levels=2)
    check_file(file, B)
    for l in smooth:
        print(l)
    rows = e.smooth_rows
    assert rows[0]['points'].shape[1] == 4 and not rows[0]['points'][..., 2].any() and not rows[0]['views'].any()    # no pixels
    usable = torch.isfinite(torch.cat([r['anchor'] for r in rows])).all(-1) & torch.isfinite(torch.cat([r['info'] for r in rows])).all(-1)
    assert np.array_equal(file['anchored'] == 1, usable.cpu().numpy()) and file['anchored'].any()
    assert len(smooth) == 2 and smooth[0].startswith('SMOOTH anchor (fused points, huber 3.0) %d tracks of mean length %s ' % (B, float(FRAMES)))
    assert 'TRI MPJPE ' in smooth[0] and 'reprojection RMS nan -> nan px' in smooth[0]
    assert smooth[1].startswith('SMOOTH filled gap joints (anchor): MPJPE ')
    assert np.isfinite(file['joints'][file['status'] != 2]).all()
