"""eval.py --smooth (model_params.smooth): the flags and their model_params keys and the two errors without a GPU; on the GPU,
on the planted evaluation batch of tests/test_eval_calib_cli.py repeated as three frames of four sequences, what --smooth adds (a
file, two last lines, nothing else moves) and that the file is a direct ops_track.track_smooth call on what the batches kept."""
import os
import subprocess
import sys
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

from test_eval_fit_cli import _cfg

FLAGS = ['--smooth', '--smooth-acc', '--smooth-gap', '--smooth-iters']


def _parse(argv):
    import eval as xeval
    parser = ArgumentParser()
    for flag, kw in xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT + xeval.CLI_CALIB + xeval.CLI_SMOOTH:
        parser.add_argument(flag, **kw)
    return xeval, parser.parse_args(['--config', 'c.yaml'] + argv)


def test_flags_and_their_config_keys():
    xeval, opt = _parse([])
    flags = dict(xeval.CLI_SMOOTH)
    assert list(flags) == FLAGS
    assert not set(flags) & (set(dict(xeval.CLI)) | set(dict(xeval.CLI_VOLUME)) | set(dict(xeval.CLI_FIT)) | set(dict(xeval.CLI_CALIB)))
    assert opt.smooth is None and opt.smooth_acc is None and opt.smooth_gap is None and opt.smooth_iters == 30
    cfg = {'model_params': {}}
    xeval.mirror_smooth_options(cfg, opt)
    assert cfg['model_params'] == {'smooth': None, 'smooth_iters': 30}
    xeval, opt = _parse(['--smooth', 'out/s.npz', '--smooth-acc', '0.2', '--smooth-gap', '3', '--smooth-iters', '12', '--calibrate', 'c.npz'])
    xeval.mirror_smooth_options(cfg, opt)
    assert cfg['model_params'] == {'smooth': 'out/s.npz', 'smooth_acc': 0.2, 'smooth_gap': 3, 'smooth_iters': 12}
    assert opt.calibrate == 'c.npz'                                     # the two go together


def test_one_camera_and_several_ranks_are_errors(monkeypatch):
    import eval as xeval
    with pytest.raises(ValueError, match='smooth needs 2 to'):
        xeval.Eval(_cfg([0], smooth='a.npz'), torch.nn.Identity(), [], 'log')
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='WORLD_SIZE == 1'):
        xeval.Eval(_cfg([0, 1], smooth='a.npz'), torch.nn.Identity(), [], 'log')


def test_the_track_module_is_not_imported_without_the_flag():
    import eval as xeval
    pkg = os.path.dirname(os.path.abspath(xeval.__file__))
    code = "import sys; sys.path[:0] = %r; import eval; print('xas_amd.ops_track' in sys.modules)" % ([pkg, os.path.dirname(pkg)],)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == 'False', r.stderr[-2000:]


@pytest.mark.gpu
def test_smooth_writes_its_file_and_moves_nothing_else(tmp_path):
    import eval as xeval
    from test_eval_calib_cli import _setup
    from xas_amd import ops_track
    cams, xd, det = _setup()
    B, frames = xd['cam_0_joints'].shape[0], 3
    batches = [dict(xd, cam_0_img_path=['img/seq_%s_%06d.jpg' % ('abcdefgh'[b], 10 + 2 * f) for b in range(B)]) for f in range(frames)]
    path = str(tmp_path / 'out' / 'smooth.npz')
    keys = dict(tri_refine='lm')
    texts, outs = {}, {}
    for tag, extra in (('today', {}), ('off', dict(smooth=None)), ('smooth', dict(smooth=path, smooth_iters=10))):
        e = xeval.Eval(_cfg(cams, **keys, **extra), det, [dict(b) for b in batches], str(tmp_path / tag), tri='robust')
        outs[tag] = e.eval_batch(dict(batches[0]), 'best')
        if tag == 'smooth':
            e.smooth_rows = []
        e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        if tag == 'smooth':
            rows = e.smooth_rows
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt').read().strip().split('\n')
    bits = lambda t: t.reshape(-1).contiguous().view(torch.uint8)
    for tag in ('off', 'smooth'):
        assert set(outs[tag]) == set(outs['today']) and all(torch.equal(bits(outs[tag][k]), bits(outs['today'][k])) for k in outs['today'])
    assert texts['off'] == texts['today']
    n = len(texts['today'])
    assert texts['smooth'][:n] == texts['today'] and len(texts['smooth']) == n + 2
    first, second = texts['smooth'][n:]
    print(first)
    print(second)
    assert first.startswith('SMOOTH %d tracks of mean length %s (acc %s, gap %d, 10 trials): TRI MPJPE ' % (
        B, float(frames), ops_track.TRACK_ACC_W, ops_track.TRACK_MAX_GAP))
    assert ' mm, reprojection RMS ' in first and ' px, gaps filled ' in first and ' , passed through ' in first
    assert second.startswith('SMOOTH filled gap joints: MPJPE ')
    assert not os.path.exists(path + '.tmp.npz')
    N, K = B * frames, 18
    with np.load(path) as z:
        assert sorted(z.files) == ['cost', 'frame', 'joints', 'status', 'track', 'track_status', 'trials']
        file = {k: z[k] for k in z.files}
    assert file['joints'].shape == (N, K, 3) and file['status'].shape == (N, K) and file['track'].shape == (N,) and file['frame'].shape == (N,)
    assert file['track_status'].shape == (B, K) and file['cost'].shape == (B, K, 2) and file['trials'].shape == (B, K)
    assert file['track'].tolist() == list(range(B)) * frames and file['frame'].tolist() == sorted([10, 12, 14] * B)
    assert (file['cost'][..., 1] <= file['cost'][..., 0]).all()
    cat = lambda k: None if rows[0][k] is None else torch.cat([r[k] for r in rows])
    assert rows[0]['views'] is not None and rows[0]['paths'] == batches[0]['cam_0_img_path']
    track, frame = ops_track.tracks_of([p for r in rows for p in r['paths']], ops_track.TRACK_MAX_GAP)
    direct = ops_track.track_smooth(cat('points'), cat('pmat'), cat('init'), track, frame, views=cat('views'), max_iter=10)
    assert np.array_equal(direct['xyzw'][..., :3].cpu().numpy().view(np.uint32), file['joints'].view(np.uint32))
    assert np.array_equal(direct['status'].cpu().numpy(), file['status'])
    # with --calibrate beside it each keeps its own rows
    both = xeval.Eval(_cfg(cams, smooth=path, calibrate=str(tmp_path / 'c.npz'), **keys), det, [], str(tmp_path / 'both'), tri='robust')
    both.eval_batch(dict(batches[0]), 'best')
    assert len(both.smooth_rows) == 1 and len(both.calib_rows) == 1
    # no paths in the batch: one key, the frame is the running index
    bare = xeval.Eval(_cfg(cams, smooth=path, **keys), det, [dict(xd), dict(xd)], str(tmp_path / 'bare'), tri='robust')
    bare.record(*bare.eval(None, *xeval.init_tables(bare.cal_per_act), mode='best'))
    with np.load(path) as z:
        assert z['track'].tolist() == [0] * (2 * B) and z['frame'].tolist() == list(range(2 * B))
