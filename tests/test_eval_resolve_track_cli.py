"""eval.py --resolve-track (model_params.resolve_track): the flags and their model_params keys and the error without a GPU; on
the GPU, on the planted evaluation batch of tests/test_eval_calib_cli.py repeated as frames of sequences, with four cameras and
with one: what the flag adds (a file, one last line per camera, nothing else moves) and that the file is a direct
ops_track.track_resolve call on what the batches kept."""
import os
import subprocess
import sys
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

from test_eval_fit_cli import _cfg

FLAGS = ['--resolve-track', '--rt-vel', '--rt-hyp', '--rt-swap', '--rt-gap']


def _parse(argv):
    import eval as xeval
    parser = ArgumentParser()
    for flag, kw in xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT + xeval.CLI_CALIB + xeval.CLI_SMOOTH + xeval.CLI_RESOLVE_TRACK:
        parser.add_argument(flag, **kw)
    return xeval, parser.parse_args(['--config', 'c.yaml'] + argv)


def test_flags_and_their_config_keys():
    xeval, opt = _parse([])
    flags = dict(xeval.CLI_RESOLVE_TRACK)
    assert list(flags) == FLAGS
    older = (xeval.CLI, xeval.CLI_VOLUME, xeval.CLI_FIT, xeval.CLI_CALIB, xeval.CLI_SMOOTH)
    assert not set(flags) & {f for table in older for f in dict(table)}
    assert list(dict(xeval.CLI_SMOOTH)) == ['--smooth', '--smooth-acc', '--smooth-gap', '--smooth-iters']     # as they were
    assert all(getattr(opt, k) is None for k in ('resolve_track', 'rt_vel', 'rt_hyp', 'rt_swap', 'rt_gap'))
    cfg = {'model_params': {}}
    xeval.mirror_resolve_track_options(cfg, opt)
    assert cfg['model_params'] == {}                                     # only the flags given become keys
    xeval, opt = _parse(['--resolve-track', 'out/r.npz', '--rt-hyp', '100', '--rt-gap', '3', '--smooth', 's.npz'])
    xeval.mirror_resolve_track_options(cfg, opt)
    assert cfg['model_params'] == {'resolve_track': 'out/r.npz', 'rt_hyp': 100.0, 'rt_gap': 3}
    assert opt.smooth == 's.npz'                                         # the two go together
    xeval, opt = _parse(['--resolve-track', 'r.npz', '--rt-vel', '0.5', '--rt-swap', '0'])
    cfg = {'model_params': {}}
    xeval.mirror_resolve_track_options(cfg, opt)
    assert cfg['model_params'] == {'resolve_track': 'r.npz', 'rt_vel': 0.5, 'rt_swap': 0.0}


def test_several_ranks_are_an_error_and_one_camera_is_not(monkeypatch):
    import eval as xeval
    from xas_amd import ops_track
    e = xeval.Eval(_cfg([0], resolve_track='a.npz', rt_swap=7.0), torch.nn.Identity(), [], 'log')
    assert (e.rt_vel, e.rt_hyp, e.rt_swap, e.rt_gap) == (ops_track.TRACK_VEL_W, ops_track.TRACK_HYP_W, 7.0, ops_track.TRACK_MAX_GAP)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='resolve_track needs WORLD_SIZE == 1'):
        xeval.Eval(_cfg([0], resolve_track='a.npz'), torch.nn.Identity(), [], 'log')
    assert xeval.Eval(_cfg([0]), torch.nn.Identity(), [], 'log').resolve_track is None      # without the key: no such error


def test_the_track_module_is_not_imported_without_the_flag():
    import eval as xeval
    pkg = os.path.dirname(os.path.abspath(xeval.__file__))
    code = ("import sys; sys.path[:0] = %r; import eval, torch; "
            "eval.Eval({'model_params': {'cam_id_list': [0]}, 'dataset_params': {'dataset': {'name': 'mpi_inf_3dhp'}}}, "
            "torch.nn.Identity(), [], 'log'); print('xas_amd.ops_track' in sys.modules)") % ([pkg, os.path.dirname(pkg)],)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == 'False', r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize('ncam', [4, 1])
def test_resolve_track_writes_its_file_and_moves_nothing_else(tmp_path, ncam):
    import eval as xeval
    from test_eval_calib_cli import _setup
    from xas_amd import ops_track
    cams, xd, det = _setup()
    cams = cams[:ncam]
    B, frames = xd['cam_0_joints'].shape[0], 3
    batches = [dict(xd, cam_0_img_path=['img/seq_%s_%06d.jpg' % ('abcdefgh'[b], 10 + 2 * f) for b in range(B)]) for f in range(frames)]
    path = str(tmp_path / 'out' / 'tracks.npz')
    texts, outs = {}, {}
    for tag, extra in (('today', {}), ('off', dict(resolve_track=None)), ('on', dict(resolve_track=path, rt_hyp=100.0))):
        e = xeval.Eval(_cfg(cams, **extra), det, [dict(b) for b in batches], str(tmp_path / tag))
        outs[tag] = e.eval_batch(dict(batches[0]), 'best')
        if tag == 'on':
            e.rt_rows = []
        e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        if tag == 'on':
            rows = e.rt_rows
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt').read().strip().split('\n')
    bits = lambda t: t.reshape(-1).contiguous().view(torch.uint8)
    for tag in ('off', 'on'):
        assert set(outs[tag]) == set(outs['today']) and all(torch.equal(bits(outs[tag][k]), bits(outs['today'][k])) for k in outs['today'])
    assert texts['off'] == texts['today']
    n = len(texts['today'])
    assert texts['on'][:n] == texts['today'] and len(texts['on']) == n + ncam
    for c, line in zip(cams, texts['on'][n:]):
        print(line)
        assert line.startswith('RESOLVE track cam_%d: %d tracks of mean length %s (vel %s, hyp 100.0, swap %s, gap %d): MPJPE hypothesis 0 as given ' % (
            c, B, float(frames), ops_track.TRACK_VEL_W, ops_track.TRACK_SWAP_W, ops_track.TRACK_MAX_GAP))
        assert ' mm (best with labels: ' in line and ' mm), exchanged ' in line and ' , hypothesis 0 kept ' in line and ' , passed through ' in line
    assert not os.path.exists(path + '.tmp.npz')
    N, K = B * frames, 18
    with np.load(path) as z:
        file = {k: z[k] for k in z.files}
    names = ('cost', 'frame', 'hyp', 'joints', 'named', 'sel', 'status', 'swap', 'track')
    assert sorted(file) == sorted('cam_%d_%s' % (c, k) for c in cams for k in names)
    assert len(rows) == frames and rows[0]['mode'] == 'best'
    for c in cams:
        m = 'cam_%d' % c
        f = {k: file['%s_%s' % (m, k)] for k in names}
        assert f['joints'].shape == (N, K, 3) and f['sel'].shape == (N, K, 3) and f['joints'].dtype == f['sel'].dtype == np.float32
        assert all(f[k].shape == (N, K) and f[k].dtype == np.uint8 for k in ('hyp', 'swap', 'status'))
        assert f['track'].shape == (N,) and f['frame'].shape == (N,) and f['cost'].shape == (B, K) and f['named'].shape == (B, K)
        assert f['cost'].dtype == np.float64 and f['named'].dtype == np.uint8
        assert f['track'].tolist() == list(range(B)) * frames and f['frame'].tolist() == sorted([10, 12, 14] * B)
        cat = lambda k: torch.cat([r[m][k] for r in rows])
        assert rows[0][m]['paths'] == batches[0]['cam_0_img_path'] and cat('kps').shape[0] == N and cat('kps').dim() == 4
        track, frame = ops_track.tracks_of([p for r in rows for p in r[m]['paths']], ops_track.TRACK_MAX_GAP)
        direct = ops_track.track_resolve(cat('kps'), cat('world'), track, frame, hyp_w=100.0, gt=cat('labels'))
        for k in ('sel', 'hyp', 'swap', 'status', 'cost', 'named'):
            assert np.array_equal(direct[k].cpu().numpy().view(np.uint8), f[k].view(np.uint8)), (m, k)
        perm = xeval.ops_eval.switch_perm(K, xeval.ops_eval.SWITCH_PAIRS, 'cuda')
        joints = ops_track.resolved_gather(cat('world'), direct['hyp'], direct['swap'], perm)
        assert np.array_equal(joints.cpu().numpy().view(np.uint32), f['joints'].view(np.uint32))
        assert (f['status'] == 0).any()                                  # three frames per track: the units with finite candidates are resolved
    # no paths in the batch: one key, the frame is the running index
    bare = xeval.Eval(_cfg(cams, resolve_track=path), det, [dict(xd), dict(xd)], str(tmp_path / 'bare'))
    bare.record(*bare.eval(None, *xeval.init_tables(bare.cal_per_act), mode='best'))
    with np.load(path) as z:
        assert z['cam_0_track'].tolist() == [0] * (2 * B) and z['cam_0_frame'].tolist() == list(range(2 * B))
