"""eval.py --smooth-bones (model_params.smooth_bones): the flag, its model_params key and its errors without a GPU, and that
nothing reaches ops_track.track_skeleton_smooth without it; on the GPU, on the planted batch of tests/test_eval_smooth_cli.py,
that with the flag the file is a direct ops_track.track_skeleton_smooth call on what the batches kept and gains its columns."""
import os
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

from _track_skeleton_inputs import PARENTS18
from test_eval_fit_cli import _cfg


def _parse(argv):
    import eval as xeval
    parser = ArgumentParser()
    for flag, kw in (xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT + xeval.CLI_CALIB + xeval.CLI_SMOOTH + xeval.CLI_RESOLVE_TRACK +
                     xeval.CLI_SMOOTH_ANCHOR + xeval.CLI_SMOOTH_BONES):
        parser.add_argument(flag, **kw)
    return xeval, parser.parse_args(['--config', 'c.yaml'] + argv)


def test_flag_and_its_config_key():
    xeval, opt = _parse([])
    assert list(dict(xeval.CLI_SMOOTH_BONES)) == ['--smooth-bones'] and opt.smooth_bones is None
    older = xeval.CLI + xeval.CLI_VOLUME + xeval.CLI_FIT + xeval.CLI_CALIB + xeval.CLI_SMOOTH + xeval.CLI_RESOLVE_TRACK + xeval.CLI_SMOOTH_ANCHOR
    assert '--smooth-bones' not in dict(older)
    cfg = {'model_params': {}}
    xeval.mirror_smooth_bones_options(cfg, opt)
    assert cfg['model_params'] == {}                                    # not given: no key
    xeval, opt = _parse(['--smooth', 's.npz', '--smooth-bones'])
    xeval.mirror_smooth_bones_options(cfg, opt)
    assert cfg['model_params'] == {'smooth_bones': True}                # the default weight, which lives in ops_track
    xeval, opt = _parse(['--smooth', 's.npz', '--smooth-bones', '0.5', '--smooth-data', 'anchor'])
    xeval.mirror_smooth_bones_options(cfg, opt)
    assert cfg['model_params'] == {'smooth_bones': 0.5} and opt.smooth_data == 'anchor'


def test_it_is_refused_without_smooth():
    xeval, opt = _parse(['--smooth-bones'])
    with pytest.raises(ValueError, match='needs --smooth'):
        xeval.mirror_smooth_bones_options({'model_params': {}}, opt)
    with pytest.raises(ValueError, match='smooth_bones couples the joints'):
        xeval.Eval(_cfg([0, 1], smooth_bones=0.1), torch.nn.Identity(), [], 'log')


def test_the_weight_and_the_bones_come_from_the_config():
    import eval as xeval
    from xas_amd import ops_track
    e = xeval.Eval(_cfg([0, 1], smooth='a.npz', smooth_bones=True, parent_ids=PARENTS18), torch.nn.Identity(), [], 'log')
    assert e.smooth_bones == ops_track.TRACK_BONE_W == 0.1 and e.bones.shape == (17, 2)
    assert xeval.Eval(_cfg([0, 1], smooth='a.npz', smooth_bones=0.25, parent_ids=PARENTS18), torch.nn.Identity(), [], 'log').smooth_bones == 0.25
    off = xeval.Eval(_cfg([0, 1], smooth='a.npz'), torch.nn.Identity(), [], 'log')
    assert off.smooth_bones is None and off.bone_columns({}) == {} and off.bone_words({}, None) == ('', '')
    false = xeval.Eval(_cfg([0, 1], smooth='a.npz', smooth_bones=False), torch.nn.Identity(), [], 'log')       # `smooth_bones: false` is off
    assert false.smooth_bones is None
    xeval.Eval(_cfg([0, 1], smooth_bones=False), torch.nn.Identity(), [], 'log')                                # and no error without smooth


def test_without_the_flag_the_skeleton_smoother_is_not_reached(monkeypatch):
    """write_smooth without the flag calls track_smooth with the arguments it always had; track_skeleton_smooth and
    track_bone_lengths are not touched."""
    import eval as xeval
    from xas_amd import ops_track
    seen = {}

    def forbidden(*a, **k):
        raise AssertionError('reached without --smooth-bones')

    def fake(points, pmat, init, track, frame, **kw):
        seen.update(kw)
        N, K = init.shape[:2]
        return {'xyzw': init.clone(), 'status': torch.zeros(N, K, dtype=torch.uint8), 'resid': torch.ones(N, K, 2), 'tracks': torch.zeros(1),
                'track_status': torch.zeros(1, K, dtype=torch.uint8), 'cost': torch.zeros(1, K, 2), 'trials': torch.zeros(1, K)}
    monkeypatch.setattr(ops_track, 'track_skeleton_smooth', forbidden)
    monkeypatch.setattr(ops_track, 'track_bone_lengths', forbidden)
    monkeypatch.setattr(ops_track, 'track_smooth', fake)
    monkeypatch.setattr(xeval, 'joint_errors', lambda joints, gt: torch.zeros(joints.shape[:2]))         # the metric kernel needs a GPU
    monkeypatch.setattr(xeval, 'save_npz', lambda path, cols: seen.setdefault('cols', sorted(cols)))
    e = xeval.Eval(_cfg([0, 1], smooth='a.npz'), torch.nn.Identity(), [], 'log')
    N, K = 3, 18
    e.smooth_rows = [dict(points=torch.zeros(N, 2, K, 3), pmat=torch.zeros(N, 2, 3, 4), init=torch.ones(N, K, 4), gt=torch.ones(N, K, 3),
                          views=None, paths=None)]
    lines = e.write_smooth()
    assert len(lines) == 2 and lines[0].startswith('SMOOTH 1 tracks')
    assert seen['cols'] == ['cost', 'frame', 'joints', 'status', 'track', 'track_status', 'trials']
    assert set(seen) - {'cols'} == {'views', 'weighted', 'huber_px', 'acc_w', 'max_iter'}


def test_with_anchors_the_flag_takes_the_skeleton_smoother_too(monkeypatch):
    """--smooth-data anchor with one camera and --smooth-bones: write_smooth_anchor hands its anchors and their information to
    track_skeleton_smooth with the lengths of track_bone_lengths, and track_anchor_smooth is not reached."""
    import eval as xeval
    from xas_amd import _lib, ops_track
    seen = {}
    N, K = 4, 18

    def forbidden(*a, **k):
        raise AssertionError('the per-joint smoother was reached with --smooth-bones')

    def fake(points, pmat, init, track, frame, bones, **kw):
        seen.update(kw, bones=bones)
        return {'xyzw': init.clone(), 'status': torch.ones(N, K, dtype=torch.uint8), 'resid': torch.ones(N, K, 2), 'tracks': torch.zeros(1),
                'track_status': torch.zeros(1, dtype=torch.uint8), 'cost': torch.zeros(1, 2), 'trials': torch.zeros(1),
                'bone': torch.full((N, 17, 2), 2.0), 'length': kw['length']}
    monkeypatch.setattr(ops_track, 'track_anchor_smooth', forbidden)
    monkeypatch.setattr(ops_track, 'track_smooth', forbidden)
    monkeypatch.setattr(ops_track, 'track_skeleton_smooth', fake)
    monkeypatch.setattr(xeval, 'joint_errors', lambda joints, gt: torch.zeros(joints.shape[:2]))         # the metric kernel needs a GPU
    monkeypatch.setattr(xeval, 'save_npz', lambda path, cols: seen.setdefault('cols', sorted(cols)))
    e = xeval.Eval(_cfg([0], smooth='a.npz', smooth_data='anchor', smooth_bones=0.5, parent_ids=PARENTS18), torch.nn.Identity(), [], 'log')
    pmat = torch.eye(3, 4).repeat(N, 1, 1, 1)
    anchor = torch.arange(N * K * 3, dtype=torch.float32).reshape(N, K, 3) + 100.0
    e.smooth_rows = [dict(points=torch.zeros(N, 1, K, 3), pmat=pmat, init=torch.cat([anchor, torch.ones(N, K, 1)], -1), gt=torch.ones(N, K, 3),
                          views=None, paths=None, anchor=anchor)]
    lines = e.write_smooth()
    assert lines[0].startswith('SMOOTH anchor (one camera') and ', bones (17 of weight 0.5): length RMS 2.0 -> 2.0 mm' in lines[0]
    assert lines[1].startswith('SMOOTH filled gap joints (anchor)') and lines[1].endswith(', bone length RMS at them 2.0 -> 2.0 mm')
    assert seen['cols'] == ['anchored', 'bone_err', 'bone_length', 'bones', 'cost', 'frame', 'joints', 'status', 'track', 'track_status', 'trials']
    assert torch.equal(seen['anchor'], anchor) and seen['info'].shape == (N, K, 6) and seen['bone_w'] == 0.5 and seen['anchor_huber'] == e.smooth_anchor_huber
    want = ops_track.track_bone_lengths(torch.cat([anchor, torch.ones(N, K, 1)], -1), np.zeros(N, np.int64), None, e.bones)
    assert torch.equal(seen['length'], want) and np.array_equal(seen['bones'], ops_track.bones_of(PARENTS18))
    assert _lib.query('xas_track_skeleton_workspace_bytes', N, K) < e.SKELETON_WORKSPACE_WARN


@pytest.mark.gpu
def test_with_the_flag_the_file_is_a_direct_skeleton_call(tmp_path):
    import eval as xeval
    from test_eval_calib_cli import _setup
    from xas_amd import ops_track
    cams, xd, det = _setup()
    B, frames = xd['cam_0_joints'].shape[0], 3
    batches = [dict(xd, cam_0_img_path=['img/seq_%s_%06d.jpg' % ('abcdefgh'[b], 10 + 2 * f) for b in range(B)]) for f in range(frames)]
    path = str(tmp_path / 'out' / 'smooth.npz')
    e = xeval.Eval(_cfg(cams, tri_refine='lm', smooth=path, smooth_iters=10, smooth_bones=True, parent_ids=PARENTS18), det, [dict(b) for b in batches],
                   str(tmp_path / 'log'), tri='robust')
    e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
    rows = e.smooth_rows
    text = open(tmp_path / 'log' / 'eval' / 'eval_result.txt').read().strip().split('\n')
    print(text[-2])
    print(text[-1])
    assert text[-2].startswith('SMOOTH %d tracks of mean length ' % B) and ', bones (17 of weight 0.1): length RMS ' in text[-2] and text[-2].endswith(' mm')
    assert text[-1].startswith('SMOOTH filled gap joints: MPJPE ') and ', bone length RMS at them ' in text[-1]
    N, K = B * frames, 18
    with np.load(path) as z:
        assert sorted(z.files) == ['bone_err', 'bone_length', 'bones', 'cost', 'frame', 'joints', 'status', 'track', 'track_status', 'trials']
        file = {k: z[k] for k in z.files}
    assert file['bones'].shape == (17, 2) and file['bone_length'].shape == (B, 17) and file['bone_err'].shape == (N, 17, 2)
    assert file['track_status'].shape == (B,) and file['cost'].shape == (B, 2) and file['trials'].shape == (B,)      # per track
    assert (file['cost'][:, 1] <= file['cost'][:, 0]).all()
    cat = lambda k: None if rows[0][k] is None else torch.cat([r[k] for r in rows])
    track, frame = ops_track.tracks_of([p for r in rows for p in r['paths']], ops_track.TRACK_MAX_GAP)
    direct = ops_track.track_skeleton_smooth(cat('points'), cat('pmat'), cat('init'), track, frame, ops_track.bones_of(PARENTS18),
                                             views=cat('views'), max_iter=10)
    assert np.array_equal(direct['xyzw'][..., :3].cpu().numpy().view(np.uint32), file['joints'].view(np.uint32))
    assert np.array_equal(direct['bone'].cpu().numpy().view(np.uint32), file['bone_err'].view(np.uint32))
    assert np.array_equal(direct['length'].cpu().numpy().view(np.uint32), file['bone_length'].view(np.uint32))
    assert not os.path.exists(path + '.tmp.npz')
