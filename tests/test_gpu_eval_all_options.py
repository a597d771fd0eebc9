"""eval.py with every option on at once, against the runs where each post-loop option (--fit-smpl, --calibrate, --smooth,
--resolve-track) stands alone over the same upstream options (--tri robust, --resolve views, --tri-weight spread,
--tri-skeleton, --tri-volume): the planted four-camera batch of tests/test_eval_calib_cli.py as three frames with image paths,
a planted detector that answers forward, forward_logits and forward_spread, and the synthetic body of
tests/_smplfit_inputs.py.  The options must not disturb each other: same eval_batch outputs, same files, same lines, in the
documented order."""
import glob
import os

import numpy as np
import pytest
import torch

import _smplfit_inputs as si
from test_eval_fit_cli import _cfg
from test_eval_volume_cli import PlantedVolumeDetector

pytestmark = pytest.mark.gpu
D, ITERS = 8, 8
UPSTREAM = dict(tri_weight='spread', tri_refine='skeleton', tri_volume=True, tri_vol_side=2000.0, tri_vol_grid=8, tri_vol_levels=2)
# the lines after the reference's block, in the order eval_result.txt has them
ORDER = ('TRI inlier views', 'RESOLVE views', 'TRI weight spread', 'TRI refine skeleton', 'TRI volume (', 'TRI volume status',
         'FIT smpl', 'CALIBRATE rig', 'SMOOTH ', 'SMOOTH filled', 'RESOLVE track ')
OWN = {'fit_smpl': ('FIT smpl',), 'calibrate': ('CALIBRATE rig',), 'smooth': ('SMOOTH ', 'SMOOTH filled'),
       'resolve_track': ('RESOLVE track ',)}


class PlantedAllDetector(PlantedVolumeDetector):
    """forward and forward_logits as planted for --tri-volume; forward_spread with a planted spread, as in test_eval_fit_cli."""

    def forward_spread(self, img, pairs):
        kps = self.kps[self.key(img)]
        return kps, None, torch.ones(kps.shape[0], self.num_kp, 5, device=kps.device)


def prefix_of(line):
    return max((p for p in ORDER if line.startswith(p)), key=len, default=None)    # the longest: 'SMOOTH ' starts 'SMOOTH filled'


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """{'all' and each post-loop option: (eval_batch outputs of the first batch, lines of eval_result.txt, {option: file})}."""
    import eval as xeval
    import _volume_inputs as vi
    from test_eval_calib_cli import _setup
    tmp = tmp_path_factory.mktemp('all_options')
    cams, xd, planted = _setup()
    det = PlantedAllDetector()
    det.kps, det.cubes = planted.kps, {}
    B, K = xd['cam_0_joints'].shape[0], det.num_kp
    rng = np.random.Generator(np.random.PCG64(5))
    for i in range(len(cams)):                    # log-Gaussians round each camera's hypothesis 0, a little noise on top
        centre = det.kps[i][:, 0].double().cpu().numpy()
        L = np.zeros((B, D, D, K * D), np.float32)
        for b in range(B):
            for k in range(K):
                L[b, :, :, k * D:(k + 1) * D] = vi.log_gaussian((centre[b, k] + 1.0) / 2.0 * D, D, 1.0) + 0.02 * rng.normal(size=(D, D, D))
        det.cubes[i] = torch.from_numpy(L).cuda().permute(0, 3, 1, 2)
    frames = 3
    batches = [dict(xd, cam_0_img_path=['img/seq_%s_%06d.jpg' % ('abcdefgh'[b], 10 + 2 * f) for b in range(B)]) for f in range(frames)]
    model = str(tmp / 'smpl.npz')
    np.savez(model, **{k: np.asarray(v) for k, v in si.arrays(70).items()})

    def keys_of(tag, option):
        path = str(tmp / tag / 'out' / (option + '.npz'))
        return path, {'fit_smpl': dict(fit_smpl=path, smpl_model=model, fit_iters=ITERS), 'calibrate': dict(calibrate=path, calib_iters=ITERS),
                      'smooth': dict(smooth=path, smooth_iters=ITERS), 'resolve_track': dict(resolve_track=path)}[option]

    out = {}
    for tag in ('all',) + tuple(OWN):
        keys, paths = dict(UPSTREAM), {}
        for option in (tuple(OWN) if tag == 'all' else (tag,)):
            paths[option], extra = keys_of(tag, option)
            keys.update(extra)
        e = xeval.Eval(_cfg(cams, **keys), det, [dict(b) for b in batches], str(tmp / tag), tri='robust', resolve='views')
        first = e.eval_batch(dict(batches[0]), 'best')
        for rows in ('fit_rows', 'calib_rows', 'smooth_rows', 'rt_rows'):
            if hasattr(e, rows):
                setattr(e, rows, [])
        e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        files = {}
        for option, path in paths.items():
            with np.load(path) as z:
                files[option] = {k: z[k] for k in z.files}
        out[tag] = (first, open(tmp / tag / 'eval' / 'eval_result.txt').read().strip().split('\n'), files)
    out['tmp'] = str(tmp)
    return out


def test_outputs_are_the_union_of_the_single_runs(runs):
    bits = lambda t: t.reshape(-1).contiguous().view(torch.uint8)
    full = runs['all'][0]
    assert set(full) == set().union(*(set(runs[o][0]) for o in OWN))
    assert {k for k in full if k.startswith('fit_')} == set(runs['fit_smpl'][0]) - set(runs['calibrate'][0])
    for option in OWN:
        for k, v in runs[option][0].items():
            assert v.dtype == full[k].dtype and torch.equal(bits(v), bits(full[k])), (option, k)


def test_every_file_is_its_single_runs_file(runs):
    for option in OWN:
        alone, full = runs[option][2][option], runs['all'][2][option]
        assert sorted(alone) == sorted(full) and len(full) > 0
        for k in full:
            assert full[k].dtype == alone[k].dtype and full[k].shape == alone[k].shape, (option, k)
            assert full[k].tobytes() == alone[k].tobytes(), (option, k)


def test_lines_come_in_order_and_equal_the_single_runs(runs):
    lines = runs['all'][1]
    start = next(i for i, l in enumerate(lines) if prefix_of(l) is not None)
    assert lines[start - 6] == '---Tri3D-----' and all(prefix_of(l) is None for l in lines[:start])     # the reference's block
    tail = lines[start:]
    for l in tail:
        print(l)
    seen = [prefix_of(l) for l in tail]
    assert None not in seen
    assert [p for i, p in enumerate(seen) if i == 0 or seen[i - 1] != p] == list(ORDER)
    assert seen.count('RESOLVE track ') == 4 and seen.count('SMOOTH ') == seen.count('SMOOTH filled') == 1
    upstream = [l for l in tail if prefix_of(l) in ORDER[:6]]
    assert len(upstream) == 6
    for option, own in OWN.items():
        alone = runs[option][1]
        assert alone[:start] == lines[:start], option
        assert [l for l in alone[start:] if prefix_of(l) in ORDER[:6]] == upstream, option
        assert [l for l in alone[start:] if prefix_of(l) in own] == [l for l in tail if prefix_of(l) in own], option
        assert len(alone) == start + 6 + sum(seen.count(p) for p in own), option


def test_no_temporary_file_is_left(runs):
    assert glob.glob(os.path.join(runs['tmp'], '**', '*.tmp.npz'), recursive=True) == []
    assert len(glob.glob(os.path.join(runs['tmp'], '**', 'out', '*.npz'), recursive=True)) == 8
