"""eval.py --tri-volume (model_params.tri_volume) on the planted evaluation batch of tests/test_gpu_tri_robust.py: what the
flag adds to eval_batch and to eval_result.txt, and that nothing moves without it.

The detector is planted: `forward` returns the stored hypotheses as in the other eval-entry tests, `forward_logits` returns the
same hypotheses plus small heat-map cubes (D = 8), log-Gaussians round the CLEAN detections of each camera, while the
hypotheses handed out are the corrupted ones: the fusion then has something to correct."""
import numpy as np
import pytest
import torch

import _volume_inputs as vi

pytestmark = pytest.mark.gpu
D = 8


class PlantedVolumeDetector(torch.nn.Module):
    num_kp = 18
    calls = 0

    def key(self, img):
        return int(img[0, 0, 0, 0].item())

    def forward(self, img):
        return self.kps[self.key(img)], None

    def forward_logits(self, img):
        self.calls += 1
        return self.kps[self.key(img)], None, self.cubes[self.key(img)]


def _setup():
    from test_gpu_tri_robust import eval_case
    x, kps, _ = eval_case()
    cams = [0, 1, 2, 3]
    xd = {k: v.cuda() for k, v in x.items()}
    det = PlantedVolumeDetector()
    det.kps, det.cubes = {}, {}
    rng = np.random.Generator(np.random.PCG64(5))
    for i, c in enumerate(cams):
        xd['cam_%d_img' % c] = torch.full((1, 3, 256, 256), float(i), device='cuda')
        det.kps[i] = kps[c][1].cuda()                                  # the corrupted hypotheses
        clean = kps[c][0][:, 0].double().numpy()                       # [B,K,3] normalised: cell = (x + 1) / 2 * D
        B, K = clean.shape[:2]
        L = np.zeros((B, D, D, K * D), np.float32)
        for b in range(B):
            for k in range(K):
                L[b, :, :, k * D:(k + 1) * D] = vi.log_gaussian((clean[b, k] + 1.0) / 2.0 * D, D, 1.0) + 0.02 * rng.normal(size=(D, D, D))
        det.cubes[i] = torch.from_numpy(L).cuda().permute(0, 3, 1, 2)
    return cams, xd, det


def _cfg(cams, **keys):
    cfg = {'model_params': {'cam_id_list': list(cams)}, 'dataset_params': {'dataset': {'name': 'mpi_inf_3dhp'}}}
    cfg['model_params'].update(keys)
    return cfg


VOL = dict(tri_volume=True, tri_vol_side=2000.0, tri_vol_grid=8, tri_vol_levels=2)      # 250 mm cells at D = 8


@pytest.mark.parametrize('tri,resolve', [('dlt', 'gt'), ('robust', 'gt'), ('dlt', 'views')])
def test_eval_batch_fuses_only_when_asked(tmp_path, tri, resolve):
    import eval as xeval
    from modules import util as mu
    cams, xd, det = _setup()
    mk = lambda **keys: xeval.Eval(_cfg(cams, **keys), det, [], str(tmp_path), tri=tri, resolve=resolve)
    today = mk().eval_batch(xd, 'best')
    assert det.calls == 0                                             # without the flag: the calls of today, forward alone
    off = mk(tri_volume=False).eval_batch(xd, 'best')
    assert set(off) == set(today) and all(torch.equal(off[k], today[k]) for k in today) and det.calls == 0
    vol = mk(**VOL).eval_batch(xd, 'best')
    assert det.calls == len(cams)
    assert set(vol) == set(today) | {'tri_vol_move_mm', 'tri_vol_sigma_mm', 'tri_vol_status'}
    for k in today:                                                   # nothing but the triangulated pose moves
        if 'tri' not in k:
            assert torch.equal(vol[k], today[k]), k
    assert not torch.equal(vol['world_tri'], today['world_tri'])
    st = vol['tri_vol_status']
    assert st.shape == (4,) and abs(float(st.sum()) - 1.0) < 1e-6 and float(st[3]) == 0.0
    moved = (vol['world_tri'] - today['world_tri']).norm(dim=-1)
    assert abs(float(vol['tri_vol_move_mm']) - float(moved.mean())) < 1e-3 * max(1.0, float(moved.mean()))
    assert float(vol['tri_vol_sigma_mm']) > 0
    if (tri, resolve) == ('dlt', 'gt'):                               # the start is today's point and the direct call agrees
        from xas_amd import ops_eval
        chan = []
        for i, c in enumerate(cams):
            s = ops_eval.eval_select(det.kps[i], xd['cam_%d_joints' % c], mode='best', want=('swapped',))['swapped'].squeeze(-1)
            perm = ops_eval.switch_perm(18, ops_eval.SWITCH_PAIRS, s.device)
            chan.append(torch.where(s, perm, torch.arange(18, device=s.device, dtype=torch.int32)))
        direct, _ = mu.triangulation_volume(today['world_tri'], {'cam_%d' % c: det.cubes[i] for i, c in enumerate(cams)}, xd, cams,
                                            torch.stack(chan), G=8, levels=2, side_mm=2000.0)
        assert torch.equal(vol['world_tri'], direct)
        print('mpjpe_tri: today', today['mpjpe_tri'].cpu().numpy(), 'fused', vol['mpjpe_tri'].cpu().numpy())


def test_result_file_gains_two_lines_with_the_flag_only(tmp_path):
    import eval as xeval
    cams, xd, det = _setup()
    texts = {}
    for tag, keys in (('today', {}), ('off', dict(tri_volume=False)), ('volume', VOL)):
        e = xeval.Eval(_cfg(cams, **keys), det, [dict(xd), dict(xd)], str(tmp_path / tag))
        e.record(*e.eval(None, *xeval.init_tables(e.cal_per_act), mode='best'))
        texts[tag] = open(tmp_path / tag / 'eval' / 'eval_result.txt').read()
    assert texts['off'] == texts['today']
    old, new = texts['today'].strip().split('\n'), texts['volume'].strip().split('\n')
    tri = old.index('---Tri3D-----')
    assert len(new) == len(old) + 2 and new[:tri + 1] == old[:tri + 1]
    assert new[tri + 1:tri + 4] != old[tri + 1:tri + 4]               # mpjpe, n-mpjpe, p-mpjpe of the triangulated pose
    assert new[-2].startswith('TRI volume (side 2000.0 mm, grid 8, levels 2): moved ') and ' mm, sigma ' in new[-2] and new[-2].endswith(' mm')
    assert new[-1].startswith('TRI volume status: fused ') and ' passed through ' in new[-1] and ' mode on a face ' in new[-1]


def test_the_flag_refuses_the_flip_test_and_too_many_cameras(tmp_path):
    import eval as xeval
    det = PlantedVolumeDetector()
    with pytest.raises(ValueError, match='--tri-volume does not go with --flip'):
        xeval.Eval(_cfg([0, 1, 2, 3], tri_volume=True), det, [], str(tmp_path), flip_test=True)
    with pytest.raises(ValueError, match='tri_volume fuses at most 6 cameras; cam_id_list has 7'):
        xeval.Eval(_cfg(list(range(7)), tri_volume=True), det, [], str(tmp_path))
    xeval.Eval(_cfg(list(range(7))), det, [], str(tmp_path), flip_test=True)      # neither applies without the flag
    flags = dict(xeval.CLI_VOLUME)
    assert not set(flags) & set(dict(xeval.CLI))
    assert flags['--tri-volume']['default'] is False and flags['--tri-vol-side']['default'] == 800.0
    assert flags['--tri-vol-grid']['default'] == 16 and flags['--tri-vol-levels']['default'] == 2
