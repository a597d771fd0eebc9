"""Online pseudo samples on the GPU: modules.util.render_smpl_to_patch against its parts (project_smpl_to_patch_kps for the
joints, ops_render.render_mesh on the same projected vertices for the image), xas_amd.pseudo.PseudoSynth's seeding, and one
training step on a batch that PseudoSynth filled.  The SMPL arrays are the synthetic stand-ins of tests/golden/inputs.py at a
small vertex count with a seeded face list; the batch is xas_amd.synthetic's, B = 2, two cameras."""
import numpy as np
import pytest
import torch

import inputs as gi

pytestmark = pytest.mark.gpu
V, F, CAMS = 96, 160, [0, 1]


def smpl_arrays():
    a = gi.smpl_buffers(41, V=V)
    a['v_template'] = a['v_template'] * 0.6                              # metres: a body-sized cloud
    a['f'] = np.random.Generator(np.random.PCG64(42)).integers(0, V, (F, 3))
    return a


def setup(B=2):
    from modules.smplpytorch.pytorch.smpl_layer import SMPL_Layer
    from xas_amd.synthetic import synthetic_batch
    a = smpl_arrays()
    layer = SMPL_Layer.from_arrays(a, center_idx=0).cuda()
    reg = torch.as_tensor(a['h36m_regressor']).cuda()
    x = synthetic_batch(B, CAMS, torch.device('cuda'), seed=8)
    g = torch.Generator().manual_seed(9)
    pose = (0.3 * torch.randn(B, 69, generator=g)).cuda()
    betas = torch.randn(B, 10, generator=g).cuda()
    q, _ = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))
    return layer, reg, x, q.cuda().contiguous(), pose, betas


def bank(N=5):
    g = torch.Generator().manual_seed(10)
    return {'pose': (0.3 * torch.randn(N, 72, generator=g)).numpy(), 'betas': torch.randn(N, 10, generator=g).numpy()}


@pytest.mark.parametrize('look', ['shade', 'parts'])
def test_render_smpl_to_patch_is_its_parts(look):
    from modules import util as mu
    from xas_amd import ops_head, ops_render
    layer, reg, x, rot, pose, betas = setup()
    for mode in ('cam_0', 'cam_1'):
        S = x[mode + '_img'].shape[-1]
        img, mask, joints = mu.render_smpl_to_patch(rot, pose, betas, layer, reg, x, mode, look=look, size=S)
        assert img.shape == (2, 3, S, S) and mask.shape == (2, 1, S, S) and joints.shape == (2, 18, 3)
        kps = mu.project_smpl_to_patch_kps(rot, pose, betas, layer, reg, x, mode)
        expect = torch.cat([kps[..., :2] / (S - 1.0) * 2.0 - 1.0, kps[..., 2:3] / float(S)], dim=-1)
        assert torch.equal(joints, expect)
        world = mu.project_smpl_to_patch_kps(rot, pose, betas, layer, reg, x, mode, convert_verts=True)
        assert (ops_head.world_to_patch(world, x, mode, stop_at_image=True)[..., 2] > 0).all()     # nothing behind the camera here
        pix = ops_head.world_to_patch(world, x, mode, is_norm=False)
        rgb = ops_render.part_colours(layer.th_weights, layer.th_faces) if look == 'parts' else None
        r = ops_render.render_mesh(pix, layer.th_faces, face_rgb=rgb, ambient=1.0 if look == 'parts' else 0.35, size=S)
        assert torch.equal(img, r['img']) and torch.equal(mask, r['mask'])
        print('%s %s: %d of %d pixels covered' % (look, mode, int(mask.sum()), mask.numel()))
        assert 0 < float(mask.sum()) < mask.numel() and float(img.min()) >= 0 and float(img.max()) <= 1
        if look == 'parts':
            palette = torch.tensor(ops_render.PART_PALETTE, device='cuda')
            cols = img.permute(0, 2, 3, 1)[mask[:, 0] > 0]
            assert ((cols[:, None] - palette[None]).abs().amax(-1) == 0).any(1).all()


def test_vertices_behind_the_camera_are_dropped():
    from modules import util as mu
    layer, reg, x, rot, pose, betas = setup()
    x = dict(x)
    x['cam_0_pelvis'] = x['cam_0_pelvis'].clone()
    x['cam_0_pelvis'][0, 2] = -4000.0                                    # sample 0 wholly behind its camera
    img, mask, _ = mu.render_smpl_to_patch(rot, pose, betas, layer, reg, x, 'cam_0')
    assert float(mask[0].sum()) == 0 and float(img[0].abs().sum()) == 0 and float(mask[1].sum()) > 0


def test_pseudo_synth_is_seeded():
    from xas_amd.pseudo import PseudoSynth
    from xas_amd.synthetic import synthetic_batch
    layer, reg, x, *_ = setup()
    keys = ['cam_%d' % c for c in CAMS]
    outs = []
    for seed in (3, 3, 4):
        xb = dict(x)
        PseudoSynth(bank(), layer, reg, 'shade', seed=seed).fill(xb, keys)
        outs.append(xb)
    for k in keys:
        for name, shape in (('_pseudo_img', x[k + '_img'].shape), ('_pseudo_joints', (2, 18, 3))):
            a, b, c = (o[k + name] for o in outs)
            assert a.shape == shape and a is not x[k + name] and torch.isfinite(a).all()
            assert torch.equal(a, b) and not torch.equal(a, c)
    # every camera and sample draws for itself
    assert not torch.equal(outs[0]['cam_0_pseudo_joints'][0] - outs[0]['cam_0_pseudo_joints'][0, :1],
                           outs[0]['cam_0_pseudo_joints'][1] - outs[0]['cam_0_pseudo_joints'][1, :1])
    # mean / std as the loader applies them to a 0..255 image
    xb = dict(x)
    PseudoSynth(bank(), layer, reg, 'shade', seed=3, mean=[10.0, 20.0, 30.0], std=[50.0, 60.0, 70.0]).fill(xb, keys)
    m, s = torch.tensor([10.0, 20.0, 30.0], device='cuda').view(1, 3, 1, 1), torch.tensor([50.0, 60.0, 70.0], device='cuda').view(1, 3, 1, 1)
    back = (xb['cam_0_pseudo_img'] * s + m) / 255.0
    assert float((back - outs[0]['cam_0_pseudo_img']).abs().max()) < 1e-5


def test_one_training_step_on_rendered_pseudo_samples():
    from xas_amd import engine
    from xas_amd.pseudo import PseudoSynth
    from xas_amd.synthetic import model_config, synthetic_batch
    cfg = model_config('HM36_Multi_SynthS1')
    cfg['model_params']['cam_id_list'] = CAMS
    torch.manual_seed(0)
    model, disc, od, odisc = engine.prepare_model(cfg, smpl_arrays())
    model.cuda().train(), disc.cuda().train()
    step = engine.TrainStep(cfg, model, disc, od, odisc)
    x = synthetic_batch(2, CAMS, torch.device('cuda'), seed=3)
    before = x['cam_0_pseudo_img']
    PseudoSynth(bank(), model.smpl_layer, model.h36m_regressor, 'shade', seed=1).fill(x, ['cam_%d' % c for c in CAMS])
    assert x['cam_0_pseudo_img'] is not before and x['cam_0_pseudo_img'].shape == before.shape
    ld, lk, tot, _ = step(x)
    torch.cuda.synchronize()
    assert 'smpl_pseudo_img' in lk and all(torch.isfinite(v).all() for v in lk.values())
    assert torch.isfinite(tot) and torch.isfinite(ld)
