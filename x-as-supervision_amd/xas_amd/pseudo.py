"""Online pseudo samples (train.py --pseudo-online): an SMPL body from a bank of poses, turned by a random angle about the
vertical, placed at each sample's own pelvis, seen by the sample's own camera and rendered on the device
(modules.util.render_smpl_to_patch) - `<cam>_pseudo_img` and `<cam>_pseudo_joints` of every step from parameters alone.
The reference reads both from pre-rendered files ('{iter}_cam_{id}_{batch}.png', dataloader.py:193-230) that nothing in it
produces; there is no parity with those images."""
import numpy as np
import torch

from modules.util import render_smpl_to_patch


def _rodrigues(aa):
    """Axis-angle [N,3] -> rotation matrices [N,3,3] (float64, CPU)."""
    th = aa.norm(dim=1, keepdim=True)
    k = aa / th.clamp(min=1e-12)
    z = torch.zeros_like(th[:, 0])
    K = torch.stack([z, -k[:, 2], k[:, 1], k[:, 2], z, -k[:, 0], -k[:, 1], k[:, 0], z], dim=1).view(-1, 3, 3)
    s, c = torch.sin(th).view(-1, 1, 1), torch.cos(th).view(-1, 1, 1)
    return torch.eye(3, dtype=aa.dtype).expand_as(K) + s * K + (1 - c) * (K @ K)


def load_smpl_arrays(path):
    """`--smpl-model` given an .npz of exported SMPL arrays (SMPL_Layer.from_arrays' keys + `h36m_regressor`) -> that dict."""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


class PseudoSynth:
    """bank: path of (or mapping like) an .npz with `pose` [N,72] axis-angle (root orientation first) and optionally `betas`
    [N,10].  look: 'shade' | 'parts' (modules.util.RENDER_LOOKS).  up: the world's vertical, the axis of the random turn.
    mean, std: the config's dataset_params.dataiter entries; None = 0 and 255, the /255 of xas_amd.synthetic.
    Every draw comes from one CPU torch.Generator (the convention of modules.util.random_rotation_3D): the same seed and the
    same sequence of fill() calls give the same batches."""

    def __init__(self, bank, smpl_layer, h36m_regressor, look='shade', up=(0, 0, 1), seed=0, mean=None, std=None):
        if smpl_layer is None or h36m_regressor is None:
            raise RuntimeError('PseudoSynth needs an SMPL layer and the H36M joint regressor (train.py --smpl-model)')
        if isinstance(bank, (str, bytes)) or hasattr(bank, '__fspath__'):
            with np.load(bank, allow_pickle=False) as z:
                bank = {k: z[k] for k in z.files}
        pose = torch.as_tensor(np.asarray(bank['pose']), dtype=torch.float32)
        if pose.dim() != 2 or pose.shape[1] != 72 or pose.shape[0] == 0:
            raise ValueError('PseudoSynth: bank `pose` must be [N,72] with N >= 1, got %s' % (tuple(pose.shape),))
        betas = bank['betas'] if 'betas' in bank else np.zeros((pose.shape[0], 10), np.float32)
        betas = torch.as_tensor(np.asarray(betas), dtype=torch.float32)
        if tuple(betas.shape) != (pose.shape[0], 10):
            raise ValueError('PseudoSynth: bank `betas` must be [N,10], got %s' % (tuple(betas.shape),))
        self.pose, self.betas = pose, betas
        self.root = _rodrigues(pose[:, :3].double())                    # [N,3,3]
        up = torch.tensor(up, dtype=torch.float64)
        self.up = up / up.norm()
        self.smpl_layer, self.h36m_regressor, self.look = smpl_layer, h36m_regressor, look
        self.mean = torch.tensor([0.0] * 3 if mean is None else list(mean), dtype=torch.float32).view(1, 3, 1, 1)
        self.std = torch.tensor([255.0] * 3 if std is None else list(std), dtype=torch.float32).view(1, 3, 1, 1)
        self.gen = torch.Generator().manual_seed(int(seed))

    def draw(self, B):
        """-> (rows [B] int64, angles [B] float64 in [0, 2 pi)) from the CPU generator."""
        rows = torch.randint(self.pose.shape[0], (B,), generator=self.gen)
        ang = torch.rand(B, generator=self.gen, dtype=torch.float64) * (2.0 * torch.pi)
        return rows, ang

    def fill(self, x, cam_keys):
        """Writes `<key>_pseudo_img` [B,3,S,S] (normalised as the loader normalises a PNG, (255 v - mean) / std, without the
        file's 8-bit rounding) and `<key>_pseudo_joints` [B,18,3] into the batch dict `x` for every key of `cam_keys`; every
        sample and camera gets a row of the bank and an angle of its own.  -> x."""
        for key in cam_keys:
            img_key = key + '_img'
            dev, B, S = x[img_key].device, x[img_key].shape[0], x[img_key].shape[-1]
            rows, ang = self.draw(B)
            turn = _rodrigues(self.up.unsqueeze(0) * ang.unsqueeze(1)) @ self.root[rows]       # column-vector rotation
            # project_smpl_to_patch_kps multiplies row vectors from the right: p . G with G = R^T
            G = turn.transpose(1, 2).float().to(dev)
            if self.mean.device != dev:                                 # once: the layer and the constants follow the batch
                self.smpl_layer = self.smpl_layer.to(dev)
                self.h36m_regressor, self.mean, self.std = (t.to(dev) for t in (self.h36m_regressor, self.mean, self.std))
            img, _, joints = render_smpl_to_patch(G, self.pose[rows, 3:].to(dev), self.betas[rows].to(dev), self.smpl_layer,
                                                  self.h36m_regressor, x, key, look=self.look, size=S)
            x[key + '_pseudo_img'] = (img * 255.0 - self.mean) / self.std
            x[key + '_pseudo_joints'] = joints
        return x
