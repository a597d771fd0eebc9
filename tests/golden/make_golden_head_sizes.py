#!/usr/bin/env python3
"""Generate tests/golden/head_sizes.npz: the reference's own soft-argmax head functions on the seeded logits of
head_sizes_inputs.py, at cube sides other than 16/32/64.  The reference is IMPORTED from a checkout (as make_golden.py
does; none of its text is stored).  Run:  XAS_REFERENCE=<checkout> python tests/golden/make_golden_head_sizes.py

Only `generate_3d_integral_preds_tensor` / `find_peak` of KPDetector3DMulti and KPDetector3D are called, on bare instances
(no network is built); the softmax in front and the normalisation behind are the three lines of their `forward`.

Stored per case `<name>_...`: kps, z_peak_indices (multi-hypothesis cases), depth_prob_map, the reference autograd's
grad_logits for the seeded grad_kps sub-sampled at GRAD_STRIDE and its abs().max(), `crc` of the logits, and
`dev_kps` / `dev_dmap` / `dev_grad`: the reference's float32 result against the float64 restatement of
head_sizes_inputs.py (max abs; the gradient relative to the float64 gradient's maximum).  The tests' bars are multiples
of these.  The reference run in float64 is asserted to agree with the restatement to 1e-12 (hypotheses matched by depth), and the planted tie to be an
exact tie in the reference's float32 marginal, resolved to the lower bin."""
import os
import sys
import types

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('XAS_REFERENCE') or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REF or not os.path.isdir(os.path.join(REF, 'modules')):
    sys.exit('set XAS_REFERENCE (or pass the path) to a checkout of the reference project')
sys.path.insert(0, REF)
sys.path.insert(0, HERE)

import numpy as np                                                        # noqa: E402
import torch                                                              # noqa: E402
import torch.nn as nn                                                     # noqa: E402
import torch.nn.functional as F                                           # noqa: E402

# the reference's detector modules import easydict and torchvision's block classes at module level; neither is used here
_ed = types.ModuleType('easydict')
_ed.EasyDict = type('EasyDict', (dict,), {'__getattr__': dict.__getitem__, '__setattr__': dict.__setitem__})
sys.modules.setdefault('easydict', _ed)
if 'torchvision' not in sys.modules:
    _tv, _tvm, _tvr = (types.ModuleType(n) for n in ('torchvision', 'torchvision.models', 'torchvision.models.resnet'))
    _tvr.Bottleneck = type('Bottleneck', (nn.Module,), {'expansion': 4})
    _tvr.BasicBlock = type('BasicBlock', (nn.Module,), {'expansion': 1})
    _tv.models, _tvm.resnet = _tvm, _tvr
    sys.modules.update({'torchvision': _tv, 'torchvision.models': _tvm, 'torchvision.models.resnet': _tvr})

from modules.keypoint_detector_integral_multi import KPDetector3DMulti   # noqa: E402
from modules.keypoint_detector_integral import KPDetector3D              # noqa: E402
import modules.keypoint_detector_integral_multi as _m                     # noqa: E402
import head_sizes_inputs as hs                                            # noqa: E402

assert os.path.realpath(_m.__file__).startswith(os.path.realpath(REF) + os.sep)
torch.set_num_threads(8)


def bare(cls, **attrs):
    obj = cls.__new__(cls)
    nn.Module.__init__(obj)
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def ref_head(lg, K, num_hypo, neighbor):
    """-> kps [B,Hy,K,3], depth_prob_map [K,D], z_peak_indices [B,K,Hy] or None, pz [B,K,D]."""
    B, C, H, W = lg.shape
    D = C // K
    hm = F.softmax(lg.view(B, K, -1), 2).view(B, K, D, H, W)
    got = {}
    if neighbor:
        det = bare(KPDetector3DMulti, num_kp=K, num_hypo=num_hypo, neighbor_size=neighbor)
        orig = det.find_peak

        def find_peak(accu_z):
            got['pz'] = accu_z.detach().clone()
            return got.setdefault('idx', orig(accu_z))
        det.find_peak = find_peak
        x, y, z, dmap = det.generate_3d_integral_preds_tensor(hm, D, H, W)
        x, y, z = x / H * 2 - 1, y / W * 2 - 1, z / D * 2 - 1
        kps = torch.cat((x.unsqueeze(1).repeat(1, num_hypo, 1, 1), y.unsqueeze(1).repeat(1, num_hypo, 1, 1),
                         z.permute(0, 2, 1).unsqueeze(-1)), dim=-1)
        return kps, dmap, got['idx'], got['pz']
    det = bare(KPDetector3D, num_kp=K)
    x, y, z, dmap = det.generate_3d_integral_preds_tensor(hm, D, H, W)
    kps = torch.cat((x / H * 2 - 1, y / W * 2 - 1, z / D * 2 - 1), dim=2).unsqueeze(1)
    return kps, dmap, None, None


out = {}
for name, (D, K, B, hy, nb, seed) in hs.CASES.items():
    lg_np = hs.logits(name)
    gw = torch.from_numpy(hs.grad_kps(name))
    lg = torch.from_numpy(lg_np).requires_grad_(True)
    kps, dmap, idx, pz = ref_head(lg, K, hy, nb)
    (kps * gw).sum().backward()
    g32 = lg.grad
    # float64: the restatement (the tests' yardstick), and the reference itself as a check of the restatement
    l64 = torch.from_numpy(lg_np).double().requires_grad_(True)
    k64, pz64, i64 = hs.restate(l64, K, hy, nb)
    (k64 * gw.double()).sum().backward()
    g64 = l64.grad
    with torch.no_grad():
        rk, rd, ri, _ = ref_head(torch.from_numpy(lg_np).double(), K, hy, nb)
    # (hypotheses sorted by depth for this check: the order torch.topk gives EQUAL float64 scores is its own business)
    e64 = (float((rk.sort(dim=1).values - k64.detach().sort(dim=1).values).abs().max()), float((rd - pz64[0].detach()).abs().max()))
    assert max(e64) < 1e-12, (name, e64)
    if nb:
        assert torch.equal(ri.sort(-1).values, i64.sort(-1).values), name
        assert torch.equal(idx, i64), (name, idx[0, :2], i64[0, :2])     # the float32 run that is stored follows the tie rule
        c0, c1 = 4 * hs.tie_quads(D)[0] + 1, 4 * hs.tie_quads(D)[1] + 1
        if (0, 1) in hs.planted(name):
            assert float(pz[0, 1, c0]) == float(pz[0, 1, c1]), (name, float(pz[0, 1, c0]), float(pz[0, 1, c1]))
            assert idx[0, 1, :2].tolist() == [c0, c1], (name, idx[0, 1].tolist())
        for (b, k), (cz, amp) in hs.planted(name).items():       # every planted centre of the top amplitudes is a found peak
            want = sorted(cz if len(cz) == 3 else [c0, c1, cz[1]])
            assert sorted(idx[b, k].tolist()) == want, (name, b, k, idx[b, k].tolist(), want)
    gmax = float(g64.abs().max())
    dev = {'kps': float((kps.double() - k64).abs().max()), 'dmap': float((dmap.double() - pz64[0]).abs().max()),
           'grad': float((g32.double() - g64).abs().max()) / gmax}
    print('%-5s D=%3d K=%2d B=%d  dev kps %.3e  dmap %.3e  grad(rel) %.3e  |grad|max %.4e  crc %08x' % (
        name, D, K, B, dev['kps'], dev['dmap'], dev['grad'], float(g32.abs().max()), hs.checksum(lg_np)))
    out[name + '_kps'] = kps.detach().numpy()
    out[name + '_depth_prob_map'] = dmap.detach().numpy()
    if nb:
        out[name + '_z_peak_indices'] = idx.numpy()
    out[name + '_grad_logits_sub'] = g32.reshape(-1)[::hs.GRAD_STRIDE].numpy().copy()
    out[name + '_grad_amax'] = np.float32(g32.abs().max())
    out[name + '_crc'] = np.uint32(hs.checksum(lg_np))
    for k, v in dev.items():
        out['%s_dev_%s' % (name, k)] = np.float64(v)

path = os.path.join(HERE, 'head_sizes.npz')
np.savez_compressed(path, **out)
print('wrote', path, os.path.getsize(path), 'bytes')
