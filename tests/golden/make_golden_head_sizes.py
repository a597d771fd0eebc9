#!/usr/bin/env python3
"""Generate tests/golden/head_sizes.npz (table CASES of head_sizes_inputs.py) and head_edges.npz (table EDGES): the
reference's own soft-argmax head functions on the seeded logits, at cube sides other than 16/32/64 and at the launch-geometry
edges.  The reference is IMPORTED from a checkout (as make_golden.py does; none of its text is stored).
Run:  XAS_REFERENCE=<checkout> python tests/golden/make_golden_head_sizes.py [cases] [edges]      (default: both files)

Only `generate_3d_integral_preds_tensor` / `find_peak` of KPDetector3DMulti and KPDetector3D are called, on bare instances
(no network is built); the softmax in front and the normalisation behind are the three lines of their `forward`.

Stored per case `<name>_...`: kps, z_peak_indices (multi-hypothesis cases), depth_prob_map, the reference autograd's
grad_logits for the seeded grad_kps sub-sampled at GRAD_STRIDE and its abs().max(), `crc` of the logits, and
`dev_kps` / `dev_dmap` / `dev_grad`: the reference's float32 result against the float64 restatement of
head_sizes_inputs.py (max abs; the gradient relative to the float64 gradient's maximum).  The tests' bars are multiples
of these.  The reference run in float64 is asserted to agree with the restatement to 1e-12 (hypotheses matched by depth), and the planted tie to be an
exact tie in the reference's float32 marginal, resolved to the lower bin.

EDGES only: the joints of `edge_unordered` (an exact tie at D = 128, zero-score fill-ins) are those whose hypothesis order the
reference leaves to torch.topk; what it returned is stored as it is, but `dev_kps`, `dev_grad` and `grad_amax` leave these
joints out, the tests compare them with float64 and with the literal lists of `edge_expected` only, and this script asserts
that the float64 AND the float32 restatement give exactly those lists."""
import os
import sys
import types

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
TABLES = [a for a in sys.argv[1:] if a in ('cases', 'edges')] or ['cases', 'edges']
_paths = [a for a in sys.argv[1:] if a not in ('cases', 'edges')]
REF = os.environ.get('XAS_REFERENCE') or (_paths[0] if _paths else None)
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


def generate(table, make_logits, unordered, tie_joints, planted_want):
    out = {}
    for name, (D, K, B, hy, nb, seed) in table.items():
        lg_np = make_logits(name)
        gw = torch.from_numpy(hs.grad_kps(name))
        keep = torch.ones(B, K, dtype=torch.bool)              # joints whose hypothesis order the reference defines
        for b, k in unordered(name):
            keep[b, k] = False
        kk = keep.view(B, 1, K, 1)                              # over kps [B,Hy,K,3]
        kg = keep.view(B, K, 1, 1, 1)                           # over logits [B,K,D,H,W]
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
            i32 = hs.restate(torch.from_numpy(lg_np), K, hy, nb)[2]
        # (hypotheses sorted by depth for this check: the order torch.topk gives EQUAL float64 scores is its own business)
        e64 = (float(((rk.sort(dim=1).values - k64.detach().sort(dim=1).values) * kk).abs().max()), float((rd - pz64[0].detach()).abs().max()))
        assert max(e64) < 1e-12, (name, e64)
        if nb:
            assert torch.equal(ri.sort(-1).values[keep], i64.sort(-1).values[keep]), name
            assert torch.equal(idx[keep], i64[keep]), (name, idx[0, :2], i64[0, :2])   # the float32 run that is stored follows the tie rule
            assert torch.equal(i32, i64), name                  # and so does the float32 restatement, everywhere
            for b, k in unordered(name):
                print('  %s joint (%d, %d): reference float32 %s, float64 %s; the rule gives %s' % (
                    name, b, k, idx[b, k].tolist(), ri[b, k].tolist(), i64[b, k].tolist()))
            for (b, k), (c0, c1) in tie_joints(name).items():
                assert float(pz[b, k, c0]) == float(pz[b, k, c1]), (name, float(pz[b, k, c0]), float(pz[b, k, c1]))
                assert float(pz64[b, k, c0].detach()) == float(pz64[b, k, c1].detach()), name
                assert i64[b, k, :2].tolist() == [c0, c1], (name, i64[b, k].tolist())
            for (b, k), want in planted_want(name).items():   # every planted centre of the top amplitudes is a found peak
                assert i64[b, k].tolist() == want, (name, b, k, i64[b, k].tolist(), want)
        gmax = float(g64.abs().max())
        g32v = g32.view(B, K, D, D, D)
        dev = {'kps': float(((kps.detach().double() - k64.detach()) * kk).abs().max()), 'dmap': float((dmap.detach().double() - pz64[0].detach()).abs().max()),
               'grad': float(((g32v.double() - g64.view(B, K, D, D, D)) * kg).abs().max()) / gmax}
        assert all(0 < v < 1e-3 for v in dev.values()), (name, dev)
        amax = float((g32v * kg).abs().max())
        print('%-6s D=%3d K=%3d B=%d  dev kps %.3e  dmap %.3e  grad(rel) %.3e  |grad|max %.4e  crc %08x' % (
            name, D, K, B, dev['kps'], dev['dmap'], dev['grad'], amax, hs.checksum(lg_np)), flush=True)
        out[name + '_kps'] = kps.detach().numpy()
        out[name + '_depth_prob_map'] = dmap.detach().numpy()
        if nb:
            out[name + '_z_peak_indices'] = idx.numpy()
        out[name + '_grad_logits_sub'] = g32.reshape(-1)[::hs.GRAD_STRIDE].numpy().copy()
        out[name + '_grad_amax'] = np.float32(amax)
        out[name + '_crc'] = np.uint32(hs.checksum(lg_np))
        for k, v in dev.items():
            out['%s_dev_%s' % (name, k)] = np.float64(v)
    return out


def write(fname, out):
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


def case_ties(name):
    D = hs.CASES[name][0]
    a, b = hs.tie_quads(D)
    return {(0, 1): (4 * a + 1, 4 * b + 1)} if (0, 1) in hs.planted(name) else {}


def case_want(name):
    D = hs.CASES[name][0]
    a, b = hs.tie_quads(D)
    return {bk: ([c for _, c in sorted(zip(amp, cz), reverse=True)] if len(cz) == 3 else [4 * a + 1, 4 * b + 1, cz[1]])
            for bk, (cz, amp) in hs.planted(name).items()}


def edge_ties(name):
    return {bk: (4 * t[0] + 1, 4 * t[1] + 1) for bk, (cz, amp, t, noise) in hs.edge_planted(name).items() if t}


if 'cases' in TABLES:
    write('head_sizes.npz', generate(hs.CASES, hs.logits, lambda name: [], case_ties, case_want))
if 'edges' in TABLES:
    write('head_edges.npz', generate(hs.EDGES, hs.edge_logits, hs.edge_unordered, edge_ties, hs.edge_expected))
