"""The multi-view consistency loss without a GPU: both entry points are exported, declared in include/xas_hip.h under their
comment and bound by the ctypes table with matching argument lists; their argument checks answer before any launch and name the
limit; train.py knows the four --mv flags and leaves the older ones as they were; and the inputs of every case of
tests/test_gpu_multiview.py are validated here with the oracle alone: the oracle's analytic gradient against
torch.linalg.eigh's float64 autograd and against central differences, the eigenvalue ratio of every compared joint, and a
decidable hypothesis choice."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'x-as-supervision_amd')
FWD, BWD = 'xas_multiview_consistency_fwd', 'xas_multiview_consistency_bwd'
SIGS = {FWD: ('pppppiiiiffipppppp', 'i'), BWD: ('pppppppiiiiffippp', 'i')}


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib, ops_eval
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in SIGS.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig and _lib.SIGNATURES[name] == sig
        assert len(_lib.fn(name).argtypes) == len(sig[0])
    header = open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()
    decl = re.search(r'/\*((?:(?!\*/).)*)\*/\s*#define XAS_MV_DETACH_TARGET (\d+)[^\n]*\n\s*int\s+%s\s*\((?:(?!/\*).)*int\s+%s\s*\(' % (
        FWD, BWD), header, re.S)
    assert decl, 'include/xas_hip.h does not declare the two entry points under their comment and flag'
    spec = decl.group(1)
    for phrase in ('in double', 'PASSED THROUGH', 'exactly 0', 'first minimum', 'ascending order', 'no atomics', 'EVERY entry',
                   '(lambda_0 - lambda_j)', 'sym(v_j x^T)', '2 c_v^2 a_u^T g_G P2_v', '2 huber_px e - huber_px^2', '1 <= Hy <= 8',
                   'B*K < 2^31', 'mm^2'):
        assert phrase in spec, 'the specification does not fix %r' % phrase
    assert int(decl.group(2)) == 1 == ops_eval.MV_DETACH_TARGET


def test_abi_version_is_unchanged():
    from xas_amd import _lib
    assert _lib.fn('xas_abi_version')() == 3 == _lib.ABI_VERSION


@pytest.mark.parametrize('name', [FWD, BWD])
def test_argument_checks_return_errors_without_a_gpu(name):
    from xas_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)                       # any aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    f = _lib.fn(name)
    n_in, n_out = (4, 5) if name == FWD else (4, 4)                   # required buffers before and after the scalars (weight may be NULL)

    def call(B=2, V=4, Hy=3, K=5, size=256.0, huber=0.0, flags=0, null=None):
        bufs = [one] * (n_in + n_out)
        if null is not None:
            bufs[null] = None
        if name == FWD:
            return f(*bufs[:4], None, B, V, Hy, K, size, huber, flags, *bufs[4:], None)
        return f(*bufs[:4], None, bufs[4], bufs[5], B, V, Hy, K, size, huber, flags, *bufs[6:], None)
    for V in (1, 7):
        assert call(V=V) == 1 and 'V=%d views (needs 2 <= V <= XAS_TRI_MAX_VIEWS = 6)' % V in err()
    for Hy in (0, 9):
        assert call(Hy=Hy) == 1 and 'Hy=%d hypotheses (needs 1 <= Hy <= 8)' % Hy in err()
    assert call(B=0) == 1 and 'bad shape B=0 K=5' in err()
    assert call(K=0) == 1 and 'bad shape B=2 K=0' in err()
    assert call(B=1 << 16, K=1 << 15) == 1 and 'B*K < 2^31' in err()
    for bad in (-1.0, float('inf'), float('nan')):
        assert call(huber=bad) == 1 and 'needs a finite huber_px >= 0' in err()
    assert call(size=1.0) == 1 and 'image_size' in err()
    for bad in (2, 3, 1 << 30, -2):
        assert call(flags=bad) == 1 and 'unknown flag bits' in err() and 'XAS_MV_DETACH_TARGET = 1' in err()
    for i in range(n_in + n_out):
        assert call(null=i) == 1 and 'null buffer (everything but weight is required)' in err()
    assert name[4:] in err()


def test_train_knows_the_flags_and_leaves_the_others_alone():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, os.path.join(PKG, 'train.py'), '--help'], capture_output=True, text=True, env=env, timeout=170)
    assert r.returncode == 0, r.stderr
    for flag in ('--mv-2d W', '--mv-3d W', '--mv-huber PX', '--mv-detach'):
        assert flag in r.stdout, flag
    import train as xtrain
    cli = dict(xtrain.CLI)
    assert list(cli) == ['--config', '--log_dir', '--checkpoint', '--batch_size', '--epoch', '--worker', '--extra_tag', '--finetune',
                         '--seed', '--synthetic', '--mv-2d', '--mv-3d', '--mv-huber', '--mv-detach']
    # the older flags, word for word
    assert cli['--config'] == dict(required=True, help='path to config')
    assert cli['--log_dir'] == dict(default='log', help='path to log into')
    assert cli['--checkpoint'] == dict(default=None, help='path to checkpoint to restore')
    assert cli['--batch_size'] == dict(default=None, type=int) == cli['--epoch']
    assert cli['--worker'] == dict(default=10, type=int) and cli['--extra_tag'] == dict(default='')
    assert cli['--finetune'] == dict(default=False, action='store_true', help='finetune the model')
    assert cli['--seed'] == dict(default=-1, type=int)
    assert cli['--synthetic'] == dict(default=0, type=int, help='train on N synthetic batches per epoch')
    assert cli['--mv-2d']['default'] is None and cli['--mv-3d']['default'] is None and cli['--mv-huber']['default'] == 0.0
    from argparse import ArgumentParser
    parser = ArgumentParser()
    for flag, kw in xtrain.CLI:
        parser.add_argument(flag, **kw)
    assert xtrain.multiview_entry(parser.parse_args(['--config', 'c', '--mv-huber', '3'])) is None        # neither weight: nothing
    assert xtrain.multiview_entry(parser.parse_args(['--config', 'c', '--mv-3d', '1e-4', '--mv-detach'])) == dict(
        weight_2d=0.0, weight_3d=1e-4, huber_px=0.0, detach_target=True)
    assert xtrain.multiview_entry(parser.parse_args(['--config', 'c', '--mv-2d', '2', '--mv-huber', '3'])) == dict(
        weight_2d=2.0, weight_3d=0.0, huber_px=3.0, detach_target=False)


def test_signatures():
    from modules import util as mu
    from xas_amd import ops_eval
    p = inspect.signature(ops_eval.multiview_consistency).parameters
    assert list(p) == ['kps_xy', 'trans_image', 'world', 'pmat', 'weight', 'image_size', 'huber_px', 'detach_target']
    assert [p[n].default for n in list(p)[4:]] == [None, 256.0, 0.0, False]
    p = inspect.signature(mu.multiview_consistency_loss).parameters
    assert list(p) == ['kps_by_cam', 'world_by_cam', 'params', 'cam_id_list', 'weight_2d', 'weight_3d', 'huber_px', 'detach_target',
                       'weights']
    assert [p[n].default for n in list(p)[6:]] == [0.0, False, None]
    # the existing ones, unchanged
    p = inspect.signature(mu.batch_triangulate).parameters
    assert list(p) == ['keypoints_', 'Pall', 'robust_px'] and p['robust_px'].default is None
    p = inspect.signature(mu.triangulation).parameters
    assert list(p) == ['keypoints', 'params', 'cam_id_list', 'is_norm', 'RECT_WIDTH', 'robust_px', 'return_inliers']
    p = inspect.signature(mu.triangulation_weighted).parameters
    assert list(p) == ['keypoints', 'params', 'cam_id_list', 'weights', 'is_norm', 'RECT_WIDTH', 'robust_px', 'return_inliers', 'inputs']
    p = inspect.signature(mu.triangulation_refined).parameters
    assert list(p) == ['keypoints', 'params', 'cam_id_list', 'weights', 'is_norm', 'RECT_WIDTH', 'robust_px', 'huber_px', 'want', 'inputs']


def test_model_refuses_a_camera_count_it_cannot_triangulate():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import inputs as gi
    from modules.model import Counter3DModel
    for cams in ((0,), tuple(range(7))):
        cfg = gi.model_params('S1', cam_ids=cams)
        cfg['loss_config']['multiview_loss'] = dict(weight_2d=1.0, weight_3d=0.0)
        with pytest.raises(ValueError, match='multiview_loss triangulates over 2 to 6 cameras; cam_id_list has %d' % len(cams)):
            Counter3DModel(cfg, None, None, None, None)
    cfg = gi.model_params('S1', cam_ids=(0,))
    Counter3DModel(cfg, None, None, None, None)                       # without the key one camera is what it always was


def _names():
    import test_gpu_multiview as t
    return list(t.CASES)


@pytest.mark.parametrize('detach', [False, True], ids=['through_x', 'detached'])
@pytest.mark.parametrize('name', _names())
def test_oracle_gradient_matches_float64_autograd(name, detach):
    """torch.linalg.eigh's float64 autograd on the same loss against the analytic gradient evaluated on the SAME eigensystem
    (torch's, handed to the oracle).  Then both sides are float64 evaluations of one smooth function of one (lambda, v), and only
    the GRADIENTS say anything: reproj, depth and xyz are equal by construction.  On noisy four-view rigs the gradients agree to
    ~4e-16 to 6e-14 relative, and 1e-10 of the largest entry leaves two orders and more for the eigenvalue gaps of the other cases.
    The 1e-10 is NOT met by the oracle on its own eigensystem: numpy's eigh of the same Gram matrix, whose entries span 1e6 to
    1e13, stands 1e-10 to 3.4e-8 of the largest entry from torch's in every quantity.  That distance is the conditioning of
    the DLT in float64, not the gradient formula (central differences below cover the oracle's own eigensystem); it is held to
    1e-6 here, 30 times what was seen, on every case that compares values, and tests/test_gpu_multiview.py builds its bound on it."""
    import test_gpu_multiview as t
    import _multiview_oracle as mo
    c, g, own, _ = t.case(name, detach)
    y = mo.torch_loss(c, torch.float64, own['status'], g[0], g[1], detach)
    o = mo.run(c, g[0], g[1], detach, eig=(y['lam'], y['vec']))
    assert np.array_equal(o['status'], own['status'])
    with np.errstate(invalid='ignore'):
        cmp = (o['status'] == 0) & o['decidable'] & (o['ratio'] >= mo.RATIO_MIN) & o['gap']    # (no gap: the term is left out)
    if not cmp.any():
        assert name in t.PASSED_THROUGH or name == 'illcond'
        return
    # noise-free points: the reprojection terms are differences that cancel to ~1e-5 px, and what two float64 evaluations differ
    # by is relative to what cancels, not to what is left.  Their scale is that of the same quantity at 2 px of noise.
    scale_of = t.case('noisy_b2v4h3k5', detach)[2] if name.startswith('clean') else o
    for key in ('reproj', 'depth', 'xyz', 'grad_kps_xy', 'grad_world'):
        a, b = t.per_joint(o[key], key)[cmp], t.per_joint(y[key], key)[cmp]
        rel = np.abs(a - b).max() / np.nanmax(np.abs(scale_of[key]))
        rel_own = np.abs(t.per_joint(own[key], key)[cmp] - b).max() / np.nanmax(np.abs(scale_of[key]))
        print('%s %s: oracle vs float64 autograd %.3g relative on one eigensystem, %.3g on its own' % (name, key, rel, rel_own))
        assert not c['compare'] or rel_own <= 1e-6, (name, key, rel_own)
        assert rel <= 1e-10, (name, key, rel)
    assert np.array_equal(np.moveaxis(o['hsel'], 2, 1)[cmp], np.moveaxis(y['hsel'], 2, 1)[cmp])


def test_oracle_gradient_matches_central_differences():
    """d objective / d input by central differences in float64, for a few entries of kps_xy and world of three cases.  Two
    float64 evaluations of the objective (~10 to 100) differ by ~1e-9 relative through the DLT's conditioning (see above), so a
    step h leaves 1e-8 / 2h of rounding: h = 1e-4 in x, y (0.05 px; the loss is next to quadratic in the points, its third
    derivative comes from the perspective division alone) and 0.1 mm in world (exactly quadratic there) keep both errors below
    1e-5 of gradients of the size met here."""
    import test_gpu_multiview as t
    import _multiview_oracle as mo
    for name in ('noisy_b2v4h3k5', 'weighted', 'huber_off'):       # (Huber's rho is not next to quadratic: the autograd test has it)
        c, g, o, _ = t.case(name, False)
        c64 = dict(c, kps_xy=c['kps_xy'].astype(np.float64), world=c['world'].astype(np.float64))
        for key, idx, h in (('kps_xy', (0, 1, 2, 0), 1e-4), ('kps_xy', (1, 3, 4, 1), 1e-4), ('world', (0, 2, int(o['hsel'][0, 2, 3]), 3, 1), 1e-1)):
            f = []
            for s in (h, -h):
                moved = dict(c64, **{key: c64[key].copy()})
                moved[key][idx] += s
                f.append(mo.objective(moved, g[0], g[1]))
            fd = (f[0] - f[1]) / (2 * h)
            an = o['grad_' + key][idx]
            print('%s d/d%s%s: analytic %.9g, central differences %.9g' % (name, key, list(idx), an, fd))
            assert abs(fd - an) <= 1e-5 * abs(an), (name, key, idx, fd, an)


@pytest.mark.parametrize('name', _names())
def test_gpu_case_inputs_are_well_conditioned(name):
    """Every case of the GPU file: every compared joint has lambda_1 / lambda_0 >= 50 and a decidable hypothesis choice; no case
    but the one built to be degenerate excludes a solved joint, and that one excludes all of its joints."""
    import test_gpu_multiview as t
    import _multiview_oracle as mo
    c, g, o, _ = t.case(name)
    solved = o['status'] == 0
    cmp = t.compared(name)
    excluded = solved & ~cmp
    print('%s: %d joints, %d passed through, %d excluded, lambda_1 / lambda_0 min %.3g' % (
        name, solved.size, (~solved).sum(), excluded.sum(), np.nanmin(o['ratio']) if solved.any() else np.nan))
    assert (o['ratio'][cmp] >= mo.RATIO_MIN).all() and o['decidable'][cmp].all()
    if name == 'illcond':
        assert excluded.all() or not solved.any()
        assert not cmp.any() and o['ratio'][solved].min() < mo.RATIO_MIN / 10
    else:
        assert not excluded.any(), 'share excluded: %.3g' % excluded.mean()
    assert solved.all() != (name in t.PASSED_THROUGH or name == 'nan_point')
    if name in t.PASSED_THROUGH:
        assert not solved.any()
    if name == 'nan_point':
        assert (~solved).sum() == 1 and not solved[0, 2]
    if name == 'clean_b2v4h3k5':
        assert np.abs(o['xyz'] - c['planted']).max() < 1e-2 and o['reproj'].max() < 1e-6
    if name.startswith('noisy'):
        assert 1.0 < o['reproj'].mean() < 4 * 2 * t_sigma() ** 2
    if name == 'weighted':
        w = c['weight']
        assert 9.0 < w.max() / w.min() < 12.0
    if name == 'huber':
        assert (o['reproj'] < t.case('huber_off')[2]['reproj']).all()
    if name != "illcond":
        assert (o["hsel"][np.broadcast_to(solved[:, None], o["hsel"].shape)] == 0).all()          # the planted hypothesis is index 0


def t_sigma():
    from _refine_inputs import SIGMA_PX
    return SIGMA_PX
