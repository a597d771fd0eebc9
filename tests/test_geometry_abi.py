"""The patch->world, line-mask and mask-loss entry points of csrc/geometry.hip and csrc/losses.hip in the C ABI, without a GPU:
they are exported by the built library, declared in include/xas_hip.h and bound by the ctypes table; the two block-count
queries state the launch geometry the kernels use; every bad-argument call answers 1 with a message before any launch
(xas_draw_lines_max_bwd checks what xas_draw_lines_max_fwd checks, body_width included)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('xas_patch_to_world_fwd', 'xas_patch_to_world_bwd', 'xas_draw_lines_max_fwd', 'xas_draw_lines_max_bwd',
         'xas_lines_nblk', 'xas_mask_loss_fwd', 'xas_mask_loss_bwd', 'xas_loss_nblk')
GEO_NORM, GEO_MONO, GEO_PATCH, GEO_IMAGE = 1, 2, 4, 8


def _header():
    return open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()


@pytest.mark.parametrize('name', NAMES)
def test_symbol_is_exported_declared_and_bound(name):
    from xas_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name), 'library does not export %s' % name
    m = re.search(r'\b(int|size_t)\s+%s\s*\(([^)]*)\)' % name, _header())
    assert m, 'include/xas_hip.h does not declare %s' % name
    assert name in _lib.SIGNATURES
    f = _lib.fn(name)
    assert len(f.argtypes) == len(_lib.SIGNATURES[name][0]) == len(m.group(2).split(',')), 'arity of %s' % name


def test_geometry_flags_equal_the_header():
    from xas_amd import ops_head
    src = _header()
    for flag, value in (('XAS_GEO_NORM', GEO_NORM), ('XAS_GEO_MONO', GEO_MONO), ('XAS_GEO_PATCH', GEO_PATCH),
                        ('XAS_GEO_IMAGE', GEO_IMAGE)):
        assert '#define %s %d' % (flag, value) in src
        assert getattr(ops_head, flag[4:]) == value


@pytest.mark.parametrize('S', [2, 3, 5, 31, 32, 33, 64, 256])
def test_lines_nblk_is_one_block_per_1024_pixels(S):
    """256 threads x 4 pixels"""
    from xas_amd import _lib
    assert _lib.query('xas_lines_nblk', S) == -(-S * S // 1024)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 4095, 4096, 4097, 4096 * 256, 4096 * 256 + 1, 32 * 256 * 256, 3 * 2 ** 31 + 1])
def test_loss_nblk_is_one_block_per_4096_elements(n):
    """256 threads x 16 elements; n is a long"""
    from xas_amd import _lib
    assert _lib.query('xas_loss_nblk', n) == -(-n // 4096)


ONE = ctypes.c_void_p(64)               # any aligned non-null pointer: never dereferenced on these paths


def _refused(f, args, word):
    from xas_amd import _lib
    lib = _lib.load()
    assert f(*args, None) == 1, args
    msg = lib.xas_last_error().decode()
    assert word in msg, (args, msg)


def _with(args, **kw):
    """args as an ordered dict -> tuple with some replaced"""
    d = dict(args)
    for k, v in kw.items():
        assert k in d
        d[k] = v
    return tuple(d.values())


_ids = lambda d: ','.join('%s=%s' % kv for kv in d.items())

P2W_FWD = (('kps', ONE), ('trans_image', ONE), ('k_mat', ONE), ('pelvis', ONE), ('rot_world', ONE), ('trans_world', ONE),
           ('B', 2), ('Hy', 3), ('K', 18), ('image_size', 256.0), ('rect_width', 2000.0), ('flags', GEO_NORM | GEO_PATCH),
           ('world', ONE))
P2W_BWD = (('kps', ONE), ('grad_world', ONE)) + P2W_FWD[1:12] + (('grad_kps', ONE),)
P2W_BAD = [dict(kps=None), dict(trans_image=None), dict(pelvis=None), dict(k_mat=None), dict(rot_world=None),
           dict(trans_world=None), dict(B=0), dict(Hy=0), dict(K=0), dict(B=-1), dict(K=-3)]


@pytest.mark.parametrize('bad', P2W_BAD + [dict(world=None), dict(flags=GEO_NORM | GEO_PATCH | GEO_IMAGE, kps=None),
                                           dict(flags=GEO_PATCH | GEO_IMAGE, k_mat=None, rot_world=None, trans_world=None,
                                                trans_image=None)], ids=_ids)
def test_patch_to_world_forward_refuses(bad):
    """(the image mode may leave the intrinsics and extrinsics out, but nothing else)"""
    from xas_amd import _lib
    _refused(_lib.fn('xas_patch_to_world_fwd'), _with(P2W_FWD, **bad), 'patch_to_world')


@pytest.mark.parametrize('bad', P2W_BAD + [dict(grad_world=None), dict(grad_kps=None), dict(flags=GEO_IMAGE),
                                           dict(flags=GEO_NORM | GEO_PATCH | GEO_IMAGE)], ids=_ids)
def test_patch_to_world_backward_refuses(bad):
    """what the forward refuses, and the forward-only image mode"""
    from xas_amd import _lib
    _refused(_lib.fn('xas_patch_to_world_bwd'), _with(P2W_BWD, **bad), 'patch_to_world bwd')


LINES_FWD = (('kps', ONE), ('kp_stride_b', 36), ('kp_stride_j', 2), ('B', 2), ('K', 18), ('parents', ONE), ('children', ONE),
             ('L', 25), ('fine_mask', 0), ('body_width', 3.0e-3), ('S', 64), ('mask', ONE))
LINES_BWD = LINES_FWD[:11] + (('grad_mask', ONE), ('partial', ONE), ('grad_kps_xy', ONE))
# what both directions must refuse
LINES_BAD = [dict(kps=None), dict(parents=None), dict(children=None), dict(L=0), dict(L=33), dict(L=-1), dict(K=0), dict(K=65),
             dict(S=1), dict(S=0), dict(B=0), dict(body_width=0.0), dict(body_width=-3.0e-3), dict(body_width=float('nan'))]


@pytest.mark.parametrize('bad', LINES_BAD + [dict(mask=None)], ids=_ids)
def test_draw_lines_forward_refuses(bad):
    from xas_amd import _lib
    _refused(_lib.fn('xas_draw_lines_max_fwd'), _with(LINES_FWD, **bad), 'draw_lines')


@pytest.mark.parametrize('bad', LINES_BAD + [dict(grad_mask=None), dict(partial=None), dict(grad_kps_xy=None)], ids=_ids)
def test_draw_lines_backward_refuses_what_the_forward_refuses(bad):
    from xas_amd import _lib
    _refused(_lib.fn('xas_draw_lines_max_bwd'), _with(LINES_BWD, **bad), 'draw_lines bwd')


LOSS_FWD = (('m', ONE), ('gt', ONE), ('weight', ONE), ('n', 4097), ('mode', 3), ('partial', ONE), ('out', ONE))
LOSS_BWD = LOSS_FWD[:5] + (('out', ONE), ('grad_scalar', ONE), ('dm', ONE))
LOSS_BAD = [dict(m=None), dict(gt=None), dict(out=None), dict(n=0), dict(n=-1), dict(mode=2, weight=None),
            dict(mode=3, weight=None)]


@pytest.mark.parametrize('bad', LOSS_BAD + [dict(partial=None)], ids=_ids)
def test_mask_loss_forward_refuses(bad):
    from xas_amd import _lib
    _refused(_lib.fn('xas_mask_loss_fwd'), _with(LOSS_FWD, **bad), 'mask_loss')


@pytest.mark.parametrize('bad', LOSS_BAD + [dict(grad_scalar=None), dict(dm=None)], ids=_ids)
def test_mask_loss_backward_refuses(bad):
    from xas_amd import _lib
    _refused(_lib.fn('xas_mask_loss_bwd'), _with(LOSS_BWD, **bad), 'mask_loss bwd')
