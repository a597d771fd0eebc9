"""The discriminator and joint-loss entry points of csrc/gcn.hip and csrc/losses.hip in the C ABI, without a GPU: they are exported by the
built library, declared in include/xas_hip.h and bound by the ctypes table; the graph-LayerNorm workspace query states the
layout that the forward and the backward carve out of it; every bad-argument call answers 1 with a message before any
launch (xas_pose_loss_bwd checks what xas_pose_loss_fwd checks)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('xas_graph_aggregate', 'xas_gln_workspace_floats', 'xas_gln_fwd', 'xas_gln_bwd', 'xas_pose_loss_fwd',
         'xas_pose_loss_bwd', 'xas_lsgan_fwd', 'xas_lsgan_bwd')


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


@pytest.mark.parametrize('n,nblk', [(1, 1), (2048, 1), (2049, 2), (131072, 64), (131073, 64)])
def test_gln_workspace_layout(n, nblk):
    """One (sum, sum of squares) pair per partial block and group for the forward - blocks of 256 threads x 8 elements,
    capped at 64 - and for the backward [G][2][C] channel sums followed by [G][2] scalars; 8 floats of slack.  The two
    passes use the same buffer from its start, so the query covers the larger and, as it is written, their sum."""
    from xas_amd import _lib
    q = _lib.fn('xas_gln_workspace_floats')
    for G, C in ((1, 1), (5, 128), (65, 5), (9, 64), (2, 300)):
        fwd = G * nblk * 2
        bwd = G * 2 * C + G * 2
        assert q(n, G, C) == G * (2 * nblk + 2 + 2 * C) + 8 == fwd + bwd + 8
        assert q(n, G, C) >= max(fwd, bwd)


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


POSE_FWD = (('pred', ONE), ('gt', ONE), ('B', 4), ('Hy', 3), ('K', 18), ('kind', 1), ('w0', 1.0), ('w1', 1.0), ('w2', 0.0),
            ('out', ONE))
POSE_BWD = POSE_FWD + (('grad_scalar', ONE), ('grad_pred', ONE), ('grad_aux', None))
# what both directions must refuse
POSE_BAD = [dict(pred=None), dict(out=None), dict(kind=-1), dict(kind=3), dict(kind=0, gt=None), dict(kind=1, K=16),
            dict(kind=2, K=16), dict(Hy=0), dict(Hy=7), dict(B=0), dict(B=-2), dict(kind=0, K=0), dict(K=-1)]


@pytest.mark.parametrize('bad', POSE_BAD, ids=lambda d: ','.join('%s=%s' % kv for kv in d.items()))
def test_pose_loss_forward_refuses(bad):
    from xas_amd import _lib
    _refused(_lib.fn('xas_pose_loss_fwd'), _with(POSE_FWD, **bad), 'pose_loss')


@pytest.mark.parametrize('bad', POSE_BAD + [dict(grad_scalar=None), dict(grad_pred=None)],
                         ids=lambda d: ','.join('%s=%s' % kv for kv in d.items()))
def test_pose_loss_backward_refuses_what_the_forward_refuses(bad):
    from xas_amd import _lib
    _refused(_lib.fn('xas_pose_loss_bwd'), _with(POSE_BWD, **bad), 'pose_loss bwd')


def test_gln_graph_aggregate_and_lsgan_refuse_null_and_non_positive():
    from xas_amd import _lib
    agg = (('x', ONE), ('adj', ONE), ('B', 2), ('N', 18), ('C', 128), ('y', ONE))
    for bad in (dict(x=None), dict(adj=None), dict(y=None), dict(B=0), dict(N=0), dict(C=0), dict(B=-1), dict(N=-1), dict(C=-1)):
        _refused(_lib.fn('xas_graph_aggregate'), _with(agg, **bad), 'graph_aggregate')
    fwd = (('x', ONE), ('gamma', ONE), ('beta', ONE), ('residual', None), ('rows', 36), ('C', 128), ('groups', 2), ('eps', 1e-5),
           ('y', ONE), ('stats', ONE), ('workspace', ONE))
    for bad in (dict(x=None), dict(gamma=None), dict(beta=None), dict(y=None), dict(stats=None), dict(workspace=None),
                dict(rows=0), dict(C=0), dict(groups=0), dict(rows=-3), dict(C=-1), dict(groups=-1)):
        _refused(_lib.fn('xas_gln_fwd'), _with(fwd, **bad), 'gln_fwd')
    bwd = (('x', ONE), ('beta', ONE), ('dy', ONE), ('gamma', ONE), ('stats', ONE), ('rows', 36), ('C', 128), ('groups', 2),
           ('eps', 1e-5), ('dx', ONE), ('dgamma', ONE), ('dbeta', ONE), ('workspace', ONE))
    for bad in (dict(x=None), dict(beta=None), dict(dy=None), dict(gamma=None), dict(stats=None), dict(dx=None), dict(dgamma=None),
                dict(dbeta=None), dict(workspace=None), dict(rows=0), dict(C=0), dict(groups=0), dict(rows=-3), dict(C=-1),
                dict(groups=-1)):
        _refused(_lib.fn('xas_gln_bwd'), _with(bwd, **bad), 'gln_bwd')
    lf = (('logits', ONE), ('B', 4), ('Hy', 3), ('target', 1.0), ('out', ONE), ('idx', ONE))
    for bad in (dict(logits=None), dict(out=None), dict(idx=None), dict(B=0), dict(Hy=0), dict(B=-1), dict(Hy=-1)):
        _refused(_lib.fn('xas_lsgan_fwd'), _with(lf, **bad), 'lsgan')
    lb = (('logits', ONE), ('B', 4), ('Hy', 3), ('target', 1.0), ('idx', ONE), ('grad_scalar', ONE), ('grad_logits', ONE))
    for bad in (dict(logits=None), dict(idx=None), dict(grad_scalar=None), dict(grad_logits=None), dict(B=0), dict(Hy=0),
                dict(B=-1), dict(Hy=-1)):
        _refused(_lib.fn('xas_lsgan_bwd'), _with(lb, **bad), 'lsgan bwd')
