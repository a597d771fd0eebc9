"""The averaged-weights optimizer step in the C ABI, without a GPU: the two entry points are exported by the built library,
declared in include/xas_hip.h and bound by the ctypes table; the argument checks answer before any launch; the constructor
option of FusedAdam."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('xas_adam_step_ema', 'xas_adam_step_guarded_ema')


def _header():
    return open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()


@pytest.mark.parametrize('name', NAMES)
def test_symbol_is_exported_declared_and_bound(name):
    from xas_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name), 'library does not export %s' % name
    decl = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, _header())
    assert decl, 'include/xas_hip.h does not declare %s' % name
    assert name in _lib.SIGNATURES
    f = _lib.fn(name)
    assert len(f.argtypes) == len(_lib.SIGNATURES[name][0]) == len(decl.group(1).split(','))


def test_argument_checks_return_errors_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)                       # any aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    nan = float('nan')
    a = _lib.fn('xas_adam_step_ema')
    #        p    g    m    v    ema  n  lr    b1   b2     eps  step decay  1-decay stream
    assert a(one, one, one, one, None, 8, 1e-3, 0.5, 0.999, 1e-8, 1, 0.999, 0.001, None) == 1 and 'shadow arena (ema) is null' in err()
    for n in (6, 0, -4):
        assert a(one, one, one, one, one, n, 1e-3, 0.5, 0.999, 1e-8, 1, 0.999, 0.001, None) == 1 and 'multiple of 4' in err()
    for decay in (1.0, -0.1, 1.5, nan):
        assert a(one, one, one, one, one, 8, 1e-3, 0.5, 0.999, 1e-8, 1, decay, 0.001, None) == 1 and 'decay' in err()
    g = _lib.fn('xas_adam_step_guarded_ema')
    #        p    g    m    v    ema  n  b1   b2     eps   decay  1-decay guard stream
    assert g(one, one, one, one, None, 8, 0.5, 0.999, 1e-8, 0.999, 0.001, one, None) == 1 and 'shadow arena (ema) is null' in err()
    for n in (6, 0, -4):
        assert g(one, one, one, one, one, n, 0.5, 0.999, 1e-8, 0.999, 0.001, one, None) == 1 and 'multiple of 4' in err()
    for decay in (1.0, -0.1, 1.5, nan):
        assert g(one, one, one, one, one, 8, 0.5, 0.999, 1e-8, decay, 0.001, one, None) == 1 and 'decay' in err()
    assert g(one, one, one, one, one, 8, 0.5, 0.999, 1e-8, 0.999, 0.001, None, None) == 1 and 'guard record is null' in err()


def test_constructor_option_needs_no_gpu():
    import torch
    from xas_amd.optim import FusedAdam
    p = [torch.nn.Parameter(torch.zeros(3))]
    assert FusedAdam(p).ema_arena is None and FusedAdam(p).ema_decay is None
    assert FusedAdam(p, max_grad_norm=1.0, skip_nonfinite=True).ema_arena is None
    for guard in ({}, {'max_grad_norm': 1.0}, {'skip_nonfinite': True}, {'max_grad_norm': 1.0, 'skip_nonfinite': True}):
        o = FusedAdam(p, ema_decay=0.999, **guard)
        assert o.ema_decay == 0.999 and o.guarded == bool(guard)
    assert FusedAdam(p, ema_decay=0.0).ema_decay == 0.0
    for bad in (1.0, -0.1, float('nan')):
        with pytest.raises(ValueError):
            FusedAdam(p, ema_decay=bad)


def test_the_factors_handed_to_the_kernel():
    """decay as fp32, and 1 - decay rounded once from double."""
    import numpy as np
    import torch
    from xas_amd.optim import FusedAdam
    p = [torch.nn.Parameter(torch.zeros(3))]
    for decay in (0.999, 0.5, 0.0, 0.9999):
        d, omd = FusedAdam(p, ema_decay=decay)._ema_factors
        assert d == float(np.float32(decay)) and omd == float(np.float32(1.0 - float(np.float32(decay))))
    assert FusedAdam(p, ema_decay=0.0)._ema_factors == (0.0, 1.0)
    assert FusedAdam(p)._ema_factors is None


def test_abi_version_is_unchanged():
    from xas_amd import _lib
    assert _lib.fn('xas_abi_version')() == 3 == _lib.ABI_VERSION
