"""The guarded optimizer step in the C ABI, without a GPU: the three entry points are exported by the built library, declared
in include/xas_hip.h and bound by the ctypes table; the workspace query and the argument checks answer before any launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('xas_grad_guard_workspace_bytes', 'xas_grad_guard', 'xas_adam_step_guarded')


def _header():
    return open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()


@pytest.mark.parametrize('name', NAMES)
def test_symbol_is_exported_declared_and_bound(name):
    from xas_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name), 'library does not export %s' % name
    assert re.search(r'\b(int|size_t)\s+%s\s*\(' % name, _header()), 'include/xas_hip.h does not declare %s' % name
    assert name in _lib.SIGNATURES
    f = _lib.fn(name)
    assert len(f.argtypes) == len(_lib.SIGNATURES[name][0])


def test_guard_record_size_matches_the_header():
    from xas_amd import _lib
    assert int(re.search(r'#define XAS_GUARD_FLOATS (\d+)', _header()).group(1)) == _lib.GUARD_FLOATS == 8
    words = (_lib.GUARD_NORM, _lib.GUARD_SCALE, _lib.GUARD_SKIP, _lib.GUARD_T, _lib.GUARD_SKIPPED, _lib.GUARD_STEP_SIZE,
             _lib.GUARD_INV_SQRT_BC2, _lib.GUARD_NONFINITE)
    assert words == tuple(range(8))
    block = _header()
    block = block[block.index('Guard record:'):block.index('#define XAS_GUARD_FLOATS')]
    for i, field in enumerate(('norm', 'scale', 'skip', 't', 'skipped', 'step_size', 'inv_sqrt_bc2', 'nonfinite')):
        assert re.search(r'word %d\s+(float|int)\s+%s\b' % (i, field), block), (i, field)


def test_workspace_query():
    """One double and one flag word per block of the norm pass: blocks of 256 threads x one float4, capped at 4096."""
    from xas_amd import _lib
    q = _lib.fn('xas_grad_guard_workspace_bytes')
    assert q(4) == 12 and q(1024) == 12 and q(1028) == 24
    assert q(4096 * 256 * 4) == q(4096 * 256 * 4 + 4) == q(1 << 33) == 4096 * 12
    assert q(0) == 0 and q(-4) == 0 and q(6) == 0


def test_argument_checks_return_errors_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)                       # any aligned non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    g = _lib.fn('xas_grad_guard')
    assert g(one, 6, 1.0, 1, 1e-3, 0.5, 0.999, one, one, None) == 1 and 'multiple of 4' in err()
    assert g(None, 8, 1.0, 1, 1e-3, 0.5, 0.999, one, one, None) == 1
    assert g(one, 8, 1.0, 1, 1e-3, 0.5, 0.999, None, one, None) == 1
    assert g(one, 8, 1.0, 1, 1e-3, 0.5, 0.999, one, None, None) == 1
    assert g(one, 8, 1.0, 1, 1e-3, 0.5, 0.999, one, ctypes.c_void_p(68), None) == 1 and 'aligned' in err()
    a = _lib.fn('xas_adam_step_guarded')
    assert a(one, one, one, one, 6, 0.5, 0.999, 1e-8, one, None) == 1 and 'multiple of 4' in err()
    assert a(one, one, one, one, 8, 0.5, 0.999, 1e-8, None, None) == 1
    assert a(None, one, one, one, 8, 0.5, 0.999, 1e-8, one, None) == 1


def test_constructor_options_need_no_gpu():
    import torch
    from xas_amd.optim import FusedAdam
    p = [torch.nn.Parameter(torch.zeros(3))]
    assert not FusedAdam(p).guarded and FusedAdam(p).grad_norm is None and FusedAdam(p).skipped_steps is None
    assert FusedAdam(p, max_grad_norm=1.0).guarded and FusedAdam(p, skip_nonfinite=True).guarded
    assert not FusedAdam(p, max_grad_norm=float('inf')).guarded           # clip_grad_norm_(inf) clips nothing
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            FusedAdam(p, max_grad_norm=bad)
