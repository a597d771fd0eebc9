"""The C-ABI library loads and exports every symbol declared in include/xas_hip.h, and the ctypes
signature table matches the header.  No compute calls (CPU-only test)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_prototypes():
    src = open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    protos = {}
    for m in re.finditer(r'\b(int|size_t|const char\*)\s+(xas_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S):
        ret, name, args = m.groups()
        codes = ''
        args = args.strip()
        if args and args != 'void':
            for a in args.split(','):
                a = a.strip()
                if 'xas_conv_shape' in a:
                    codes += 's'
                elif '*' in a:
                    codes += 'p'
                elif re.match(r'(const\s+)?unsigned\b', a):
                    codes += 'u'
                elif re.match(r'(const\s+)?long\b', a):
                    codes += 'l'
                elif re.match(r'(const\s+)?int\b', a):
                    codes += 'i'
                elif re.match(r'(const\s+)?float\b', a):
                    codes += 'f'
                elif re.match(r'(const\s+)?double\b', a):
                    codes += 'd'
                elif re.match(r'(const\s+)?size_t\b', a):
                    codes += 'z'
                else:
                    raise AssertionError('unparsed argument %r in %s' % (a, name))
        protos[name] = (codes, {'int': 'i', 'size_t': 'z', 'const char*': 'c'}[ret])
    return protos


def test_library_is_built():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build_lib(verbose=False)
    assert os.path.exists(ge.LIB)


def test_exports_and_signatures():
    import ctypes
    from xas_amd import _lib
    lib = _lib.load()
    protos = header_prototypes()
    assert len(protos) > 30
    for name, (codes, ret) in protos.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        if name == 'xas_last_error':
            continue
        assert name in _lib.SIGNATURES, 'no ctypes signature for %s' % name
        assert _lib.SIGNATURES[name] == (codes, ret), '%s: table %r vs header %r' % (name, _lib.SIGNATURES[name], (codes, ret))
    assert set(_lib.SIGNATURES) <= set(protos)
    assert ctypes.sizeof(_lib.ConvShape) == 12 * 4 + 16 and _lib.ConvShape.grad_amax.offset == 48 and _lib.ConvShape.x_amax.offset == 56      # 12 ints + the two operand-maximum pointers
    assert lib.xas_abi_version() == 3
    # recorded maxima: the slot layout of the header is the one the Python side allocates
    import re
    from xas_amd import ops_nn
    src = open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()
    sub, stride = (int(re.search(r'#define %s (\d+)' % n, src).group(1)) for n in ('XAS_AMAX_SUB', 'XAS_AMAX_STRIDE'))
    assert sub * stride == ops_nn.AMAX_SLOT_FLOATS and stride * 4 == 128


def test_tuning_flags_match_the_header():
    """Every XAS_TUNE_* of the header has an equal _lib.TUNE_*, and the reverse."""
    from xas_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    header = {}
    for name, base, shift in re.findall(r'\bXAS_(TUNE_\w+)\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*[,}\n]', src):
        header[name] = int(base) << int(shift or 0)
    mirror = {k: v for k, v in vars(_lib).items() if k.startswith('TUNE_')}
    assert len(header) >= 10 and len(header) == len(re.findall(r'\bXAS_TUNE_\w+\s*=', src))
    assert header == mirror


def test_plan_tables_match_the_header():
    """The field, route and kernel names of _lib's xas_conv_igemm_plan wrapper are the header's enums, in the header's order."""
    from xas_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'xas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)

    def enum(prefix):
        return {n.lower(): int(v) for n, v in re.findall(r'\bXAS_%s_(\w+)\s*=\s*(\d+)' % prefix, src)}
    fields = enum('PLAN')
    assert fields.pop('ints') == len(_lib.PLAN_FIELDS)
    assert fields == {n: i for i, n in enumerate(_lib.PLAN_FIELDS)}
    assert enum('ROUTE') == {n: i for i, n in enumerate(_lib.PLAN_ROUTES) if n}
    assert enum('KERNEL') == {n: i for i, n in enumerate(_lib.PLAN_KERNELS) if n}


def test_igemm_plan_answers_without_a_gpu():
    """xas_conv_igemm_plan never touches the device: one shape per route, the refusals, and the fields that do not apply."""
    import ctypes
    from xas_amd import _lib
    lib = _lib.load()
    f = _lib.fn('xas_conv_igemm_plan')
    out = (ctypes.c_int * len(_lib.PLAN_FIELDS))()
    outp = ctypes.cast(out, ctypes.c_void_p)
    good = _lib.ConvShape(2, 8, 8, 32, 32, 3, 3, 1, 1, 8, 8, 1 + _lib.PREC_F32)
    assert f(None, 0, 0, outp) == 1 and 'null shape' in lib.xas_last_error().decode()
    assert f(ctypes.byref(good), 0, 0, None) == 1 and f(ctypes.byref(good), 2, 0, outp) == 1
    assert 'conv_igemm_plan' in lib.xas_last_error().decode()
    bad = _lib.ConvShape(2, 8, 8, 0, 32, 3, 3, 1, 1, 8, 8)
    assert f(ctypes.byref(bad), 0, 0, outp) == 1
    assert f(ctypes.byref(_lib.ConvShape(2, 8, 8, 32, 32, 3, 3, 1, 1, 7, 8)), 0, 0, outp) == 1 and 'inconsistent' in lib.xas_last_error().decode()
    assert f(ctypes.byref(_lib.ConvShape(2, 7, 8, 32, 32, 3, 3, 1, 1, 8, 8)), 1, 0, outp) == 1 and 'too small' in lib.xas_last_error().decode()
    prec = _lib.query('xas_get_precision')
    try:
        _lib.query('xas_set_tuning', 0)
        p = _lib.conv_igemm_plan(good, 0)
        assert p == dict(route='mfma', kernel='igemm_buf', bm=128, bn=32, pipelined=1, phases=1, pieces=0, patch_width=0, tpb=0, images=2)
        p = _lib.conv_igemm_plan(_lib.ConvShape(2, 8, 8, 32, 32, 3, 3, 1, 1, 8, 8, 1 + _lib.PREC_BF16X6), 1)
        assert (p['kernel'], p['bn'], p['pieces'], p['patch_width'], p['pipelined']) == ('igemm_x6t', 32, 3, 8, 0)
        stem = _lib.ConvShape(1, 16, 32, 3, 64, 7, 7, 2, 3, 8, 16, 1 + _lib.PREC_F32)
        assert _lib.conv_igemm_plan(stem, 0)['route'] == 'stem_f32' and _lib.conv_igemm_plan(stem, 0, True)['route'] == 'direct'
        assert _lib.conv_igemm_plan(stem, 1) == dict(route='direct', kernel=None, bm=0, bn=0, pipelined=0, phases=0, pieces=0,
                                                     patch_width=0, tpb=0, images=1)
        thin = _lib.ConvShape(1, 3, 5, 4, 1, 3, 3, 1, 1, 3, 5)
        assert _lib.conv_igemm_plan(thin, 0)['route'] == 'thin_vec_to_scalar' and _lib.conv_igemm_plan(thin, 1)['route'] == 'thin_scalar_to_vec'
        # stride 2: four phases in the data gradient, one in the forward; the tuning flags are read at the time of the query
        s2 = _lib.ConvShape(2, 17, 13, 128, 128, 3, 3, 2, 1, 9, 7, 1 + _lib.PREC_F32)
        assert _lib.conv_igemm_plan(s2, 1)['phases'] == 4 and _lib.conv_igemm_plan(s2, 0)['phases'] == 1
        _lib.query('xas_set_tuning', _lib.TUNE_GLOBAL_LOAD | _lib.TUNE_PLAIN_KLOOP)
        p = _lib.conv_igemm_plan(s2, 1)
        assert (p['kernel'], p['pipelined']) == ('igemm', 0)
    finally:
        _lib.query('xas_set_tuning', 0)                 # (the library has no getter: 0 is what every test starts from and leaves)
    assert _lib.query('xas_get_precision') == prec


def test_no_cpu_fallback():
    import torch
    from xas_amd import ops_head
    with pytest.raises(RuntimeError):
        ops_head.softargmax_multi(torch.zeros(1, 32, 16, 16), 2, 3, 15)


def test_argument_checks_return_errors_without_a_gpu():
    """Every entry point validates its arguments BEFORE touching the device: status 1 and a message, no launch."""
    import ctypes
    from xas_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                       # any non-null pointer: never dereferenced on these paths
    err = lambda: lib.xas_last_error().decode()
    f = _lib.fn
    assert f('xas_eval_select')(one, one, one, 2, 3, 65, 3, 256.0, 0, None, None, None, None, None) == 1
    assert 'K <= 64' in err()
    assert f('xas_eval_select')(one, one, one, 2, 3, 18, 4, 256.0, 0, None, None, None, None, None) == 1
    assert f('xas_triangulate_dlt')(one, one, 2, 1, 18, one, None) == 1 and '2 views' in err()
    assert f('xas_pose_metrics')(one, one, None, 2, 2, 1.0, 0, 0.15, None, None, None, None, None) == 1
    assert f('xas_pose_metrics')(one, one, None, 2, 18, 1.0, 3, 0.15, None, None, None, None, None) == 1
    assert f('xas_projection_matrix')(None, one, one, 2, one, None) == 1
    shp = _lib.ConvShape(2, 8, 8, 3, 64, 3, 3, 1, 1, 8, 8)         # Cin = 3: not on the accumulating MFMA path
    assert f('xas_conv_dgrad_acc')(one, one, one, ctypes.byref(shp), None) == 1 and 'MFMA path' in err()
    assert f('xas_bn_bwd_reduce')(None, None, one, one, one, None, None, 1e-5, 1, 64, 64, 1, one, one, None, None, None, None) == 1
    assert f('xas_bn_bwd_apply')(None, one, one, one, one, one, None, one, 1e-5, 1, 64, 64, 1, 64.0, one, None, None, None) == 1
    assert 'invertible' in err().lower() or 'null buffer' in err()
