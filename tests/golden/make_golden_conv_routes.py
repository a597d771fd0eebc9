#!/usr/bin/env python3
"""Generate tests/golden/conv_routes.json: what the host-side queries of csrc/conv.hip answer for a table of shapes.

The queries (xas_conv_kernel_class, xas_conv_weight_planes, the *_workspace_floats sizes, xas_conv_fwd_head_chunks) never
touch the device, so this runs on a machine without a GPU.  The file is a record of the dispatch rules at the time it was
written: a change that is meant to leave routing alone must reproduce it (tests/test_conv_routes.py), a change that moves a
shape to another kernel regenerates it and shows the moved entries in its diff.
Run:  python tests/golden/make_golden_conv_routes.py        (on a built tree; XAS_HIP_LIB selects another build)

A case = shape x precision x operand maxima x tuning flag; per case the record is
  [class(0), class(1), class(2), planes(0), planes(1), wgrad_ws, head_chunks(K of the shape), head_chunks(K = 17),
   fwd_bnstats_ws(G) for G in GROUPS, dgrad_bn_bwd_ws(G) for G in GROUPS]."""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'conv_routes.json')

# (N, Hi, Wi, Cin, Cout, R, S, stride, pad); Ho / Wo follow from them
_SHAPES_3x3 = [            # 3x3 stride 1 pad 1: (N, H, W, Cin, Cout)
    (2, 32, 32, 4, 1), (2, 32, 32, 64, 1), (2, 32, 32, 12, 1), (2, 32, 32, 68, 1),     # thin Cout == 1: C = 4, 64; 256 % (C / 4) != 0; C > 64
    (2, 32, 32, 1, 32), (2, 32, 32, 1, 64), (2, 32, 32, 1, 6),                            # thin Cin == 1; C % 4 != 0
    (2, 32, 32, 3, 16), (2, 32, 32, 32, 8), (2, 32, 32, 16, 32), (2, 32, 32, 32, 18),     # direct forward / data gradient; Cout % 4 != 0
    (2, 32, 32, 48, 50), (2, 32, 32, 32, 12),
    (2, 16, 16, 32, 64), (2, 16, 16, 32, 32), (2, 16, 16, 64, 128), (2, 16, 16, 36, 64),  # tap re-use: 64, 32 and 128 output channels; Cin % 32 != 0
    (2, 8, 8, 64, 64), (3, 8, 8, 64, 64), (4, 8, 8, 32, 32), (2, 8, 8, 512, 512),         # W == 8: N even, N odd
    (2, 12, 16, 64, 64), (2, 16, 24, 64, 64),                                             # H % 8 != 0; W % 16 != 0
    (2, 4, 4, 64, 64), (8, 4, 8, 64, 64),                                                 # 31 / Wo + 1 > Ho: the carry condition fails
    (8, 64, 64, 64, 32), (9, 64, 64, 64, 32), (8, 64, 64, 64, 64), (9, 64, 64, 64, 64),   # pick_tile bands at 256 / 288 blocks of 128 rows
    (8, 64, 64, 64, 128), (9, 64, 64, 64, 128), (8, 64, 64, 64, 96), (9, 64, 64, 64, 48),
    (16, 64, 64, 64, 256), (16, 32, 32, 128, 512),                                        # Cout % 256 == 0 at large M
    (700, 64, 64, 256, 256), (600, 64, 64, 32, 256), (600, 64, 64, 256, 32),              # image ranges: every pass / the gradient side / the input side
]
_SHAPES_1x1 = [            # 1x1 stride 1 pad 0
    (2, 32, 32, 32, 1),                                                                   # Cout == 1 that is not thin
    (2, 64, 64, 64, 256), (2, 64, 64, 256, 64), (64, 64, 64, 64, 256), (64, 64, 64, 256, 64),
    (8, 64, 64, 64, 40), (9, 64, 64, 64, 40), (8, 64, 64, 64, 80), (9, 64, 64, 64, 80),   # pick_tile bands
    (8, 64, 64, 64, 128), (9, 64, 64, 64, 128), (9, 64, 64, 96, 384),
    (2, 16, 16, 32, 64), (2, 16, 16, 32, 128), (6, 64, 64, 32, 256), (2, 8, 8, 32, 64),   # statistics epilogue: each tile height, and rows per group below a tile
    (6, 16, 16, 32, 64), (3, 16, 16, 64, 64),                                             # groups that do not divide N
    (2, 64, 64, 256, 1088), (4, 64, 64, 256, 1152), (2, 64, 32, 256, 1088), (2, 64, 64, 48, 1088),   # head: K = 17, 18; Wo != 64; Cin % 32 != 0
    (600, 64, 64, 256, 64), (600, 64, 64, 64, 256), (160, 64, 64, 256, 1088),             # image ranges
]
SHAPES = ([s + (3, 3, 1, 1) for s in _SHAPES_3x3] + [s + (1, 1, 1, 0) for s in _SHAPES_1x1] + [
    (2, 256, 256, 3, 64, 7, 7, 2, 3), (2, 256, 256, 3, 32, 7, 7, 2, 3), (2, 250, 250, 3, 64, 7, 7, 2, 3),   # stem; Cout 32; no stem weight gradient
    (2, 224, 224, 3, 64, 7, 7, 2, 3), (2, 256, 256, 3, 64, 7, 7, 2, 2), (2, 256, 256, 4, 64, 7, 7, 2, 3),
    (2, 32, 32, 64, 128, 3, 3, 2, 1), (16, 64, 64, 128, 256, 3, 3, 2, 1),                                   # 3x3 stride 2
    (2, 32, 32, 64, 128, 1, 1, 2, 0), (16, 64, 64, 256, 512, 1, 1, 2, 0),                                   # 1x1 stride 2
    (2, 16, 16, 256, 256, 4, 4, 2, 1), (64, 32, 32, 256, 256, 4, 4, 2, 1),                                  # 4x4 stride 2 pad 1 (deconv)
    (2, 32, 32, 32, 1, 3, 3, 2, 1), (2, 32, 32, 1, 32, 3, 3, 1, 0),                                         # one channel, but not 'same' 3x3
])
PRECISIONS = (0, 1, 2, 3)                       # XAS_PREC_F32, BF16, BF16X6, F16X3
AMAX = ('none', 'grad', 'both')                 # operand maxima that come with the shape
TUNES = ('0', 'GENERAL_KERNELS', 'NO_WIDE_TILES', 'WGRAD_GLOBAL_LOAD', 'STEM_FWD_F32')
GROUPS = (1, 2, 4)


def conv_shape(_lib, shape, amax):
    n, hi, wi, cin, cout, r, s, stride, pad = shape
    ho, wo = (hi + 2 * pad - r) // stride + 1, (wi + 2 * pad - s) // stride + 1
    shp = _lib.ConvShape(n, hi, wi, cin, cout, r, s, stride, pad, ho, wo, 0)
    dummy = 256                                 # the queries only test the pointers for null
    shp.grad_amax = dummy if amax in ('grad', 'both') else None
    shp.x_amax = dummy if amax == 'both' else None
    return shp


def cases():
    return itertools.product(range(len(SHAPES)), PRECISIONS, AMAX, TUNES)


def record(_lib, shape, prec, amax, tune):
    """Sets precision and tuning (the caller restores them) and asks every query."""
    q = _lib.query
    assert q('xas_set_precision', prec) == 0
    assert q('xas_set_tuning', 0 if tune == '0' else getattr(_lib, 'TUNE_' + tune)) == 0
    s = ctypes.byref(conv_shape(_lib, shape, amax))
    k = max(1, shape[4] // 64)
    return ([q('xas_conv_kernel_class', s, p) for p in (0, 1, 2)] + [q('xas_conv_weight_planes', s, p) for p in (0, 1)] +
            [q('xas_conv_wgrad_workspace_floats', s), q('xas_conv_fwd_head_chunks', s, k, 64), q('xas_conv_fwd_head_chunks', s, 17, 64)] +
            [q('xas_conv_fwd_bnstats_workspace_floats', s, g) for g in GROUPS] +
            [q('xas_conv_dgrad_bn_bwd_workspace_floats', s, g) for g in GROUPS])


def table(_lib):
    prec, tune = _lib.query('xas_get_precision'), 0       # tuning has no getter: the shipped setting is 0
    try:
        return [record(_lib, SHAPES[i], p, a, t) for i, p, a, t in cases()]
    finally:
        _lib.query('xas_set_precision', prec)
        _lib.query('xas_set_tuning', tune)


def main():
    for p in (ROOT, os.path.join(ROOT, 'x-as-supervision_amd')):
        sys.path.insert(0, p)
    from xas_amd import _lib
    _lib.load()
    doc = {'shapes': [list(s) for s in SHAPES], 'precisions': list(PRECISIONS), 'amax': list(AMAX), 'tunes': list(TUNES),
           'groups': list(GROUPS), 'records': table(_lib)}
    with open(OUT, 'w') as f:
        f.write('{\n')
        for k in ('shapes', 'precisions', 'amax', 'tunes', 'groups'):
            f.write(' %s: %s,\n' % (json.dumps(k), json.dumps(doc[k], separators=(',', ':'))))
        f.write(' "records": [\n')
        f.write(',\n'.join(json.dumps(r, separators=(',', ':')) for r in doc['records']))
        f.write('\n]}\n')
    print('wrote %s: %d cases' % (OUT, len(doc['records'])))


if __name__ == '__main__':
    main()
