"""The weight-gradient kernels of csrc/conv.hip and csrc/conv_x6.hip (conv_wgrad_impl: thin_wgrad_kernel, wgrad_cout1_kernel,
stem_wgrad_kernel, wgrad_x6t_kernel, wgrad_x6_kernel, wgrad_buf_kernel, wgrad_kernel, all finished by slab_reduce_kernel2)
ALONE against float64, through the C ABI: no layers, no autograd.

The dispatch is restated here in Python (plan(): wgrad_on_x6, wgrad_x6_tile / the tile rule and the split rounding of
wgrad_plan, wgrad_x6t_plan, buf_ok, the tap span T of launch_wgrad_buf, thin_ok, stem_wgrad_ok, the chunk rules of the thin,
Cout = 1 and stem paths, the workspace size).  Every case of CASES names the path it is meant to reach (`claim`);
test_case_table_reaches_every_path needs no GPU and checks that the restated plan sends every case where it claims, that the
claimed paths are exactly REQUIRED, that the split properties of X6_PROPERTIES all occur, and the precondition of every exact
input.  The GPU tests assert the restated plan against the library where the library can tell (xas_conv_kernel_class,
xas_conv_wgrad_workspace_floats).

Two kinds of input (x and dy NHWC, the result in OIHW order).
  exact : integers |v| <= 3 with exact zeros and all-zero pixels, every weight element with terms of both signs, and
          sum |dy| |x| < 2^24 per weight element (float64 conv2d_weight of the absolute values).  Every product and partial sum
          is then an integer fp32 holds; an integer of magnitude 3 fills one bf16 and one fp16 piece at any power-of-two scale.
          The result EQUALS float64 conv2d_weight in exact fp32, bf16x6, f16x3 (true maxima and looser bounds) and plain bf16,
          under every tuning flag, in all three output forms; xas_conv_wgrad_acc on an integer `prev` gives prev + ref.
  real  : x = 1.5 randn + 0.3, dy = randn (heavy-tailed for one case per kernel).  Two bars for the fp32-accurate modes:
          Frobenius-relative error against float64 of the same fp32 operands < 3e-6, and per weight element
          with n non-padding terms and T = sum |term|:   |dW - dW64| <= (n 2^-24 + c) T,   c = 0 for fp32 arithmetic, 2^-23
          for bf16x6 (each product within one fp32 rounding), 2^-21 for f16x3 (two operands within 2^-22 each).  n 2^-24 is
          the worst case of any summation order.  Derived, not measured; the observed ratios are printed (RATIO lines).

Every launch: the workspace is exactly xas_conv_wgrad_workspace_floats floats (queried under the launch's precision and
tuning flags), outputs are pre-filled with a large finite value, and both end in sentinel floats inside the same allocation
that must be unchanged.  The three forms (xas_conv_wgrad through xas_unpack_weight, _oihw, _acc on zeros) agree bit for bit,
and so do two calls on the same inputs."""
import collections
import functools

import pytest
import torch

from xas_amd import _lib

U = 2.0 ** -24
SENT, SENT_V, FILL = 16, -62500000.0, 1.5e30
DEV = 'cuda'
WBK, THIN_CHUNK, COUT1_CHUNK, STEM_BLOCKS = 32, 2048, 2048, 1024          # conv_shared.h / conv.hip
ST_TH, ST_TW, ST_CO, ST_K = 8, 16, 64, 147
XTARGET, X6T_BLOCKS = 1024, 1536                                            # XAS_WGRAD_XTARGET, XAS_WX6T_BLOCKS
GL, ALT, PLAIN, GENERAL, NO_STEM = (_lib.TUNE_WGRAD_GLOBAL_LOAD, _lib.TUNE_WGRAD_ALT_ORDER, _lib.TUNE_WGRAD_PLAIN_KLOOP,
                                    _lib.TUNE_GENERAL_KERNELS, _lib.TUNE_NO_STEM_WGRAD)
GRAD_IS_X = 0x100
FORMS = ('packed', 'oihw', 'acc')
ENTRY = {'packed': 'xas_conv_wgrad', 'oihw': 'xas_conv_wgrad_oihw', 'acc': 'xas_conv_wgrad_acc'}

Shape = collections.namedtuple('Shape', 'N Hi Wi Cin Cout R S stride pad Ho Wo')


def cdiv(a, b):
    return -(-a // b)


def mk(n, cin, h, w, cout, k, stride, pad):
    return Shape(n, h, w, cin, cout, k, k, stride, pad, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1)


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def thin_ok(s, C):
    return (s.R == 3 and s.S == 3 and s.stride == 1 and s.pad == 1 and C % 4 == 0 and 4 <= C <= 64 and 256 % (C // 4) == 0
            and s.Ho == s.Hi and s.Wo == s.Wi)


def is_thin(s):
    return (s.Cout == 1 and thin_ok(s, s.Cin)) or (s.Cin == 1 and thin_ok(s, s.Cout))


def stem_wgrad_ok(s):
    return (s.Cin == 3 and s.Cout == ST_CO and s.R == 7 and s.S == 7 and s.stride == 2 and s.pad == 3 and s.Ho % ST_TH == 0
            and s.Wo % ST_TW == 0 and s.Ho * 2 == s.Hi and s.Wo * 2 == s.Wi)


def small_enough(s):
    xbytes = (s.N * s.Hi * s.Wi + s.pad * s.Wi + s.pad) * s.Cin * 4
    return xbytes < 0x7fffff00 and s.N * s.Ho * s.Wo * s.Cout * 4 < 0x7fffff00


def one_carry(s):
    return 31 // s.Wo + 1 <= s.Ho


def wgrad_on_x6(s, prec, tune, aligned=True):
    if prec == 'f32' or tune & GL:
        return False
    return s.Cin % 4 == 0 and s.Cout % 4 == 0 and s.Cout >= 16 and aligned and small_enough(s) and one_carry(s)


def wgrad_tile(Cout, KK):
    """wgrad_x6_tile, and the same rule in wgrad_plan."""
    bm = 128 if Cout >= 96 else (64 if Cout > 32 else 32)
    return bm, 128 if (KK > 64 or bm == 32) else 64


def wgrad_plan(s, x6, tune):
    """-> bm, bn, splits, pixels per split."""
    KK, M = s.R * s.S * s.Cin, s.N * s.Ho * s.Wo
    bm, bn = wgrad_tile(s.Cout, KK)
    nct = cdiv(s.Cout, bm)
    tiles = nct * cdiv(KK, bn)
    sp = cdiv(XTARGET if x6 else 1024, tiles)
    sp = max(1, min(sp, max(1, M // (128 if x6 else 256))))
    if x6 and sp >= 8:
        sp -= sp % 8
    elif x6 or not tune & ALT:
        while sp > 1 and (sp * nct) % 8 != 0 and sp * nct > 8:
            sp -= 1
    per = cdiv(cdiv(M, sp), WBK) * WBK
    return bm, bn, cdiv(M, per), per


def wgrad_x6t_plan(s):
    """-> bm, splits, patches per split, or None."""
    if (s.R, s.S, s.stride, s.pad) != (3, 3, 1, 1) or s.Ho != s.Hi or s.Wo != s.Wi or s.Cin % 32 or s.Hi % 8:
        return None
    if not (s.Wi % 16 == 0 or (s.Wi == 8 and s.N % 2 == 0)) or s.Cout not in (32, 64):
        return None
    np_ = s.N * s.Hi * s.Wi // 128
    sp = max(1, min(cdiv(X6T_BLOCKS, s.Cin // 32), np_ // 2))
    pps = cdiv(np_, sp)
    return s.Cout, cdiv(np_, pps), pps


def buf_T(Cin, bn):
    """launch_wgrad_buf: taps a column tile can span."""
    if Cin % bn == 0:
        return 1
    if Cin % (bn // 2) == 0:
        return 2
    return 4 if bn >= 128 and Cin % (bn // 4) == 0 else None


def pieces_of(prec, amax):
    return {'f32': 0, 'bf16': 1, 'bf16x6': 3, 'f16x3': 2 if amax else 3}[prec]


def plan(s, prec, tune=0, aligned=True, amax=False):
    """conv_wgrad_impl -> the path: kernel, tile, T, K loop, block order, vector loads, slabs (splits), steps per slab, steps
    of the last slab, operand pieces.  A step: 32 pixels (MFMA kernels), a 128-pixel patch (x6t, stem), 256 pixels (thin),
    one pixel (Cout = 1)."""
    KK, M = s.R * s.S * s.Cin, s.N * s.Ho * s.Wo
    if s.Cout % 4 and s.Cout != 1:
        return dict(kernel='refused')
    if is_thin(s):
        Mi = s.N * s.Hi * s.Wi
        chunks = min(cdiv(Mi, THIN_CHUNK), 1024)
        per = cdiv(cdiv(Mi, chunks), 256) * 256
        chunks = cdiv(Mi, per)
        return dict(kernel='thin', orient='cout1' if s.Cout == 1 else 'cin1', splits=chunks, steps=per // 256,
                    last=cdiv(Mi - (chunks - 1) * per, 256), last_pixels=Mi - (chunks - 1) * per)
    if s.Cout == 1:
        chunks = cdiv(M, COUT1_CHUNK)
        return dict(kernel='cout1', splits=chunks, steps=COUT1_CHUNK, last=M - (chunks - 1) * COUT1_CHUNK)
    if stem_wgrad_ok(s) and not tune & NO_STEM:
        patches = s.N * (s.Ho // ST_TH) * (s.Wo // ST_TW)
        ppb = cdiv(patches, STEM_BLOCKS)
        blocks = cdiv(patches, ppb)
        return dict(kernel='stem', splits=2 * blocks, steps=ppb, last=patches - (blocks - 1) * ppb)
    x6 = wgrad_on_x6(s, prec, tune, aligned)
    bm, bn, splits, mps = wgrad_plan(s, x6, tune)
    steps, last = mps // WBK, cdiv(M - (splits - 1) * mps, WBK)
    vec = s.Cin % 4 == 0 and aligned
    buf_ok = vec and s.Cin % 32 == 0 and small_enough(s) and one_carry(s) and not tune & GL
    t = wgrad_x6t_plan(s) if x6 and not tune & GENERAL else None
    if t:
        tbm, tsplits, pps = t
        np_ = s.N * s.Hi * s.Wi // 128
        return dict(kernel='x6t', tile=(tbm,), tw=16 if s.Wo % 16 == 0 else 8, splits=tsplits, steps=pps,
                    last=np_ - (tsplits - 1) * pps, pieces=pieces_of(prec, amax))
    if x6:
        return dict(kernel='x6', tile=(bm, bn), order='xcd' if splits % 8 == 0 else 'grouped', splits=splits, steps=steps,
                    last=last, pieces=pieces_of(prec, amax), M=M)
    order = 'alt' if tune & ALT else 'shipped'
    if buf_ok:
        return dict(kernel='buf', tile=(bm, bn), T=buf_T(s.Cin, bn), kloop='plain' if tune & PLAIN else 'pipe', order=order,
                    splits=splits, steps=steps, last=last)
    tile = (32, 128) if bm == 32 else ((bm, 64) if bn == 64 and vec else (bm, 128))
    return dict(kernel='general', tile=tile, vec=vec, order=order, splits=splits, steps=steps, last=last)


def path_key(p):
    k = p['kernel']
    if k == 'thin':
        return k, p['orient']
    if k == 'x6t':
        return k, p['tile'][0], p['tw']
    if k == 'x6':
        return k, p['tile']
    if k == 'buf':
        return k, p['tile'], p['T'], p['kloop'], p['order']
    if k == 'general':
        return k, p['tile'], p['vec']
    return (k,)


def workspace_floats(s, prec, tune):
    """xas_conv_wgrad_workspace_floats: the largest of the three plans (the alignment of x is unknown to the query)."""
    if is_thin(s):
        return (cdiv(s.N * s.Hi * s.Wi, THIN_CHUNK) + 1) * (s.Cin if s.Cout == 1 else s.Cout) * 9
    if s.Cout == 1:
        return cdiv(s.N * s.Ho * s.Wo, COUT1_CHUNK) * s.R * s.S * s.Cin
    if stem_wgrad_ok(s):
        return 2 * STEM_BLOCKS * ST_CO * ST_K
    t = wgrad_x6t_plan(s)
    sp = max(wgrad_plan(s, False, tune)[2], wgrad_plan(s, True, tune)[2], t[1] if t else 0)
    return sp * s.Cout * s.R * s.S * s.Cin


def kernel_class(s, prec, tune, amax):
    """xas_conv_kernel_class(s, 2): 0 no MFMA, 1 exact fp32, 2 bf16, 3 bf16x6, 4 f16x3."""
    if is_thin(s) or s.Cout == 1:
        return 0
    return {0: 1, 1: 2, 3: 3, 2: 4}[pieces_of(prec, amax)] if wgrad_on_x6(s, prec, tune) else 1


# ------------------------------------------------------------------------------------------------ the case table
# fam: the arithmetic modes a case runs in.  'f32': exact fp32; 'split': bf16x6, f16x3 (true and looser maxima), bf16 - one
# dispatch, three operand formats; 'any': kernels that do not look at the mode, run in exact fp32 and in the default mode.
MODES = {'f32': ('f32',), 'split': ('bf16x6', 'f16x3', 'f16x3_loose_dy', 'f16x3_loose_x', 'f16x3_loose_both', 'bf16'),
         'any': ('f32', 'bf16x6')}
ACCURATE = {'f32': ('f32',), 'split': ('bf16x6', 'f16x3'), 'any': ('f32', 'bf16x6')}
Case = collections.namedtuple('Case', 'id shape fam tune claim misalign heavy')
CASES = []


def case(cid, shape, fam, claim, tune=0, misalign=False, heavy=False):
    CASES.append(Case(cid, mk(*shape), fam, tune, claim, misalign, heavy))


# thin_wgrad_kernel, both orientations
for C_, n_, h_, w_, extra in ((4, 1, 3, 5, dict(splits=1, last_pixels=15)), (8, 2, 7, 9, dict(splits=1)),
                              (64, 3, 33, 21, dict(splits=2, steps=5, last_pixels=799))):
    case('thin_cout1_C%d' % C_, (n_, C_, h_, w_, 1, 3, 1, 1), 'any', dict(kernel='thin', orient='cout1', **extra), heavy=C_ == 64)
    case('thin_cin1_C%d' % C_, (n_, 1, h_, w_, C_, 3, 1, 1), 'any', dict(kernel='thin', orient='cin1', **extra))
# wgrad_cout1_kernel
case('cout1_linear_512', (32, 512, 1, 1, 1, 1, 1, 0), 'any', dict(kernel='cout1', splits=1))
case('cout1_3x3_C12', (3, 12, 27, 27, 1, 3, 1, 1), 'any', dict(kernel='cout1', splits=2, last=139), heavy=True)
case('cout1_3x3_s2', (2, 32, 17, 13, 1, 3, 2, 1), 'any', dict(kernel='cout1', splits=1))
# stem_wgrad_kernel
case('stem_1_patch', (1, 3, 16, 32, 64, 7, 2, 3), 'any', dict(kernel='stem', splits=2, steps=1))
case('stem_12_patches', (3, 3, 32, 64, 64, 7, 2, 3), 'any', dict(kernel='stem', splits=24, steps=1), heavy=True)
# (65 images of 64 x 128 are 1040 patches in 520 FULL blocks; 115 of 48 x 96 are 1035: the last block holds one)
case('stem_1035_patches', (115, 3, 48, 96, 64, 7, 2, 3), 'any', dict(kernel='stem', splits=2 * 518, steps=2, last=1))
case('stem_refused_50x70', (2, 3, 50, 70, 64, 7, 2, 3), 'any', dict(kernel='general', tile=(64, 128), vec=False, splits=6))
case('stem_switched_off', (3, 3, 32, 64, 64, 7, 2, 3), 'any', dict(kernel='general', tile=(64, 128), vec=False), tune=NO_STEM)
# wgrad_x6t_kernel, and the same shapes with the kernel switched off
X6T = [('1patch_bm32', (1, 32, 8, 16, 32, 3, 1, 1), dict(kernel='x6t', tile=(32,), tw=16, splits=1, steps=1)),
       ('8wide_bm64', (2, 64, 8, 8, 64, 3, 1, 1), dict(kernel='x6t', tile=(64,), tw=8, splits=1, steps=1)),
       ('8wide_5patches', (10, 32, 8, 8, 32, 3, 1, 1), dict(kernel='x6t', tile=(32,), tw=8, splits=2, steps=3, last=2)),
       ('16wide_5patches', (5, 64, 8, 16, 64, 3, 1, 1), dict(kernel='x6t', tile=(64,), tw=16, splits=2, steps=3, last=2)),
       ('3_channel_blocks', (2, 96, 24, 48, 64, 3, 1, 1), dict(kernel='x6t', tile=(64,), tw=16, splits=9, steps=2)),
       ('8wide_odd_N', (3, 32, 8, 8, 32, 3, 1, 1), dict(kernel='x6', tile=(32, 128), splits=1, steps=6))]
for name_, shape_, claim_ in X6T:
    case('x6t_' + name_, shape_, 'split', claim_, heavy=name_ == '3_channel_blocks')
    case('x6t_' + name_ + '_off', shape_, 'split', dict(kernel='x6'), tune=GENERAL)
# wgrad_x6_kernel, five tiles; the same shapes on wgrad_kernel with vector loads (XAS_TUNE_WGRAD_GLOBAL_LOAD)
X6 = [('32x128_ragged', (2, 36, 9, 7, 20, 3, 1, 1), (32, 128), dict(splits=1, steps=4, M=126)),
      ('32x128_1x1', (5, 32, 16, 16, 32, 1, 1, 0), (32, 128), dict(splits=8, steps=5, order='xcd')),
      ('64x64_cout48', (3, 64, 8, 16, 48, 1, 1, 0), (64, 64), dict(splits=3, steps=4, order='grouped')),
      ('64x64_cin16', (1, 16, 4, 8, 64, 1, 1, 0), (64, 64), dict(splits=1, steps=1)),
      ('64x128_s2', (7, 128, 17, 13, 64, 3, 2, 1), (64, 128), dict(splits=3, steps=5, last=4, M=441)),
      ('128x64', (2, 64, 12, 12, 100, 1, 1, 0), (128, 64), dict(splits=2, steps=5, last=4)),
      ('128x128_3x3', (2, 96, 8, 8, 160, 3, 1, 1), (128, 128), dict(splits=1, steps=4)),
      ('128x128_4x4s2', (4, 256, 16, 16, 256, 4, 2, 1), (128, 128), dict(splits=2, steps=4))]
for name_, shape_, tile_, extra in X6:
    case('x6_' + name_, shape_, 'split', dict(kernel='x6', tile=tile_, **extra), heavy=name_ == '128x128_3x3')
    if name_ not in ('32x128_ragged', '64x64_cin16', '128x128_4x4s2'):
        case('general_vec_' + name_, shape_, 'any', dict(kernel='general', tile=tile_, vec=True), tune=GL, heavy=name_ == '128x128_3x3')
# the carry boundary 31 / Wo + 1 <= Ho: on it (x6 / buf) and one step beyond it (wgrad_kernel)
for k_, pad_ in ((1, 0), (3, 1)):
    for ho_, wo_ in ((4, 8), (2, 16), (1, 32), (8, 4), (16, 2), (32, 1), (6, 6), (7, 5)):
        case('carry_%dx%d_k%d_x6' % (ho_, wo_, k_), (3, 32, ho_, wo_, 32, k_, 1, pad_), 'split', dict(kernel='x6', tile=(32, 128)))
        case('carry_%dx%d_k%d_buf' % (ho_, wo_, k_), (3, 32, ho_, wo_, 32, k_, 1, pad_), 'f32', dict(kernel='buf', tile=(32, 128), T=4))
    for ho_, wo_ in ((3, 8), (7, 4), (5, 6), (4, 4)):
        for fam_ in ('split', 'f32'):
            case('beyond_%dx%d_k%d_%s' % (ho_, wo_, k_, fam_), (3, 32, ho_, wo_, 32, k_, 1, pad_), fam_,
                 dict(kernel='general', tile=(32, 128), vec=True))
# wgrad_buf_kernel: every tile x T; PLAIN_KLOOP and ALT_ORDER once per tile
for bm_, cout_ in ((32, 32), (64, 64), (128, 128)):
    case('buf_%dx128_T1' % bm_, (3, 128, 12, 16, cout_, 1, 1, 0), 'f32', dict(kernel='buf', tile=(bm_, 128), T=1, splits=2, steps=9),
         heavy=bm_ == 64)
    case('buf_%dx128_T2' % bm_, (2, 192, 8, 8, cout_, 3, 1, 1), 'f32', dict(kernel='buf', tile=(bm_, 128), T=2, splits=1, steps=4))
    case('buf_%dx128_T4' % bm_, (3, 96, 17, 13, cout_, 3, 2, 1), 'f32', dict(kernel='buf', tile=(bm_, 128), T=4, splits=1, last=6))
    case('buf_%dx128_plain' % bm_, (3, 96, 17, 13, cout_, 3, 2, 1), 'f32', dict(kernel='buf', tile=(bm_, 128), T=4, kloop='plain'), tune=PLAIN)
    case('buf_%dx128_alt' % bm_, (3, 128, 12, 16, cout_, 1, 1, 0), 'f32', dict(kernel='buf', tile=(bm_, 128), T=1, order='alt', splits=2),
         tune=ALT)
for bm_, cout_ in ((64, 64), (128, 128)):
    case('buf_%dx64_T1' % bm_, (3, 64, 12, 16, cout_, 1, 1, 0), 'f32', dict(kernel='buf', tile=(bm_, 64), T=1, splits=2))
    case('buf_%dx64_T2' % bm_, (2, 32, 9, 7, cout_, 1, 1, 0), 'f32', dict(kernel='buf', tile=(bm_, 64), T=2, splits=1, last=4))
    case('buf_%dx64_plain' % bm_, (2, 32, 9, 7, cout_, 1, 1, 0), 'f32', dict(kernel='buf', tile=(bm_, 64), T=2, kloop='plain'), tune=PLAIN)
    case('buf_%dx64_alt' % bm_, (3, 64, 12, 16, cout_, 1, 1, 0), 'f32', dict(kernel='buf', tile=(bm_, 64), T=1, order='alt', splits=2), tune=ALT)
# wgrad_kernel
case('general_f32_cin36', (2, 36, 9, 7, 20, 3, 1, 1), 'f32', dict(kernel='general', tile=(32, 128), vec=True))
case('general_linear_cin6', (576, 6, 1, 1, 32, 1, 1, 0), 'any', dict(kernel='general', tile=(32, 128), vec=False, splits=2, steps=9))
case('general_cin1_cout12', (2, 1, 9, 7, 12, 3, 1, 1), 'any', dict(kernel='general', tile=(32, 128), vec=False), heavy=True)
case('misaligned_x_off_x6t', (2, 64, 8, 16, 64, 3, 1, 1), 'split', dict(kernel='general', tile=(64, 128), vec=False), misalign=True)
case('misaligned_x_off_x6', (3, 64, 8, 16, 48, 1, 1, 0), 'split', dict(kernel='general', tile=(64, 128), vec=False), misalign=True)
case('misaligned_x_off_buf', (3, 128, 12, 16, 128, 1, 1, 0), 'f32', dict(kernel='general', tile=(128, 128), vec=False), misalign=True)

CASE_IDS = [c.id for c in CASES]
TILES = ((32, 128), (64, 64), (64, 128), (128, 64), (128, 128))
REQUIRED = ({('thin', 'cout1'), ('thin', 'cin1'), ('cout1',), ('stem',), ('x6t', 32, 16), ('x6t', 32, 8), ('x6t', 64, 16), ('x6t', 64, 8)}
            | {('x6', t) for t in TILES} | {('general', t, True) for t in TILES}
            | {('general', (32, 128), False), ('general', (64, 128), False), ('general', (128, 128), False)}
            | {('buf', t, T, 'pipe', 'shipped') for t in TILES for T in ((1, 2, 4) if t[1] == 128 else (1, 2))}
            | {('buf', (bm, 128), 4, 'plain', 'shipped') for bm in (32, 64, 128)} | {('buf', (bm, 64), 2, 'plain', 'shipped') for bm in (64, 128)}
            | {('buf', (bm, 128), 1, 'pipe', 'alt') for bm in (32, 64, 128)} | {('buf', (bm, 64), 1, 'pipe', 'alt') for bm in (64, 128)})
X6_PROPERTIES = {'splits % 8 == 0', 'splits % 8 != 0', 'splits == 1', 'one step per split', 'odd steps', 'even steps',
                 'M % 32 != 0', 'short last split'}


def x6_properties(p):
    out = {'splits % 8 == 0' if p['splits'] % 8 == 0 else 'splits % 8 != 0', 'odd steps' if p['steps'] % 2 else 'even steps'}
    if p['splits'] == 1:
        out.add('splits == 1')
    if p['steps'] == 1:
        out.add('one step per split')
    if p['M'] % 32:
        out.add('M % 32 != 0')
    if p['splits'] > 1 and p['last'] < p['steps']:
        out.add('short last split')
    return out


def amax_of_mode(mode):
    return mode.startswith('f16x3')


def prec_of_mode(mode):
    return 'f16x3' if mode.startswith('f16x3') else mode


# ------------------------------------------------------------------------------------------------ inputs and float64
def cw64(x, dy, s):
    return torch.nn.grad.conv2d_weight(x, (s.Cout, s.Cin, s.R, s.S), dy, s.stride, s.pad)


def term_count(s):
    """[R][S]: how many (image, output pixel) terms of a weight element at tap (r, q) lie inside the image."""
    def axis(n_out, n_in, k):
        return torch.tensor([sum(0 <= o * s.stride - s.pad + r < n_in for o in range(n_out)) for r in range(k)], dtype=torch.float64)
    return s.N * axis(s.Ho, s.Hi, s.R).view(-1, 1) * axis(s.Wo, s.Wi, s.S).view(1, -1)


@functools.lru_cache(maxsize=None)
def exact_inputs(s):
    """x, dy (NCHW float64, integers |v| <= 3, 4 % exact zeros, 6 % all-zero pixels), float64 dW, sum |term|.  Drawn again
    until every weight element with a term has terms of both signs (|sum| < sum of magnitudes)."""
    n = term_count(s)
    for attempt in range(400):
        g = torch.Generator().manual_seed(1000 * (sum(s) + 7 * s.Cin + 3 * s.Wi) + attempt)

        def draw(N, C, H, W):
            v = torch.randint(1, 4, (N, C, H, W), generator=g) * (2 * torch.randint(0, 2, (N, C, H, W), generator=g) - 1)
            v[torch.rand(N, C, H, W, generator=g) < 0.04] = 0
            v[(torch.rand(N, 1, H, W, generator=g) < 0.06).expand(N, C, H, W)] = 0
            return v.double()
        x, dy = draw(s.N, s.Cin, s.Hi, s.Wi), draw(s.N, s.Cout, s.Ho, s.Wo)
        ref, mag = cw64(x, dy, s), cw64(x.abs(), dy.abs(), s)
        zero_pixel = s.N * s.Ho * s.Wo < 40 or (bool((x == 0).all(1).any()) and bool((dy == 0).all(1).any()))
        if zero_pixel and bool(((ref.abs() < mag) | (n == 0)).all()):
            return x, dy, ref, mag
    raise AssertionError('no exact input with both signs in every receptive field: %s' % (s,))


@functools.lru_cache(maxsize=None)
def real_inputs(s, heavy, scale_x=1.0, scale_dy=1.0):
    """fp32 x = 1.5 randn + 0.3, dy = randn (heavy: times exp(2 randn)) as NCHW float64, float64 dW, sum |term|."""
    g = torch.Generator().manual_seed(sum(s) + 13 * s.Cout)
    x = ((torch.randn(s.N, s.Cin, s.Hi, s.Wi, generator=g) * 1.5 + 0.3) * scale_x).float()
    dy = torch.randn(s.N, s.Cout, s.Ho, s.Wo, generator=g)
    if heavy:
        dy = dy * torch.exp(torch.randn(s.N, s.Cout, s.Ho, s.Wo, generator=g) * 2.0)
    dy = (dy * scale_dy).float()
    x, dy = x.double(), dy.double()
    return x, dy, cw64(x, dy, s), cw64(x.abs(), dy.abs(), s)


# ------------------------------------------------------------------------------------------------ the CPU-only check
def test_case_table_reaches_every_path():
    """No GPU: the restated plan sends every case to the path it claims in every mode it runs in, the claimed paths are
    exactly REQUIRED, the split properties all occur on wgrad_x6_kernel, every exact input meets its precondition."""
    reached, props = set(), set()
    for c in CASES:
        for mode in MODES[c.fam]:
            p = plan(c.shape, prec_of_mode(mode), c.tune, not c.misalign, amax_of_mode(mode))
            for k, v in c.claim.items():
                assert p.get(k) == v, '%s (%s): %s is %r, claimed %r  [%r]' % (c.id, mode, k, p.get(k), v, p)
            assert p['kernel'] != 'buf' or p['T'] is not None
            reached.add(path_key(p))
            if p['kernel'] not in ('thin', 'stem'):                 # the slabs of the launch fit the workspace the query hands out
                assert p['splits'] * c.shape.Cout * c.shape.R * c.shape.S * c.shape.Cin <= workspace_floats(c.shape, prec_of_mode(mode), c.tune)
            if p['kernel'] == 'x6':
                props |= x6_properties(p)
            if p['kernel'] in ('x6', 'x6t'):
                assert p['pieces'] == {'bf16': 1, 'bf16x6': 3}.get(mode, 2), (c.id, mode)
        x, dy, ref, mag = exact_inputs(c.shape)
        assert float(x.abs().max()) <= 3 and float(dy.abs().max()) <= 3 and bool((x == x.round()).all()) and bool((dy == dy.round()).all())
        assert float(mag.max()) < 2 ** 24, c.id
        assert (bool((x == 0).all(1).any()) and bool((dy == 0).all(1).any())) or c.shape.N * c.shape.Ho * c.shape.Wo < 40, c.id   # all-zero pixels
        assert bool(((ref.abs() < mag) | (term_count(c.shape) == 0)).all()), c.id
    assert reached == REQUIRED, 'not reached: %s; not required: %s' % (sorted(map(str, REQUIRED - reached)), sorted(map(str, reached - REQUIRED)))
    assert props == X6_PROPERTIES, X6_PROPERTIES - props
    assert plan(mk(2, 32, 8, 8, 6, 1, 1, 0), 'f32')['kernel'] == 'refused'


# ------------------------------------------------------------------------------------------------ plumbing (GPU)
gpu = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _library_back(request):
    def back():
        if _lib._lib is not None:
            _lib.query('xas_set_tuning', 0)
            _lib.query('xas_set_precision', _lib.PREC_DEFAULT)
    request.addfinalizer(back)


class Buf:
    """n floats (pre-filled) followed by SENT sentinel floats; `lead` floats in front move the start off 16-byte alignment."""

    def __init__(self, n, fill=FILL, src=None, lead=0):
        self.n, self.lead = n, lead
        self.all = torch.full((lead + n + SENT,), fill, device=DEV)
        self.all[lead + n:] = SENT_V
        if src is not None:
            self.all[lead:lead + n] = src.reshape(-1).float()
        self.t = self.all[lead:lead + n]

    def ptr(self):
        return self.all.data_ptr() + 4 * self.lead

    def intact(self):
        assert bool((self.all[self.lead + self.n:] == SENT_V).all()), 'floats behind a buffer of %d were written' % self.n


def bits(t):
    return t.contiguous().view(torch.int32)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


class Operands:
    """x and dy of a case on the device (NHWC fp32); misalign: x starts one float into its allocation."""

    def __init__(self, x, dy, misalign=False):
        self.xb = Buf(x.numel(), src=nhwc(x), lead=1 if misalign else 0)
        self.x, self.dy = self.xb.t, nhwc(dy)
        assert (self.xb.ptr() % 16 != 0) == misalign and self.dy.data_ptr() % 16 == 0


def conv_shape(s, mode, ops, flags=0):
    """The ConvShape of a launch in `mode` (the process precision is set to it).  f16x3: the measured maxima
    (shape_with_maxima), or each replaced by a looser upper bound."""
    from xas_amd import ops_nn as O
    prec = prec_of_mode(mode)
    assert _lib.query('xas_set_precision', _lib.PREC_NAMES[prec]) == 0
    shp = O._shape(s.N, s.Hi, s.Wi, s.Cin, s.Cout, s.R, s.S, s.stride, s.pad, s.Ho, s.Wo, flags)
    if prec != 'f16x3':
        return shp
    if mode == 'f16x3' and flags == 0 and ops.xb.lead == 0:
        out = O.shape_with_maxima(shp, ops.dy, ops.x)
    else:
        fd = 100.5 if mode in ('f16x3_loose_dy', 'f16x3_loose_both') else 1.0
        fx = 37.25 if mode in ('f16x3_loose_x', 'f16x3_loose_both') else 1.0
        a, b = O.amax_slot_from_value(ops.dy.abs().max() * fd), O.amax_slot_from_value(ops.x.abs().max() * fx)
        if flags & GRAD_IS_X:                                   # grad_amax describes the x argument, x_amax the dy argument
            a, b = b, a
        out = _lib.ConvShape(*[getattr(shp, f) for f in Shape._fields], flags, a.data_ptr(), b.data_ptr())
        out._slots = (a, b)
    assert out.grad_amax and out.x_amax
    return out


def launch(s, shp, ops, form, tune, prev=None, want_ws=None):
    """One weight gradient -> [Cout][Cin][R][S] (a copy).  Sentinels behind the output and the exactly-sized workspace."""
    nw = s.Cout * s.Cin * s.R * s.S
    _lib.query('xas_set_tuning', tune)
    try:
        nws = _lib.query('xas_conv_wgrad_workspace_floats', shp)
        assert nws > 0 and (want_ws is None or nws == want_ws), 'workspace %d floats, restated plan %s' % (nws, want_ws)
        ws = Buf(nws)
        out = Buf(nw, src=prev) if form == 'acc' else Buf(nw)
        assert form != 'acc' or prev is not None
        _lib.call(ENTRY[form], ops.xb.ptr(), ops.dy.data_ptr(), out.ptr(), ws.ptr(), shp)
    finally:
        _lib.query('xas_set_tuning', 0)
    torch.cuda.synchronize()
    ws.intact(), out.intact(), ops.xb.intact()
    if form == 'packed':
        o2 = Buf(nw)
        _lib.call('xas_unpack_weight', out.ptr(), o2.ptr(), s.Cout, s.Cin, s.R, s.S, 0)
        torch.cuda.synchronize()
        o2.intact()
        out = o2
    return out.t.view(s.Cout, s.Cin, s.R, s.S).clone()


def check_library_agrees(c, mode, shp):
    """xas_conv_kernel_class under the launch's flags against the restated plan."""
    _lib.query('xas_set_tuning', c.tune)
    try:
        got = _lib.query('xas_conv_kernel_class', shp, 2)
    finally:
        _lib.query('xas_set_tuning', 0)
    assert got == kernel_class(c.shape, prec_of_mode(mode), c.tune, amax_of_mode(mode)), (c.id, mode, got)


# ------------------------------------------------------------------------------------------------ exact inputs
@gpu
@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_exact(c):
    """Integers: every mode, every form EQUALS float64; the forms agree bit for bit; prev + dW exactly; a second call gives
    the same bits; sentinels intact (launch())."""
    s = c.shape
    x, dy, ref, mag = exact_inputs(s)
    ops = Operands(x, dy, c.misalign)
    ref_d = ref.to(DEV)
    zeros = torch.zeros_like(ref_d)
    prev = ((torch.arange(ref.numel(), device=DEV) % 41) - 20.).view_as(ref_d)
    for mode in MODES[c.fam]:
        shp = conv_shape(s, mode, ops)
        check_library_agrees(c, mode, shp)
        want_ws = workspace_floats(s, prec_of_mode(mode), c.tune)
        outs = {f: launch(s, shp, ops, f, c.tune, prev=zeros, want_ws=want_ws) for f in FORMS}
        for f, o in outs.items():
            bad = (o.double() != ref_d).nonzero()
            assert bad.numel() == 0, '%s %s %s: %d of %d elements differ, first at %s: %r, float64 %r' % (
                c.id, mode, f, bad.shape[0], ref.numel(), bad[0].tolist(), float(o[tuple(bad[0])]), float(ref_d[tuple(bad[0])]))
            assert torch.equal(bits(o), bits(outs['oihw'])), '%s %s: form %s differs from oihw in its bits' % (c.id, mode, f)
        acc = launch(s, shp, ops, 'acc', c.tune, prev=prev)
        assert torch.equal(acc.double(), prev.double() + ref_d), '%s %s: accumulated form' % (c.id, mode)
        assert torch.equal(bits(launch(s, shp, ops, 'oihw', c.tune)), bits(outs['oihw'])), '%s %s: second call' % (c.id, mode)


# ------------------------------------------------------------------------------------------------ real inputs
REPORT = {}


def bars(o, ref, mag, n, cterm):
    """-> Frobenius-relative error, largest element error / ((n 2^-24 + c) T)."""
    err = (o.double().cpu() - ref).abs()
    bar = (n * U + cterm) * mag
    r = torch.where(bar > 0, err / torch.where(bar > 0, bar, torch.ones_like(bar)), torch.where(err > 0, float('inf'), 0.).double())
    return float(err.norm() / ref.norm()), float(r.max())


def report(key, frob, elem):
    f0, e0 = REPORT.get(key, (0., 0.))
    REPORT[key] = (max(f0, frob), max(e0, elem))
    print('RATIO %-44s frobenius / 3e-6 = %.4f  element / bar = %.4f' % (key, frob / 3e-6, elem))


def c_of(path, mode):
    if path['kernel'] not in ('x6', 'x6t') or mode == 'f32':
        return 0.
    return 2.0 ** -21 if path['pieces'] == 2 else 2.0 ** -23


@gpu
@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_real(c):
    """Real values in the fp32-accurate modes against both bars; heavy-tailed dy too where the case is marked; the three
    forms the same bits."""
    s = c.shape
    n = term_count(s).expand(s.Cout, s.Cin, s.R, s.S)
    for heavy in ((False, True) if c.heavy else (False,)):
        x, dy, ref, mag = real_inputs(s, heavy)
        ops = Operands(x, dy, c.misalign)
        for mode in ACCURATE[c.fam]:
            shp = conv_shape(s, mode, ops)
            path = plan(s, prec_of_mode(mode), c.tune, not c.misalign, amax_of_mode(mode))
            want_ws = workspace_floats(s, prec_of_mode(mode), c.tune)
            outs = {f: launch(s, shp, ops, f, c.tune, prev=torch.zeros(ref.shape, device=DEV), want_ws=want_ws) for f in FORMS}
            o = outs['oihw']
            assert bool(torch.isfinite(o).all())
            for f in FORMS:
                assert torch.equal(bits(outs[f]), bits(o)), '%s %s: form %s differs from oihw in its bits' % (c.id, mode, f)
            frob, elem = bars(o, ref, mag, n, c_of(path, mode))
            key = '%s %s' % ('/'.join(str(v) for v in path_key(path)), 'fp32' if c_of(path, mode) == 0 else mode)
            report(key + (' heavy' if heavy else ''), frob, elem)
            assert frob < 3e-6 and elem <= 1, '%s %s: Frobenius %.3e, element ratio %.3f' % (c.id, mode, frob, elem)


@gpu
@pytest.mark.parametrize('big', ['x', 'dy'])
def test_grad_is_x_operand_magnitudes(big):
    """The ConvTranspose2d weight gradient (4x4 s2 p1, f16x3, XAS_GRAD_IS_X: grad_amax describes the x argument, x_amax the
    dy argument) with one operand at 1e4 and the other at 1e-6: a swapped assignment scales one operand's fp16 pieces to
    overflow or to zero."""
    s = mk(4, 256, 16, 16, 256, 4, 2, 1)
    sx, sd = (1e4, 1e-6) if big == 'x' else (1e-6, 1e4)
    x, dy, ref, mag = real_inputs(s, False, sx, sd)
    ops = Operands(x, dy)
    n = term_count(s).expand(s.Cout, s.Cin, s.R, s.S)
    for mode in ('f16x3', 'f16x3_loose_both'):
        shp = conv_shape(s, mode, ops, flags=GRAD_IS_X)
        assert _lib.query('xas_conv_kernel_class', shp, 2) == 4
        o = launch(s, shp, ops, 'oihw', 0)
        assert bool(torch.isfinite(o).all()), 'non-finite weight gradient'
        frob, elem = bars(o, ref, mag, n, 2.0 ** -21)
        report('x6/(128, 128) f16x3 GRAD_IS_X big %s' % big, frob, elem)
        assert frob < 3e-6 and elem <= 1, (mode, frob, elem)


# ------------------------------------------------------------------------------------------------ refusals
@gpu
def test_refusals_launch_nothing():
    """Cout = 6 and each null buffer in turn, in all three forms: non-zero status, a message, output and workspace untouched."""
    good = mk(2, 32, 8, 8, 32, 3, 1, 1)
    x, dy, _, _ = exact_inputs(good)
    ops = Operands(x, dy)
    out, ws = Buf(64 * 32 * 9), Buf(1 << 16)
    st = _lib.stream()
    err = _lib.load().xas_last_error

    def shape_of(s):
        return _lib.ConvShape(*s, 0)

    for form in FORMS:
        f = _lib.fn(ENTRY[form])
        args = [ops.xb.ptr(), ops.dy.data_ptr(), out.ptr(), ws.ptr()]
        calls = {'Cout = 6': lambda: f(*args, shape_of(good._replace(Cout=6)), st)}
        for i, name in enumerate(('x', 'dy', 'dw', 'workspace')):
            calls['null ' + name] = lambda i=i: f(*(args[:i] + [None] + args[i + 1:]), shape_of(good), st)
        for name, go in calls.items():
            rc = go()
            torch.cuda.synchronize()
            assert rc != 0, '%s %s: accepted' % (form, name)
            assert len(err().decode()) > 0 and 'conv_wgrad' in err().decode(), (form, name, err())
            out.intact(), ws.intact()
            assert bool((out.t == FILL).all()) and bool((ws.t == FILL).all()), '%s %s wrote a buffer' % (form, name)
