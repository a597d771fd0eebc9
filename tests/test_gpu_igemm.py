"""The forward and data-gradient kernels of csrc/conv.hip and csrc/conv_x6.hip (igemm_buf_kernel, igemm_kernel, igemm_x6_kernel,
igemm_x6t_kernel, igemm_x6p_kernel, stem_fwd_kernel, stem_fwd_f16_kernel, direct_fwd_kernel, direct_dgrad_kernel,
thin_vec2scalar_kernel, thin_scalar2vec_kernel) ALONE against float64, through the C ABI: xas_pack_weight / xas_split_weight
(plane count from xas_conv_weight_planes), xas_conv_fwd with and without bias, xas_conv_dgrad, xas_conv_dgrad_acc,
xas_conv_dgrad_acc_masked.  No layers, no autograd.  x, y, dy, dx are NHWC.

The dispatch is restated here in Python (plan(): fwd_route / dgrad_route, pick_tile, pick_tile_x6 with tap_tile_ok and
x6p_takes, the loader and loop choice of f32_loop with its short_k rule, the tile count of x6p_tiles_per_block).  Every case of
CASES names the pass it runs (0 forward, 1 data gradient), its runs (arithmetic mode, tuning flags) and what each run is
meant to reach (`claim`: kernel, tile, loop, phases, pieces P, patch width, tpb, M- and N-tiles and whether the last of each
is ragged - every one of these keys on the MFMA route, CLAIM_KEYS; the route alone off it).  The stem shape runs without a bias
on its two kernels and, in cases of its own, WITH a bias on direct_fwd_kernel (fwd_route looks at the bias pointer of the call).
test_case_table_reaches_every_path needs no GPU: the restated plan equals every claim, equals the library
(xas_conv_igemm_plan, xas_conv_kernel_class, xas_conv_weight_planes), the claimed paths are exactly REQUIRED, the properties
of PROPERTIES all occur, and every exact input meets its precondition.  The GPU tests ask the library once more before
every launch.

Two kinds of input.
  exact : integers |v| <= 3 with exact zeros and all-zero pixels; bias, prev and dprev integers too; every output element
          with 16 terms or more and a non-zero term has terms of both signs; sum |x| |w| + |bias| < 2^24 per output element
          (float64 of the absolute values; the one case whose reference is computed on the device: 9 K + 3 < 2^24).  Every
          product and partial sum is then an integer fp32 holds.  An integer of magnitude <= 3 fills ONE piece of every
          format at the scales in use: bf16 has 8 significant bits; the fp16 pieces hold 2^10 w (<= 3072, 11 bits) and s x
          with s the power of two that puts the (true or looser) maximum below 2^15.  So the result EQUALS float64 in exact
          fp32, bf16x6, f16x3 (true maximum, and a four times larger bound) and plain bf16 under every tuning flag of the
          case; xas_conv_dgrad_acc gives prev + ref, the masked form ref + mask * dprev; a dx pixel no tap reaches is 0.
  real  : forward x = 1.5 randn + 0.3, w = randn / sqrt(fan-in); data gradient dy = randn; heavy-tailed (times exp(2 randn))
          for one case per kernel.  The fp32-accurate modes only, two bars: Frobenius-relative error against float64 of the
          same fp32 operands < 3e-6, and per element with n non-padding terms (bias and prev counted)
          and T = sum |term|:   |y - y64| <= (n 2^-24 + c) T,   c = 0 for fp32 arithmetic, 2^-23 for bf16x6, 2^-21 for
          f16x3 (tests/test_gpu_wgrad.py derives them: two operands within 2^-22 each, the dropped product of the second
          pieces another 2^-22), f16x3 plus the floor the conv_x6.hip header documents, n 2^-39 max|a| max|w|.  n 2^-24 is
          the worst case of any summation order.  Derived, not measured; the observed ratios are printed (RATIO lines).

Every launch: the output lies inside a larger allocation, pre-filled with a large finite value, with sentinel floats before
and behind it that must be unchanged; two calls on the same inputs agree bit for bit.  Kernels documented to give the same
bits are compared across the runs of a case (`same_bits`): the four loader / loop variants of the exact-fp32 kernels
(tests/test_gpu_nn.py test_igemm_loader_loop_variants) and the persistent against the one-tile 64 x 256 kernel
(tests/test_gpu_persistent_gemm.py).  The tap re-use kernel is documented to agree with the general one to rounding only
(tests/test_gpu_tap_kernels.py): on exact inputs both equal float64, on real inputs each meets the bars on its own."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

from xas_amd import _lib

U = 2.0 ** -24
PRE, SENT, SENT_V, FILL = 16, 16, -62500000.0, 1.5e30
DEV = 'cuda'
BK, TILE128_MIN_BLOCKS, X6P_MAX_K, X6P_ROUND = 32, 256, 4096, 768 * 4          # conv_shared.h / conv_x6.hip
PLAIN, GL, GENERAL, NO_WIDE, STEM_F32, NO_X6P = (_lib.TUNE_PLAIN_KLOOP, _lib.TUNE_GLOBAL_LOAD, _lib.TUNE_GENERAL_KERNELS,
                                                 _lib.TUNE_NO_WIDE_TILES, _lib.TUNE_STEM_FWD_F32, _lib.TUNE_NO_X6P)

Shape = collections.namedtuple('Shape', 'N Hi Wi Cin Cout R S stride pad Ho Wo')


def cdiv(a, b):
    return -(-a // b)


def mk(n, cin, h, w, cout, k, stride, pad):
    return Shape(n, h, w, cin, cout, k, k, stride, pad, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1)


# ------------------------------------------------------------------------------------------------ modes
# mode -> (precision, the operand maximum comes with the call, factor on the maximum)
MODE = {'f32': ('f32', False, 1.), 'bf16': ('bf16', False, 1.), 'bf16x6': ('bf16x6', False, 1.), 'f16x3': ('f16x3', True, 1.),
        'f16x3_loose': ('f16x3', True, 4.), 'f16x3_nomax': ('f16x3', False, 1.)}
ACCURATE = ('f32', 'bf16x6', 'f16x3', 'f16x3_nomax')


def pieces_of(mode):
    prec, amax, _ = MODE[mode]
    return {'f32': 0, 'bf16': 1, 'bf16x6': 3, 'f16x3': 2 if amax else 3}[prec]


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def thin_ok(s, C):
    return (s.R == 3 and s.S == 3 and s.stride == 1 and s.pad == 1 and C % 4 == 0 and 4 <= C <= 64 and 256 % (C // 4) == 0
            and s.Ho == s.Hi and s.Wo == s.Wi)


def is_thin(s):
    return (s.Cout == 1 and thin_ok(s, s.Cin)) or (s.Cin == 1 and thin_ok(s, s.Cout))


def is_stem(s):
    return (s.Cin, s.R, s.S, s.stride, s.pad, s.Cout) == (3, 7, 7, 2, 3, 64)


def route(s, pass_, mode, tune, has_bias):
    """fwd_route / dgrad_route."""
    prec, amax, _ = MODE[mode]
    if pass_ == 0:
        if is_stem(s) and not has_bias:
            return 'stem_f16' if prec == 'f16x3' and amax and not tune & STEM_F32 else 'stem_f32'
        if is_thin(s):
            return 'thin_vec_to_scalar' if s.Cout == 1 else 'thin_scalar_to_vec'
        return 'mfma' if s.Cin % BK == 0 and s.Cout >= 16 else 'direct'
    if is_thin(s):
        return 'thin_vec_to_scalar' if s.Cin == 1 else 'thin_scalar_to_vec'
    return 'mfma' if s.Cout % BK == 0 and s.Cin >= 16 else 'direct'


def pick_tile(Cd, rows, phases, wide=False):
    if Cd >= 96:
        if cdiv(rows, 128) * cdiv(Cd, 128) * phases <= TILE128_MIN_BLOCKS:
            return 64, 64
        return (64, 256) if wide and Cd % 256 == 0 else (128, 128)
    return (128, 64) if Cd >= 48 else (128, 32)


def phase_rows(s, pass_):
    """Rows of every launch phase (forward: one; data gradient: the pixels of dx of each of the stride^2 phases)."""
    if pass_ == 0:
        return [s.N * s.Ho * s.Wo]
    st = s.stride
    return [s.N * ((s.Hi - ph + st - 1) // st) * ((s.Wi - pw + st - 1) // st) for ph in range(st) for pw in range(st)]


def phase_ksteps(s, pass_):
    """K-steps of every phase: taps of the phase x 32-channel chunks of the gathered tensor."""
    if pass_ == 0:
        return [s.R * s.S * s.Cin // BK]
    st, out = s.stride, []
    for ph in range(st):
        for pw in range(st):
            br, bs = (ph + s.pad) % st, (pw + s.pad) % st
            nr = (s.R - br + st - 1) // st if br < s.R else 0
            ns = (s.S - bs + st - 1) // st if bs < s.S else 0
            out.append(nr * ns * s.Cout // BK)
    return out


def plan(s, pass_, mode, tune=0, has_bias=False):
    """conv_fwd_impl / conv_dgrad_impl -> what the launch runs.  Gathered tensor (Hs, Ws, Cs), produced tensor (Hd, Wd, Cd)."""
    r = route(s, pass_, mode, tune, has_bias)
    if r != 'mfma':
        return dict(route=r)
    Hs, Ws, Cs, Hd, Wd, Cd = (s.Hi, s.Wi, s.Cin, s.Ho, s.Wo, s.Cout) if pass_ == 0 else (s.Ho, s.Wo, s.Cout, s.Hi, s.Wi, s.Cin)
    rows_ph = phase_rows(s, pass_)
    rows, phases = max(rows_ph), len(rows_ph)
    P = pieces_of(mode)
    p = dict(route=r, phases=phases, pieces=P, pipelined=0, patch_width=0, tpb=0)
    if P == 0:
        bm, bn = pick_tile(Cd, rows, phases)
        buf = not tune & GL                                               # (every tensor of the table is far below 2 GiB)
        short_k = s.stride == 1 and s.R * s.S * Cs <= 2 * BK
        p.update(kernel='igemm_buf' if buf else 'igemm', pipelined=0 if (tune & PLAIN or (buf and short_k)) else 1)
    else:
        bm, bn = pick_tile(Cd, rows, phases)
        tap_ok = ((s.R, s.S, s.stride, s.pad) == (3, 3, 1, 1) and (Hd, Wd) == (Hs, Ws) and Cs % 32 == 0 and Hd % 8 == 0
                  and (Wd % 16 == 0 or (Wd == 8 and s.N % 2 == 0)))
        p['kernel'] = 'igemm_x6'
        if not tune & GENERAL and bm == 128 and phases == 1 and tap_ok:
            p.update(kernel='igemm_x6t', patch_width=16 if Wd % 16 == 0 else 8)
        elif not tune & NO_WIDE:
            bm, bn = pick_tile(Cd, rows, phases, True)
            x6p = (not tune & NO_X6P and Cs <= X6P_MAX_K and (s.R, s.S, s.stride, s.pad) == (1, 1, 1, 0) and phases == 1
                   and Cs % (2 * BK) == 0 and (Hs, Ws) == (Hd, Wd) and MODE[mode][1] and Cd % 4 == 0)
            if P == 2 and bn == 256 and x6p:
                p.update(kernel='igemm_x6p', tpb=max(1, min(8, cdiv(rows, 64) * cdiv(Cd, 256) // X6P_ROUND)))
    p.update(tile=(bm, bn), m_tiles=cdiv(rows, bm), n_tiles=cdiv(Cd, bn), ragged_m=any(m % bm for m in rows_ph), ragged_n=Cd % bn != 0)
    return p


def path_key(pass_, p):
    if p['route'] != 'mfma':
        return pass_, p['route']
    k = p['kernel']
    if k in ('igemm_buf', 'igemm'):
        return pass_, k, p['tile'], 'pipe' if p['pipelined'] else 'plain'
    if k == 'igemm_x6':
        return pass_, k, p['tile'], p['pieces']
    if k == 'igemm_x6t':
        return pass_, k, p['tile'][1], p['patch_width'], p['pieces']
    return pass_, k, p['tpb']


def kernel_class(s, pass_, mode, tune):
    """xas_conv_kernel_class(s, pass): 0 no MFMA, 1 exact fp32, 2 bf16, 3 bf16x6, 4 f16x3 (the query assumes no bias)."""
    r = route(s, pass_, mode, tune, False)
    if r in ('stem_f16', 'stem_f32'):
        return 4 if r == 'stem_f16' else 1
    return {0: 1, 1: 2, 3: 3, 2: 4}[pieces_of(mode)] if r == 'mfma' else 0


def weight_planes(s, pass_, mode, tune):
    """xas_conv_weight_planes: fp32 packed weights (0) outside the MFMA route and in exact fp32."""
    return pieces_of(mode) if route(s, pass_, mode, tune, False) == 'mfma' else 0


def properties(s, pass_, p):
    """Edges of an exact-fp32 MFMA launch."""
    Cd = s.Cout if pass_ == 0 else s.Cin
    ks, rows = phase_ksteps(s, pass_), phase_rows(s, pass_)
    out = {'scalar epilogue'} if Cd % 4 else set()
    out |= {'ragged M'} if p['ragged_m'] else set()
    out |= {'ragged N'} if p['ragged_n'] else set()
    out |= {'single K-step'} if 1 in ks else set()
    out |= {'odd K-steps'} if any(k % 2 and k > 1 for k in ks) else set()
    out |= {'even K-steps'} if any(k % 2 == 0 and k > 0 for k in ks) else set()
    out |= {'phase without taps'} if 0 in ks else set()
    out |= {'unequal phases'} if len(set(rows)) == 4 else set()
    out |= {'several M-tiles'} if p['m_tiles'] > 1 else set()
    out |= {'several N-tiles'} if p['n_tiles'] > 1 else set()
    return out


# ------------------------------------------------------------------------------------------------ the case table
# A claim on the MFMA route is COMPLETE (CLAIM_KEYS, checked by the table test): the case gives the tile grid (grid()), its
# runs give kernel, loop, pieces, patch width and tpb.  Off the MFMA route the claim is the route.
Run = collections.namedtuple('Run', 'mode tune claim')
Case = collections.namedtuple('Case', 'id pass_ shape runs claim bias no_bias same_bits heavy devref')
CASES = []
CLAIM_KEYS = {'route', 'kernel', 'tile', 'pipelined', 'phases', 'pieces', 'patch_width', 'tpb', 'm_tiles', 'n_tiles', 'ragged_m', 'ragged_n'}
F32_LOOPS = ((0, 'igemm_buf', 1), (PLAIN, 'igemm_buf', 0), (GL, 'igemm', 1), (GL | PLAIN, 'igemm', 0))
SPLIT = ('bf16x6', 'f16x3', 'f16x3_loose', 'bf16')
ANY = ('f32', 'bf16x6')                                    # kernels that do not look at the mode


def case(cid, pass_, shape, runs, claim=None, bias=True, no_bias=True, same_bits=False, heavy=False, devref=False):
    """bias / no_bias: the forward runs with / without a bias (a data gradient has none)."""
    CASES.append(Case(cid, pass_, mk(*shape), tuple(runs), claim or {}, bias and pass_ == 0, no_bias or pass_ == 1, same_bits, heavy, devref))


def grid(tile, m_tiles, ragged_m, n_tiles, ragged_n, phases=1):
    return dict(route='mfma', tile=tile, m_tiles=m_tiles, ragged_m=ragged_m, n_tiles=n_tiles, ragged_n=ragged_n, phases=phases)


def f32_runs(short_k=False):
    """The four loader / loop variants of the exact-fp32 kernels; short_k: the shipped buffer-load kernel runs its plain loop."""
    return [Run('f32', t, dict(kernel=k, pipelined=0 if (short_k and k == 'igemm_buf') else l, pieces=0, patch_width=0, tpb=0))
            for t, k, l in F32_LOOPS]


def split_runs(tunes=(0,), claims=None, modes=SPLIT, kernel='igemm_x6'):
    """Split arithmetic: `kernel` with no patches and no tpb unless the claims of a tuning flag say otherwise."""
    return [Run(m, t, dict(dict(kernel=kernel, patch_width=0, tpb=0), pipelined=0, pieces=pieces_of(m), **(claims or {}).get(t, {})))
            for t in tunes for m in modes]


def any_runs(r):
    return [Run(m, 0, dict(route=r)) for m in ANY]


def both(cid, n, cs, h, w, cd, k, stride, pad, runs, claim=None, claim1=None, **kw):
    """One GEMM problem in both passes: forward Cin = cs -> Cout = cd, data gradient of the convolution Cin = cd <- Cout = cs
    (cs channels gathered, cd produced, h x w the convolution's input either way).  claim1: what differs in the data gradient."""
    case(cid + '_fwd', 0, (n, cs, h, w, cd, k, stride, pad), runs, claim, **kw)
    case(cid + '_dgrad', 1, (n, cd, h, w, cs, k, stride, pad), runs, dict(claim or {}, **(claim1 or {})), **kw)


# ---- exact fp32: igemm_buf_kernel and igemm_kernel, pipelined and plain loop, every tile
both('f32_128x32', 2, 32, 12, 12, 20, 3, 1, 1, f32_runs(), grid((128, 32), 3, True, 1, True), same_bits=True, heavy=True)
both('f32_128x32_scalar_epilogue', 2, 32, 12, 12, 18, 3, 1, 1, f32_runs(), grid((128, 32), 3, True, 1, True), same_bits=True)
both('f32_128x64', 2, 32, 12, 12, 72, 3, 1, 1, f32_runs(), grid((128, 64), 3, True, 2, True), same_bits=True)
both('f32_64x64_s2', 2, 128, 17, 13, 100, 3, 2, 1, f32_runs(), grid((64, 64), 2, True, 2, True), dict(phases=4), same_bits=True, heavy=True)
both('f32_128x128', 5, 32, 63, 63, 224, 3, 1, 1, f32_runs(), grid((128, 128), 156, True, 2, True), same_bits=True)
both('f32_short_k_cin32', 2, 32, 9, 7, 20, 1, 1, 0, f32_runs(True), grid((128, 32), 1, True, 1, True), same_bits=True)
both('f32_short_k_cin64', 3, 64, 9, 7, 72, 1, 1, 0, f32_runs(True), grid((128, 64), 2, True, 2, True), same_bits=True)
both('f32_long_k_cin96', 3, 96, 9, 7, 72, 1, 1, 0, f32_runs(), grid((128, 64), 2, True, 2, True), same_bits=True)      # one step beyond short_k
# ---- data-gradient geometry, exact fp32 and split arithmetic: four phases, one ragged 128 x 32 tile each
GEOMETRY = [('s2_1x1', (2, 32, 9, 7, 32, 1, 2, 0)),                     # three of four pixels: no tap
            ('rows_without_taps', (2, 32, 8, 10, 32, 3, 2, 0)),         # Hi 8 > (3 - 1) * 2 + 3, Wi 10 > 9
            ('transposed_4x4s2', (2, 32, 8, 8, 64, 4, 2, 1))]
for name_, shape_ in GEOMETRY:
    case('geometry_%s_f32' % name_, 1, shape_, f32_runs(), grid((128, 32), 1, True, 1, False, 4), same_bits=True)
    case('geometry_%s_split' % name_, 1, shape_, split_runs(), grid((128, 32), 1, True, 1, False, 4), heavy=name_ == 's2_1x1')
# ---- igemm_x6_kernel: five tiles, P = 1, 2, 3
both('x6_128x32', 2, 32, 12, 12, 20, 3, 1, 1, split_runs(), grid((128, 32), 3, True, 1, True), heavy=True)
both('x6_128x64', 2, 32, 12, 12, 72, 3, 1, 1, split_runs(), grid((128, 64), 3, True, 2, True))
both('x6_64x64_s2', 2, 128, 17, 13, 100, 3, 2, 1, split_runs(), grid((64, 64), 2, True, 2, True), dict(phases=4))
both('x6_128x128', 5, 32, 63, 63, 224, 3, 1, 1, split_runs(), grid((128, 128), 156, True, 2, True))
WIDE = {0: dict(tile=(64, 256), m_tiles=272, n_tiles=1), NO_WIDE: dict(tile=(128, 128), m_tiles=136, n_tiles=2)}
both('x6_64x256_3x3', 5, 32, 59, 59, 256, 3, 1, 1, split_runs((0, NO_WIDE), WIDE), dict(route='mfma', ragged_m=True, ragged_n=False, phases=1))
both('x6_64x256_1x1_cin32', 5, 32, 59, 59, 256, 1, 1, 0, split_runs((0, NO_WIDE), WIDE), dict(route='mfma', ragged_m=True, ragged_n=False, phases=1))
# ---- igemm_x6t_kernel: BN 32 / 64 / 128, patch width 16 / 8, P = 1, 2, 3; the same shapes with the kernel switched off
TAP = [('bn32_w8_one_patch', (2, 32, 8, 8, 32, 3, 1, 1), 8, grid((128, 32), 1, False, 1, False)),
       ('bn64_w16_one_patch', (1, 32, 8, 16, 64, 3, 1, 1), 16, grid((128, 64), 1, False, 1, False)),
       ('bn32_w16', (3, 32, 16, 32, 32, 3, 1, 1), 16, grid((128, 32), 12, False, 1, False)),
       ('bn64_w8', (6, 64, 16, 8, 64, 3, 1, 1), 8, grid((128, 64), 6, False, 1, False)),
       ('bn32_ragged_n', (2, 32, 8, 8, 40, 3, 1, 1), 8, grid((128, 32), 1, False, 2, True)),
       ('bn128', (9, 32, 64, 64, 96, 3, 1, 1), 16, grid((128, 128), 288, False, 1, True))]
for name_, (n_, cs_, h_, w_, cd_, k_, st_, pd_), tw_, grid_ in TAP:
    both('x6t_' + name_, n_, cs_, h_, w_, cd_, k_, st_, pd_,
         split_runs((0, GENERAL), {0: dict(kernel='igemm_x6t', patch_width=tw_), GENERAL: dict(kernel='igemm_x6', patch_width=0)}), grid_,
         heavy=name_ == 'bn64_w8')
both('x6t_w8_odd_n_refused', 3, 32, 8, 8, 32, 3, 1, 1, split_runs(), grid((128, 32), 2, True, 1, False))
# ---- igemm_x6p_kernel: f16x3 with the operand maximum; switched off, without the maximum and at Cin 96: the 64 x 256 general kernel
F16 = ('f16x3', 'f16x3_loose')
X6P = {0: dict(kernel='igemm_x6p', tpb=1), NO_X6P: dict(kernel='igemm_x6', tpb=0)}
both('x6p_tpb1', 5, 64, 59, 59, 256, 1, 1, 0, split_runs((0, NO_X6P), X6P, F16), grid((64, 256), 272, True, 1, False), same_bits=True, heavy=True)
both('x6p_without_maximum', 5, 64, 59, 59, 256, 1, 1, 0, split_runs(modes=('f16x3_nomax', 'bf16x6', 'bf16')), grid((64, 256), 272, True, 1, False))
both('x6p_cin96_refused', 5, 96, 59, 59, 256, 1, 1, 0, split_runs(modes=F16), grid((64, 256), 272, True, 1, False))
# (1551 M-tiles x 4 N-tiles = 6204 tiles: two per block, 776 groups, the last of one tile; the reference is computed on the device)
case('x6p_tpb2_short_last_group', 0, (25, 64, 63, 63, 1024, 1, 1, 0), split_runs(claims={0: dict(kernel='igemm_x6p', tpb=2)}, modes=('f16x3',)),
     grid((64, 256), 1551, True, 4, False), devref=True)
# ---- both stem forward kernels (no bias); with a bias the stem shape runs direct_fwd_kernel in every mode
STEM_RUNS = [Run('f32', 0, dict(route='stem_f32')), Run('f16x3_nomax', 0, dict(route='stem_f32')), Run('bf16x6', 0, dict(route='stem_f32')),
             Run('f16x3', STEM_F32, dict(route='stem_f32')), Run('f16x3', 0, dict(route='stem_f16')), Run('f16x3_loose', 0, dict(route='stem_f16'))]
STEM_BIAS_RUNS = [Run(m, 0, dict(route='direct')) for m in ('f32', 'f16x3', 'bf16x6')]
case('stem_one_tile', 0, (1, 3, 16, 32, 64, 7, 2, 3), STEM_RUNS, bias=False)
case('stem_partial_tiles', 0, (3, 3, 50, 70, 64, 7, 2, 3), STEM_RUNS, bias=False, heavy=True)
case('stem_with_bias_one_tile', 0, (1, 3, 16, 32, 64, 7, 2, 3), STEM_BIAS_RUNS, no_bias=False)
case('stem_with_bias_partial_tiles', 0, (3, 3, 50, 70, 64, 7, 2, 3), STEM_BIAS_RUNS, no_bias=False, heavy=True)
# ---- direct_fwd_kernel, direct_dgrad_kernel
both('direct_cin12', 2, 12, 9, 7, 20, 3, 1, 1, any_runs('direct'), heavy=True)
both('direct_cout8', 2, 32, 9, 7, 8, 3, 1, 1, any_runs('direct'))
both('direct_s2', 2, 12, 9, 7, 20, 3, 2, 1, any_runs('direct'))
# ---- thin kernels, both orientations, both passes
for C_, n_, h_, w_ in ((4, 1, 3, 5), (8, 2, 7, 9), (64, 3, 33, 21)):
    case('thin_cout1_C%d_fwd' % C_, 0, (n_, C_, h_, w_, 1, 3, 1, 1), any_runs('thin_vec_to_scalar'), heavy=C_ == 64)
    case('thin_cin1_C%d_fwd' % C_, 0, (n_, 1, h_, w_, C_, 3, 1, 1), any_runs('thin_scalar_to_vec'), heavy=C_ == 64)
    case('thin_cin1_C%d_dgrad' % C_, 1, (n_, 1, h_, w_, C_, 3, 1, 1), any_runs('thin_vec_to_scalar'), heavy=C_ == 64)
    case('thin_cout1_C%d_dgrad' % C_, 1, (n_, C_, h_, w_, 1, 3, 1, 1), any_runs('thin_scalar_to_vec'), heavy=C_ == 64)

CASE_IDS = [c.id for c in CASES]
F32_TILES = ((128, 32), (128, 64), (64, 64), (128, 128))
X6_TILES = F32_TILES + ((64, 256),)
BOTH = (0, 1)
REQUIRED = ({(ps, k, t, l) for ps in BOTH for k in ('igemm_buf', 'igemm') for t in F32_TILES for l in ('pipe', 'plain')}
            | {(ps, 'igemm_x6', t, P) for ps in BOTH for t in X6_TILES for P in (1, 2, 3)}
            | {(ps, 'igemm_x6t', bn, tw, P) for ps in BOTH for bn, tw in ((32, 16), (32, 8), (64, 16), (64, 8), (128, 16)) for P in (1, 2, 3)}
            | {(0, 'igemm_x6p', 1), (1, 'igemm_x6p', 1), (0, 'igemm_x6p', 2)}
            | {(0, 'stem_f16'), (0, 'stem_f32'), (0, 'direct'), (1, 'direct')}
            | {(ps, r) for ps in BOTH for r in ('thin_vec_to_scalar', 'thin_scalar_to_vec')})
PROPERTIES = {'scalar epilogue', 'ragged M', 'ragged N', 'single K-step', 'odd K-steps', 'even K-steps', 'phase without taps',
              'unequal phases', 'several M-tiles', 'several N-tiles'}


# ------------------------------------------------------------------------------------------------ inputs and float64
def conv64(s, pass_, a, w):
    """float64 reference: forward of x = a, or the data gradient (input gradient) of dy = a."""
    if pass_ == 0:
        return F.conv2d(a, w, None, s.stride, s.pad)
    return torch.nn.grad.conv2d_input((s.N, s.Cin, s.Hi, s.Wi), w, a, s.stride, s.pad)


def term_count(s, pass_):
    """[1][1][H][W] of the produced tensor: the non-padding terms of an element (taps inside the image x gathered channels)."""
    one = Shape(1, s.Hi, s.Wi, 1, 1, s.R, s.S, s.stride, s.pad, s.Ho, s.Wo)
    ones = torch.ones((1, 1, s.Hi, s.Wi) if pass_ == 0 else (1, 1, s.Ho, s.Wo), dtype=torch.float64)
    return conv64(one, pass_, ones, torch.ones(1, 1, s.R, s.S, dtype=torch.float64)) * (s.Cin if pass_ == 0 else s.Cout)


def operand_dims(s, pass_):
    return (s.N, s.Cin, s.Hi, s.Wi) if pass_ == 0 else (s.N, s.Cout, s.Ho, s.Wo)


def integers(g, *dims):
    """Integers |v| <= 3, 4 % exact zeros, 6 % all-zero pixels (channel vectors)."""
    v = torch.randint(1, 4, dims, generator=g) * (2 * torch.randint(0, 2, dims, generator=g) - 1)
    v[torch.rand(dims, generator=g) < 0.04] = 0
    if len(dims) == 4:
        v[(torch.rand(dims[0], 1, dims[2], dims[3], generator=g) < 0.06).expand(dims)] = 0
    return v.double()


@functools.lru_cache(maxsize=None)
def exact_inputs(s, pass_, devref=False):
    """a (x or dy, NCHW float64), w (OIHW), bias, float64 result, sum |term|, term count.  Drawn again until every element
    with 16 terms or more and a non-zero term has terms of both signs.  devref: no reference here (the device computes it)."""
    n = term_count(s, pass_)
    for attempt in range(400):
        g = torch.Generator().manual_seed(1000 * (sum(s) + 7 * s.Cin + 3 * s.Wi + pass_) + attempt)
        a, w = integers(g, *operand_dims(s, pass_)), integers(g, s.Cout, s.Cin, s.R, s.S)
        bias = torch.randint(-3, 4, (s.Cout,), generator=g).double()
        if devref:
            return a, w, bias, None, None, n
        ref, mag = conv64(s, pass_, a, w), conv64(s, pass_, a.abs(), w.abs())
        zero_pixel = a.shape[0] * a.shape[2] * a.shape[3] < 40 or bool((a == 0).all(1).any())
        if zero_pixel and bool(((ref.abs() < mag) | (n < 16) | (mag == 0)).all()):
            return a, w, bias, ref, mag, n
    raise AssertionError('no exact input with both signs in every receptive field: %s pass %d' % (s, pass_))


@functools.lru_cache(maxsize=None)
def real_inputs(s, pass_, heavy):
    """fp32 values as float64: forward x = 1.5 randn + 0.3, data gradient dy = randn (heavy: times exp(2 randn)),
    w = randn / sqrt(fan-in), bias = randn; float64 result and sum |term| without the bias."""
    g = torch.Generator().manual_seed(sum(s) + 13 * s.Cout + pass_)
    dims = operand_dims(s, pass_)
    a = torch.randn(dims, generator=g) * 1.5 + 0.3 if pass_ == 0 else torch.randn(dims, generator=g)
    if heavy:
        a = a * torch.exp(torch.randn(dims, generator=g) * 2.0)
    w = torch.randn(s.Cout, s.Cin, s.R, s.S, generator=g) / (s.Cin * s.R * s.S) ** 0.5
    a, w, bias = a.float().double(), w.float().double(), torch.randn(s.Cout, generator=g).float().double()
    return a, w, bias, conv64(s, pass_, a, w), conv64(s, pass_, a.abs(), w.abs())


# ------------------------------------------------------------------------------------------------ the library's answers
def host_shape(s, mode, amax_ptr=16):
    """ConvShape of a call in `mode`; amax_ptr: the device pointer of the operand maximum where the mode carries one (the
    queries never dereference it: any non-null value serves on a machine without a GPU)."""
    prec, amax, _ = MODE[mode]
    return _lib.ConvShape(*s, 1 + _lib.PREC_NAMES[prec], amax_ptr if amax else None, None)


def library_plan(shp, pass_, tune, has_bias):
    _lib.query('xas_set_tuning', tune)
    try:
        return (_lib.conv_igemm_plan(shp, pass_, has_bias), _lib.query('xas_conv_kernel_class', shp, pass_),
                _lib.query('xas_conv_weight_planes', shp, pass_))
    finally:
        _lib.query('xas_set_tuning', 0)


def check_library_agrees(c, run, shp, has_bias):
    """xas_conv_igemm_plan, xas_conv_kernel_class and xas_conv_weight_planes under the run's flags against the restated plan."""
    p = plan(c.shape, c.pass_, run.mode, run.tune, has_bias)
    got, cls, planes = library_plan(shp, c.pass_, run.tune, has_bias)
    want = dict(route=p['route'], kernel=p.get('kernel'), bm=p.get('tile', (0, 0))[0], bn=p.get('tile', (0, 0))[1],
                pipelined=p.get('pipelined', 0), phases=p.get('phases', 0), pieces=p.get('pieces', 0),
                patch_width=p.get('patch_width', 0), tpb=p.get('tpb', 0), images=c.shape.N)
    assert got == want, '%s %s tune %#x: the library plans %r, restated %r' % (c.id, run.mode, run.tune, got, want)
    assert cls == kernel_class(c.shape, c.pass_, run.mode, run.tune), (c.id, run, cls)
    assert planes == weight_planes(c.shape, c.pass_, run.mode, run.tune), (c.id, run, planes)
    return p


def bias_forms(c):
    """has_bias of the launches of a case: a forward runs without and with a bias unless the case says otherwise."""
    return ([False] if c.no_bias else []) + ([True] if c.bias else [])


# ------------------------------------------------------------------------------------------------ the CPU-only check
def test_case_table_reaches_every_path():
    """No GPU: the restated plan sends every run of every case where it claims and equals the library's plan, kernel class
    and weight format; the claimed paths are exactly REQUIRED; the edges of PROPERTIES all occur on the exact-fp32 kernels,
    in both passes; every exact input meets its precondition."""
    _lib.load()
    reached, props, stem_with_bias = set(), {0: set(), 1: set()}, set()
    for c in CASES:
        assert c.bias or c.no_bias, c.id
        for run in c.runs:
            for has_bias in bias_forms(c):
                p = check_library_agrees(c, run, host_shape(c.shape, run.mode), has_bias)
                claim = dict(c.claim, **run.claim)
                assert set(claim) == (CLAIM_KEYS if p['route'] == 'mfma' else {'route'}), '%s: the claim leaves out %s' % (c.id, CLAIM_KEYS - set(claim))
                for k, v in claim.items():
                    assert p[k] == v, '%s (%s, tune %#x): %s is %r, claimed %r  [%r]' % (c.id, run.mode, run.tune, k, p[k], v, p)
                reached.add(path_key(c.pass_, p))
                if is_stem(c.shape) and has_bias:
                    stem_with_bias.add((p['route'], c.shape.Ho % 8 == 0 and c.shape.Wo % 16 == 0))
                if p.get('kernel') in ('igemm_buf', 'igemm'):
                    props[c.pass_] |= properties(c.shape, c.pass_, p)
        a, w, bias, ref, mag, n = exact_inputs(c.shape, c.pass_, c.devref)
        for t in (a, w, bias):
            assert float(t.abs().max()) <= 3 and bool((t == t.round()).all()), c.id
        assert bool((a == 0).all(1).any()) or a.shape[0] * a.shape[2] * a.shape[3] < 40, c.id                 # all-zero pixels
        if c.devref:
            assert 9 * float(n.max()) + 3 < 2 ** 24, c.id
            continue
        assert float(mag.max()) + 3 < 2 ** 24, c.id
        assert bool(((ref.abs() < mag) | (n < 16) | (mag == 0)).all()), c.id
        assert bool((ref[(n == 0).expand_as(ref)] == 0).all()), c.id
    assert stem_with_bias == {('direct', True), ('direct', False)}          # the stem shape with a bias, full and partial 8 x 16 tiles
    assert reached == REQUIRED, 'not reached: %s; not required: %s' % (sorted(map(str, REQUIRED - reached)), sorted(map(str, reached - REQUIRED)))
    assert props[0] == PROPERTIES - {'phase without taps', 'unequal phases'}, PROPERTIES - props[0]
    assert props[1] == PROPERTIES, PROPERTIES - props[1]
    # dx pixels that no tap reaches exist where the table says so
    for name_, shape_ in GEOMETRY[:2]:
        assert bool((term_count(mk(*shape_), 1) == 0).any()), name_
    assert int((term_count(mk(*GEOMETRY[0][1]), 1) == 0).sum()) == 9 * 7 - 5 * 4       # 1 x 1 stride 2: only the even pixels get a tap


# ------------------------------------------------------------------------------------------------ plumbing (GPU)
gpu = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _library_back(request):
    def back():
        if _lib._lib is not None:
            _lib.query('xas_set_tuning', 0)
    request.addfinalizer(back)


class Buf:
    """PRE sentinel floats, n floats (pre-filled), SENT sentinel floats, in one allocation."""

    def __init__(self, n, fill=FILL, src=None):
        self.n = n
        self.all = torch.full((PRE + n + SENT,), fill, device=DEV)
        self.all[:PRE] = SENT_V
        self.all[PRE + n:] = SENT_V
        self.t = self.all[PRE:PRE + n]
        if src is not None:
            self.t.copy_(src.reshape(-1))
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        assert bool((self.all[:PRE] == SENT_V).all()) and bool((self.all[PRE + self.n:] == SENT_V).all()), \
            'floats around a buffer of %d were written' % self.n

    def untouched(self):
        self.intact()
        return bool((self.t == FILL).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


def device_shape(s, mode, operand):
    """ConvShape of a launch in `mode`: f16x3 with the measured maximum of the gathered operand, or four times it."""
    _, amax, factor = MODE[mode]
    if not amax:
        return host_shape(s, mode)
    slot = torch.zeros(1024, device=DEV)                    # an amax slot (xas_hip.h XAS_AMAX_SLOT_FLOATS) holding one maximum
    slot[0] = operand.abs().max() * factor
    shp = host_shape(s, mode, slot.data_ptr())
    shp._slot = slot
    return shp


def weights_for(s, pass_, w_dev, shp):
    """The weight buffer the entry points of `pass_` want for this shape: packed fp32, or split planes of the packed weight."""
    planes = _lib.query('xas_conv_weight_planes', shp, pass_)
    packed = torch.empty(w_dev.numel(), device=DEV)
    _lib.call('xas_pack_weight', w_dev.data_ptr(), packed.data_ptr(), s.Cout, s.Cin, s.R, s.S, pass_)
    if not planes:
        return packed
    rows = s.Cin if pass_ else s.Cout
    kk = packed.numel() // rows
    split = torch.empty(_lib.query('xas_split_weight_bytes', rows, kk, planes), device=DEV, dtype=torch.uint8)
    _lib.call('xas_split_weight', packed.data_ptr(), split.data_ptr(), rows, kk, planes)
    split._packed = packed
    return split


class Launcher:
    """The operands of a case on the device and its launches; every launch checks the sentinels round its output."""

    def __init__(self, c, a, w):
        self.c, self.s = c, c.shape
        self.a, self.w = nhwc(a), w.float().to(DEV).contiguous()
        s = c.shape
        self.out_dims = (s.N, s.Ho, s.Wo, s.Cout) if c.pass_ == 0 else (s.N, s.Hi, s.Wi, s.Cin)
        self.n_out = self.out_dims[0] * self.out_dims[1] * self.out_dims[2] * self.out_dims[3]

    def prepare(self, run, has_bias=False):
        self.run = run
        self.shp = device_shape(self.s, run.mode, self.a)
        self.plan = check_library_agrees(self.c, run, self.shp, has_bias)
        self.wbuf = weights_for(self.s, self.c.pass_, self.w, self.shp)

    def go(self, entry, *extra, prev=None):
        out = Buf(self.n_out, src=prev)
        _lib.query('xas_set_tuning', self.run.tune)
        try:
            if entry == 'xas_conv_fwd':
                bias, = extra
                _lib.call(entry, self.a.data_ptr(), self.wbuf.data_ptr(), None if bias is None else bias.data_ptr(), out.ptr(), self.shp)
            else:
                _lib.call(entry, self.a.data_ptr(), self.wbuf.data_ptr(), out.ptr(), self.shp, *extra)
        finally:
            _lib.query('xas_set_tuning', 0)
        torch.cuda.synchronize()
        out.intact()
        return out.t.view(self.out_dims).clone()


def forms_of(c, L, bias, prev, dprev, mask):
    """name -> (launch, float64 addend of the reference, extra term) for every form the case runs in the prepared run."""
    if c.pass_ == 0:
        forms = {'fwd': (lambda: L.go('xas_conv_fwd', None), None)} if c.no_bias else {}
        if c.bias:
            forms['fwd_bias'] = (lambda: L.go('xas_conv_fwd', bias), bias.double().view(1, 1, 1, -1))
        return forms
    forms = {'dgrad': (lambda: L.go('xas_conv_dgrad'), None)}
    if L.plan['route'] == 'mfma' and c.shape.Cin % 4 == 0:
        on = torch.stack([(mask >> e) & 1 for e in range(4)], 1).reshape(prev.shape).double()
        forms['dgrad_acc'] = (lambda: L.go('xas_conv_dgrad_acc', prev=prev), prev.double())
        forms['dgrad_acc_masked'] = (lambda: L.go('xas_conv_dgrad_acc_masked', dprev.data_ptr(), mask.data_ptr()), on * dprev.double())
    return forms


def addends(c, L, integer):
    """bias [Cout], prev and dprev [like the result], one mask byte per float4 (all-zero and all-one bytes among them)."""
    g = torch.Generator().manual_seed(5 + L.n_out)
    draw = (lambda *d: torch.randint(-3, 4, d, generator=g).float()) if integer else (lambda *d: torch.randn(d, generator=g))
    mask = torch.randint(0, 16, (max(1, L.n_out // 4),), generator=g, dtype=torch.uint8)
    mask[::7] = 0
    mask[3::11] = 15
    return draw(c.shape.Cout).to(DEV), draw(*L.out_dims).to(DEV), draw(*L.out_dims).to(DEV), mask.to(DEV)


# ------------------------------------------------------------------------------------------------ exact inputs
@gpu
@pytest.mark.parametrize('c', CASES, ids=CASE_IDS)
def test_exact(c):
    """Integers: every run, every form EQUALS float64 (prev + ref, ref + mask * dprev for the accumulating forms); a second
    call gives the same bits; the runs of a same_bits case agree bit for bit; sentinels intact (Launcher.go)."""
    s = c.shape
    a, w, bias64, ref, mag, n = exact_inputs(s, c.pass_, c.devref)
    L = Launcher(c, a, w)
    if c.devref:                                            # 1 x 1: a float64 matmul on the device
        ref_d = (L.a.double().view(-1, s.Cin) @ L.w.double().view(s.Cout, s.Cin).t()).view(L.out_dims)
        mag_d = (L.a.double().abs().view(-1, s.Cin) @ L.w.double().abs().view(s.Cout, s.Cin).t()).view(L.out_dims)
        assert bool(((ref_d.abs() < mag_d) | (mag_d == 0)).all()) and float(mag_d.max()) + 3 < 2 ** 24
        del mag_d
    else:
        ref_d = ref.permute(0, 2, 3, 1).contiguous().to(DEV)
    bias, prev, dprev, mask = addends(c, L, True)
    bias.copy_(bias64)
    first = {}
    for run in c.runs:
        L.prepare(run, not c.no_bias)
        for name, (go, add) in forms_of(c, L, bias, prev, dprev, mask).items():
            if name == 'fwd_bias':
                L.prepare(run, True)
            o = go()
            want = ref_d if add is None else ref_d + add
            bad = (o.double() != want).nonzero()
            assert bad.numel() == 0, '%s %s tune %#x %s: %d of %d elements differ, first at %s: %r, float64 %r' % (
                c.id, run.mode, run.tune, name, bad.shape[0], o.numel(), bad[0].tolist(), float(o[tuple(bad[0])]), float(want[tuple(bad[0])]))
            assert torch.equal(bits(go()), bits(o)), '%s %s tune %#x %s: second call' % (c.id, run.mode, run.tune, name)
            if c.same_bits:
                k = (run.mode, name)
                assert torch.equal(bits(first.setdefault(k, o)), bits(o)), '%s %s %s: tune %#x differs in its bits' % (c.id, run.mode, name, run.tune)
            del o, want


# ------------------------------------------------------------------------------------------------ real inputs
def bars(o, ref, T, n, cterm, floor):
    """-> Frobenius-relative error, largest element error / ((n 2^-24 + c) T + n floor)."""
    err = (o.double() - ref).abs()
    bar = (n * U + cterm) * T + n * floor
    r = torch.where(bar > 0, err / torch.where(bar > 0, bar, torch.ones_like(bar)), torch.where(err > 0, float('inf'), 0.).double())
    return float(err.norm() / ref.norm()), float(r.max())


def c_of(p):
    """(c, per-term floor in units of max|a| max|w|) of the arithmetic a plan runs in."""
    pieces = 2 if p['route'] == 'stem_f16' else p.get('pieces', 0)
    return {0: (0., 0.), 3: (2.0 ** -23, 0.), 2: (2.0 ** -21, 2.0 ** -39)}[pieces]


@gpu
@pytest.mark.parametrize('c', [c for c in CASES if not c.devref], ids=[c.id for c in CASES if not c.devref])
def test_real(c):
    """Real values in the fp32-accurate modes against both bars; heavy-tailed operands too where the case is marked."""
    s = c.shape
    for heavy in ((False, True) if c.heavy else (False,)):
        a, w, bias64, ref, T = real_inputs(s, c.pass_, heavy)
        L = Launcher(c, a, w)
        ref_d, T_d = (t.permute(0, 2, 3, 1).contiguous().to(DEV) for t in (ref, T))
        n = term_count(s, c.pass_).permute(0, 2, 3, 1).to(DEV)
        amax_aw = float(a.abs().max()) * float(w.abs().max())
        bias, prev, dprev, mask = addends(c, L, False)
        bias.copy_(bias64)
        first = {}
        for run in c.runs:
            if run.mode not in ACCURATE:
                continue
            L.prepare(run, not c.no_bias)
            for name, (go, add) in forms_of(c, L, bias, prev, dprev, mask).items():
                if name == 'fwd_bias':
                    L.prepare(run, True)
                cterm, floor = c_of(L.plan)                 # (the plan of THIS form: a bias moves the stem shape to the direct kernel)
                o = go()
                assert bool(torch.isfinite(o).all())
                want, T1, n1 = (ref_d, T_d, n) if add is None else (ref_d + add, T_d + add.abs(), n + 1)
                frob, elem = bars(o, want, T1, n1, cterm, floor * amax_aw)
                key = '%s %s %s' % ('/'.join(str(v) for v in path_key(c.pass_, L.plan)), 'fp32' if cterm == 0 else run.mode, name)
                print('RATIO %-64s frobenius / 3e-6 = %.4f  element / bar = %.4f' % (key + (' heavy' if heavy else ''), frob / 3e-6, elem))
                assert frob < 3e-6 and elem <= 1, '%s %s tune %#x %s: Frobenius %.3e, element ratio %.3f' % (c.id, run.mode, run.tune, name, frob, elem)
                if c.same_bits:
                    k = (run.mode, name)
                    assert torch.equal(bits(first.setdefault(k, o)), bits(o)), '%s %s %s: tune %#x differs in its bits' % (c.id, run.mode, name, run.tune)


# ------------------------------------------------------------------------------------------------ refusals
@gpu
def test_refusals_launch_nothing():
    """Non-zero status, a message, the pre-filled output untouched: a 4-byte-misaligned x or weight pointer on the MFMA
    route (the check precedes the launch: nothing runs on a misaligned pointer), xas_conv_dgrad_acc on a direct and on a thin
    route, inconsistent Ho / Wo, Hi too small for Ho, null buffers."""
    good = mk(2, 32, 8, 8, 32, 3, 1, 1)
    st = _lib.stream()
    err = _lib.load().xas_last_error
    x = torch.ones(good.N * good.Hi * good.Wi * good.Cin + 4, device=DEV)
    wgt = torch.ones(1 << 16, device=DEV)
    mask = torch.zeros(1 << 14, device=DEV, dtype=torch.uint8)
    out = Buf(good.N * good.Hi * good.Wi * max(good.Cin, good.Cout))
    fwd, dgrad, acc, masked = (_lib.fn(n) for n in ('xas_conv_fwd', 'xas_conv_dgrad', 'xas_conv_dgrad_acc', 'xas_conv_dgrad_acc_masked'))
    xp, wp, op = x.data_ptr(), wgt.data_ptr(), out.ptr()
    assert xp % 16 == 0 and wp % 16 == 0

    def shp(s, mode='f32'):
        return host_shape(s, mode)
    direct, thin = mk(2, 3, 8, 8, 32, 3, 1, 1), mk(2, 8, 8, 8, 1, 3, 1, 1)
    assert plan(direct, 1, 'f32')['route'] == 'direct' and plan(thin, 1, 'f32')['route'] == 'thin_scalar_to_vec'
    calls = {}
    for mode in ('f32', 'bf16x6'):
        calls['fwd misaligned x ' + mode] = lambda mode=mode: fwd(xp + 4, wp, None, op, shp(good, mode), st)
        calls['fwd misaligned w ' + mode] = lambda mode=mode: fwd(xp, wp + 4, None, op, shp(good, mode), st)
        calls['dgrad misaligned dy ' + mode] = lambda mode=mode: dgrad(xp + 4, wp, op, shp(good, mode), st)
        calls['dgrad misaligned w ' + mode] = lambda mode=mode: dgrad(xp, wp + 4, op, shp(good, mode), st)
        calls['acc misaligned w ' + mode] = lambda mode=mode: acc(xp, wp + 4, op, shp(good, mode), st)
    calls['acc on a direct route'] = lambda: acc(xp, wp, op, shp(direct), st)
    calls['acc on a thin route'] = lambda: acc(xp, wp, op, shp(thin), st)
    calls['masked on a direct route'] = lambda: masked(xp, wp, op, shp(direct), xp, mask.data_ptr(), st)
    calls['fwd inconsistent Ho'] = lambda: fwd(xp, wp, None, op, shp(good._replace(Ho=7)), st)
    calls['fwd inconsistent Wo'] = lambda: fwd(xp, wp, None, op, shp(good._replace(Wo=9)), st)
    calls['dgrad Hi too small'] = lambda: dgrad(xp, wp, op, shp(good._replace(Hi=7)), st)
    calls['dgrad Wi too small'] = lambda: dgrad(xp, wp, op, shp(good._replace(Wi=6)), st)
    calls['acc Hi too small'] = lambda: acc(xp, wp, op, shp(good._replace(Hi=7)), st)
    for i, name in enumerate(('x', 'w', 'y')):
        args = [xp, wp, None, op]
        args[i if i < 2 else 3] = None
        calls['fwd null ' + name] = lambda args=args: fwd(*args, shp(good), st)
    for i, name in enumerate(('dy', 'w', 'dx')):
        args = [xp, wp, op]
        args[i] = None
        calls['dgrad null ' + name] = lambda args=args: dgrad(*args, shp(good), st)
        calls['acc null ' + name] = lambda args=args: acc(*args, shp(good), st)
    calls['masked null dprev'] = lambda: masked(xp, wp, op, shp(good), None, mask.data_ptr(), st)
    calls['masked null mask'] = lambda: masked(xp, wp, op, shp(good), xp, None, st)
    calls['fwd null shape'] = lambda: fwd(xp, wp, None, op, None, st)
    reasons = (('misaligned', '16-byte aligned'), ('route', 'only the MFMA path accumulates'), ('inconsistent', 'inconsistent with'),
               ('too small', 'too small for'), ('null shape', 'null shape'), ('null', 'null buffer'))
    for name, go in calls.items():
        reason = next(text for word, text in reasons if word in name)
        assert fwd(xp, wp, None, op, shp(good._replace(N=0)), st) != 0 and 'non-positive' in err().decode()      # another message first
        rc = go()
        torch.cuda.synchronize()
        assert rc != 0, '%s: accepted' % name
        assert reason in err().decode() and 'conv_' in err().decode(), '%s: refused with %r, not for %r' % (name, err().decode(), reason)
        assert out.untouched(), '%s wrote the output' % name
