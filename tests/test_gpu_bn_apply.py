"""The two element-wise batch-norm passes (xas_bn_apply_amax, xas_bn_bwd_apply_amax) ALONE against float64: mean, variance,
gamma, beta and the backward's two sums are handed in (the sums computed in float64 from the same inputs), so no reduction
kernel takes part.  Every case runs on both loop policies of csrc/bn.hip - the shipped dispatch rule and
TUNE_GENERAL_KERNELS - and covers every row of the dispatch table there plus what only the general policy accepts.

Bars (those of test_gpu_nn.test_batch_norm_train): y max-abs < 2e-5, dx relative < 2e-5, dres relative < 1e-6.  Sign
decisions (the sign bytes of the forward; in the backward the zeroed / scaled elements of dz) must be those of float64;
an element whose float64 pre-activation value lies within 1e-6 of 0 - but is not a planted exact zero - is taken out of
these comparisons (its fp32 value may round to the other side), and a case fails if that is more than 1 % of it.

The C = 2048 case: n4g is a multiple of C/4 = 512 there, so ceil(n4g / 256) is always even and the grid rounding for
C/4 > 256 acts only once the block cap is hit with a group count that makes the cap odd: 3 groups of 1366 rows
(cap 2731 -> 2732 blocks per group)."""
import pytest
import torch

from xas_amd import _lib

pytestmark = pytest.mark.gpu

EPS = 1e-5
SLOT = 1024            # floats of an amax slot (32 sub-maxima, 32 floats apart)
POLICIES = (('shipped', 0), ('general', _lib.TUNE_GENERAL_KERNELS))


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int32)


def pack_signs(pos):
    """[rows, C] bool -> one byte per float4, bit e = lane e."""
    p = pos.reshape(pos.shape[0], -1, 4).to(torch.uint8)
    return (p[..., 0] | (p[..., 1] << 1) | (p[..., 2] << 2) | (p[..., 3] << 3)).reshape(-1)


def make_case(M, C, G, act, res, seed, gamma_zero=False, dev='cpu'):
    """Inputs of one layer: x = 2 randn + 3 (mean far from 0), per-group statistics of x, a channel with beta = 0 in which a few
    rows of every group (the first, one in the middle, the last rows) get x = mean (and residual 0): pre-activation value
    exactly 0.  -> dict; 'planted' = [M, C] bool."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(M, C, generator=g, device=dev) * 2 + 3
    r = torch.randn(M, C, generator=g, device=dev) if res else None
    dy = torch.randn(M, C, generator=g, device=dev)
    gam = torch.rand(C, generator=g, device=dev) + 0.5
    bet = torch.randn(C, generator=g, device=dev)
    if gamma_zero:
        gam[5] = 0.
    bet[2] = 0.
    Mg = M // G
    xg = x.view(G, Mg, C)
    mean = torch.stack([xg[k].double().mean(0) for k in range(G)]).float()
    var = torch.stack([xg[k].double().var(0, unbiased=False) for k in range(G)]).float()
    rows = torch.tensor([0, 1, Mg // 2, Mg - 2, Mg - 1], device=dev)
    planted = torch.zeros(M, C, dtype=torch.bool, device=dev)
    for k in range(G):
        xg[k][rows, 2] = mean[k, 2]
        if res:
            r.view(G, Mg, C)[k][rows, 2] = 0.
        planted.view(G, Mg, C)[k][rows, 2] = True
    return dict(M=M, C=C, G=G, Mg=Mg, act=act, x=x, r=r, dy=dy, gam=gam, bet=bet, mean=mean, var=var, planted=planted)


def ref_rows(c, rows):
    """float64 forward of the rows `rows` (a LongTensor; all groups mixed) -> z (pre-activation), y."""
    grp = rows // c['Mg']
    m, v = c['mean'].double()[grp], c['var'].double()[grp]
    z = (c['x'][rows].double() - m) / torch.sqrt(v + EPS) * c['gam'].double() + c['bet'].double()
    if c['r'] is not None:
        z = z + c['r'][rows].double()
    y = z if c['act'] == 0 else (z.clamp(min=0) if c['act'] == 1 else torch.where(z > 0, z, 0.01 * z))
    return z, y


def dz_f64(c, z, dy):
    neg = 0. if c['act'] == 1 else 0.01
    return dy.double() if c['act'] == 0 else dy.double() * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, neg))


def sums_f64(c, chunk=65536):
    """[G][2][C]: sum dz | sum dz xhat of each group, float64, over ALL rows (in chunks: the large case stays on the device)."""
    out = torch.zeros(c['G'], 2, c['C'], dtype=torch.float64, device=c['x'].device)
    for k in range(c['G']):
        for r0 in range(k * c['Mg'], (k + 1) * c['Mg'], chunk):
            rows = torch.arange(r0, min(r0 + chunk, (k + 1) * c['Mg']), device=c['x'].device)
            z, _ = ref_rows(c, rows)
            dz = dz_f64(c, z, c['dy'][rows])
            xh = (c['x'][rows].double() - c['mean'].double()[k]) / torch.sqrt(c['var'].double()[k] + EPS)
            out[k, 0] += dz.sum(0)
            out[k, 1] += (dz * xh).sum(0)
    return out


def doubtful(z, planted):
    """Elements whose sign float64 does not settle for fp32; at most 1 % of a case."""
    d = (z.abs() <= 1e-6) & ~planted
    assert int(d.sum()) <= 0.01 * d.numel(), '%d of %d pre-activation values within 1e-6 of 0' % (int(d.sum()), d.numel())
    return d


def amax_of(slot):
    return slot.max()


def run_fwd(c, want_mask, tune):
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items()}
    y = torch.empty_like(d['x'])
    mask = torch.full((c['M'] * c['C'] // 4,), 0xff, dtype=torch.uint8, device='cuda') if want_mask else None
    slot = torch.zeros(SLOT, device='cuda')
    _lib.query('xas_set_tuning', tune)
    _lib.call('xas_bn_apply_amax', _lib.ptr(d['x']), _lib.ptr(d['mean']), _lib.ptr(d['var']), _lib.ptr(d['gam']), _lib.ptr(d['bet']),
              _lib.ptr(d['r']), EPS, c['act'], c['M'], c['C'], c['G'], _lib.ptr(y), _lib.ptr(mask), _lib.ptr(slot))
    torch.cuda.synchronize()
    _lib.query('xas_set_tuning', 0)
    return y, mask, slot


def check_fwd(c, want_mask, rows):
    """Both policies against float64 on `rows`, and against each other on everything."""
    outs = [run_fwd(c, want_mask, tune) for _, tune in POLICIES]
    z, yr = ref_rows(c, rows)
    planted = c['planted'][rows]
    assert bool(((z > 0).any(0) & (z < 0).any(0)).view(-1, 4).any(1).all()), 'a channel quadruple sees one sign only'
    assert bool((z[planted] == 0).all()) and int(planted.sum()) > 0
    skip = doubtful(z, planted)
    for (name, _), (y, mask, slot) in zip(POLICIES, outs):
        ys = y[rows.cuda()].to(z.device)
        err = float((ys.double() - yr).abs().max())
        print('%s: y max-abs error %.3e, %d doubtful signs' % (name, err, int(skip.sum())))
        assert err < 2e-5, name
        assert bool((ys[planted] == 0).all()), name
        if want_mask:
            got = mask.view(c['M'], c['C'] // 4)[rows.cuda()].reshape(-1).to(z.device)
            keep = pack_signs(~skip)                       # bits that are compared
            assert torch.equal(got & keep, pack_signs((z > 0) & ~skip)), name
            assert bool((got & pack_signs(planted) == 0).all()), name
        assert float(amax_of(slot)) == float(y.abs().max()), name
    (y0, m0, s0), (y1, m1, s1) = outs
    assert torch.equal(bits(y0), bits(y1)) and float(amax_of(s0)) == float(amax_of(s1))
    if want_mask:
        assert torch.equal(m0, m1)


# backward operand sets: which of x / y / mask the launch reads, whether it writes dres
def run_bwd(c, y, mask, sums, use, tune):
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items()}
    dx = torch.empty_like(d['x'])
    dres = torch.empty_like(d['x']) if 'dres' in use else None
    slot = torch.zeros(SLOT, device='cuda')
    need_beta = 'x' not in use or (c['act'] != 0 and 'y' not in use and 'mask' not in use)
    xd, yd, md = d['x'] if 'x' in use else None, y.cuda() if 'y' in use else None, mask.cuda() if 'mask' in use else None
    sd, bd = sums.cuda(), d['bet'] if need_beta else None          # (named: alive until the launch has run)
    _lib.query('xas_set_tuning', tune)
    _lib.call('xas_bn_bwd_apply_amax', _lib.ptr(xd), _lib.ptr(yd), _lib.ptr(d['dy']), _lib.ptr(d['mean']), _lib.ptr(d['var']),
              _lib.ptr(d['gam']), _lib.ptr(bd), _lib.ptr(sd), EPS, c['act'], c['M'], c['C'], c['G'], float(c['Mg']), _lib.ptr(dx),
              _lib.ptr(dres), _lib.ptr(md), _lib.ptr(slot))
    torch.cuda.synchronize()
    _lib.query('xas_set_tuning', 0)
    return dx, dres, slot


def bwd_operands(c, use):
    """What the launch is handed besides the case: y and the mask bytes of the float64 forward (rounded to fp32 / its signs,
    whichever `use` names) and the float64 sums."""
    step = 65536
    y = torch.empty_like(c['x']) if 'y' in use else None
    mask = torch.empty(c['M'] * c['C'] // 4, dtype=torch.uint8, device=c['x'].device) if 'mask' in use else None
    for r0 in range(0, c['M'], step):
        rr = torch.arange(r0, min(r0 + step, c['M']), device=c['x'].device)
        z, yr = ref_rows(c, rr)
        if y is not None:
            y[rr] = yr.float()
        if mask is not None:
            mask.view(c['M'], -1)[rr] = pack_signs(z > 0).view(len(rr), -1)
    return y, mask, sums_f64(c)


def check_bwd(c, use, rows):
    """Both policies against float64 on `rows`; dres against each other on everything."""
    use = set(use.split())
    y, mask, sums = bwd_operands(c, use)
    outs = [run_bwd(c, y, mask, sums.float(), use, tune) for _, tune in POLICIES]
    z, _ = ref_rows(c, rows)
    planted = c['planted'][rows]
    assert bool(((z > 0).any(0) & (z < 0).any(0)).view(-1, 4).any(1).all()), 'a channel quadruple sees one sign only'
    assert bool((z[planted] == 0).all()) and int(planted.sum()) > 0
    skip = doubtful(z, planted) if c['act'] != 0 else torch.zeros_like(planted)
    dz = dz_f64(c, z, c['dy'][rows])
    grp = rows // c['Mg']
    istd = 1. / torch.sqrt(c['var'].double()[grp] + EPS)
    xh = (c['x'][rows].double() - c['mean'].double()[grp]) * istd
    dxr = c['gam'].double() * istd * (dz - sums[grp, 0] / c['Mg'] - xh * sums[grp, 1] / c['Mg'])
    keep = (~skip).double()
    for (name, _), (dx, dres, slot) in zip(POLICIES, outs):
        e_dx = rel(dx[rows.cuda()].to(z.device) * keep, dxr * keep)
        print('%s: dx relative error %.3e, %d doubtful signs' % (name, e_dx, int(skip.sum())))
        assert e_dx < 2e-5, name
        if dres is not None:
            ds = dres[rows.cuda()].to(z.device)
            e_dr = rel(ds * keep, dz * keep)
            print('%s: dres relative error %.3e' % (name, e_dr))
            assert e_dr < 1e-6, name
            if c['act'] == 1:
                assert bool((ds[planted] == 0).all()), name             # exact zero: "not > 0"
        assert float(amax_of(slot)) == float(dx.abs().max()), name
    (dx0, dr0, _), (dx1, dr1, _) = outs
    if dr0 is not None:
        assert torch.equal(bits(dr0), bits(dr1))
    if c['gam'].eq(0).any():                                             # xhat from y with gamma = 0: xhat := 0, dx = 0
        for dx, _, _ in outs:
            assert bool((dx[:, c['gam'].eq(0).nonzero().flatten().cuda()] == 0).all())


def all_rows(c):
    return torch.arange(c['M'], device=c['x'].device)


@pytest.mark.parametrize('res', ['plain', 'res', 'res_mask'])
@pytest.mark.parametrize('act', [0, 1, 2])
def test_bn_apply_modes(act, res):
    """The nine forward modes: C = 64 (C/4 = 16), 2 groups of 150 rows (10 blocks per group, the last one partial)."""
    c = make_case(300, 64, 2, act, res != 'plain', seed=10 * act + len(res))
    check_fwd(c, res == 'res_mask', all_rows(c))


@pytest.mark.parametrize('M,C,G,act,res', [(300, 24, 2, 1, 'res_mask'), (300, 24, 2, 2, 'plain'), (3 * 1366, 2048, 3, 1, 'res_mask')],
                         ids=['C24_relu_res_mask', 'C24_leaky', 'C2048_grid_rounding'])
def test_bn_apply_channel_counts(M, C, G, act, res):
    """C/4 = 6 is no power of two: general policy on both settings.  C/4 = 512 > 256: the streaming grid is rounded up to
    whole multiples of C/4 threads (module docstring: which row count makes the rounding act)."""
    c = make_case(M, C, G, act, res != 'plain', seed=C + act, dev='cuda' if C == 2048 else 'cpu')
    check_fwd(c, res == 'res_mask', all_rows(c))


BWD_MODES = [
    # id, act, operands, gamma_zero
    ('0_none_x', 0, 'x', False),
    ('1_relu_sign_from_x', 1, 'x', False),
    ('2_leaky_xhat_from_y', 2, 'y', True),
    ('3_relu_y_dres', 1, 'x y dres', False),
    ('4_relu_y', 1, 'x y', False),
    ('5_relu_mask_dres', 1, 'x mask dres', False),
    ('6_relu_mask', 1, 'x mask', False),
    ('general_none_dres', 0, 'x dres', False),
    ('general_leaky_x_y', 2, 'x y', False),
    ('general_leaky_x_y_dres', 2, 'x y dres', False),
]


@pytest.mark.parametrize('name,act,use,gz', BWD_MODES, ids=[m[0] for m in BWD_MODES])
def test_bn_bwd_apply_modes(name, act, use, gz):
    """The seven streaming modes of the backward and three that only the general policy accepts; C = 64, 2 groups of 150 rows.
    A layer that hands on a residual gradient had a residual in its forward."""
    c = make_case(300, 64, 2, act, 'dres' in use, seed=100 + len(name) + act, gamma_zero=gz)
    check_bwd(c, use, all_rows(c))


@pytest.mark.parametrize('act,use,gz', [(1, 'x y dres', False), (2, 'y', True)], ids=['C24_relu_y_dres', 'C24_leaky_xhat_from_y'])
def test_bn_bwd_apply_c24(act, use, gz):
    c = make_case(300, 24, 2, act, 'dres' in use, seed=24 + act, gamma_zero=gz)
    check_bwd(c, use, all_rows(c))


# 525 288 rows x 64 channels, one group: n4g = 8 404 608 = 4 x (8192 x 256) + 16 000 - every thread of the capped grid makes
# one unrolled trip, the first 16 000 threads a tail trip (the last 1000 rows)
LARGE_M = 525288


def large_rows(c):
    M = c['M']
    q = 8192 * 256 // 16           # rows of one unrolled lane: samples from each of the four lanes, then the tail
    return torch.cat([torch.arange(0, 1000), torch.arange(q + q // 2, q + q // 2 + 1000), torch.arange(M // 2, M // 2 + 1000),
                      torch.arange(M - 2000, M)]).to(c['x'].device)


def test_bn_apply_large():
    """ReLU + residual + sign bytes where both the unrolled loop and the tail run; float64 on rows of every unrolled lane (head, 3/8, middle) and the
    last 2000 rows (the pass is element-wise given the statistics)."""
    c = make_case(LARGE_M, 64, 1, 1, True, seed=7, dev='cuda')
    check_fwd(c, True, large_rows(c))


def test_bn_bwd_apply_large():
    """Mode 3 (ReLU, x and y, residual gradient) at the same size."""
    c = make_case(LARGE_M, 64, 1, 1, True, seed=8, dev='cuda')
    check_bwd(c, 'x y dres', large_rows(c))
