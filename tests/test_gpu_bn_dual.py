"""The dual batch-norm passes of a block output with a projection, out = relu(bn3(x) + bn_d(xd)) (xas_bn_apply_dual_amax,
xas_bn_bwd_reduce_dual, xas_bn_bwd_apply_dual_amax; ops_nn._Bottleneck with XAS_DS_FUSE).

1. The three entry points ALONE against a float64 restatement written here (two norms, add, ReLU, and their backward), on
   both loop policies.  Bars: those of the single-norm forms of the same arithmetic - test_gpu_bn_apply (y max-abs < 2e-5,
   dx relative < 2e-5, sign decisions those of float64 outside |z| <= 1e-6) and test_gpu_col_reduce (every sum within
   128 * 2^-24 * sum |term64|; a thread adds at most 64 rows one after the other, asserted from the geometry rule).
   Inputs: beta + beta_d spread around 0 puts about half of the pre-activation values below zero (asserted: 35-65 %);
   channel 2 has beta = beta_d = 0 and rows with x = mean, xd = mean_d: exact zeros at the ReLU boundary.
   Shapes: C = 8 (streaming policy, two channel quadruples), 12 (C/4 = 3: general policy), 64; 15 rows per group (under one
   unrolled trip of the reduction: its tail only) and 1031 (unrolled trips plus a tail); 1 and 3 groups.  The streaming
   apply kernels unroll only once the block cap binds: one case at 525 288 x 64 (the size test_gpu_bn_apply uses for it).
2. One projection bottleneck 8 -> 4 -> 16, stride 2, 6 images of 6 x 10 in 3 camera groups, plain and under a prefix pass with
   one prefix group: the fused path EQUALS the separate passes (torch.equal) in the block output, the input gradient, every
   parameter gradient, the four running-statistic buffers and the two published gradient maxima.
3. The same block on two gloo ranks: fused equals unfused, and the backward sends ONE collective for the block's two norms."""

import pytest
import torch

from xas_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS, EPS_D = 1e-5, 2e-5
SLOT = 1024
POLICIES = (('shipped', 0), ('general', _lib.TUNE_GENERAL_KERNELS))
DEV = 'cuda'


@pytest.fixture(autouse=True)
def _tuning_back(request):
    request.addfinalizer(lambda: _lib.query('xas_set_tuning', 0))


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def pack_signs(pos):
    p = pos.reshape(pos.shape[0], -1, 4).to(torch.uint8)
    return (p[..., 0] | (p[..., 1] << 1) | (p[..., 2] << 2) | (p[..., 3] << 3)).reshape(-1)


def grp_sum(t, G):
    return t.view(G, -1, t.shape[-1]).sum(1)


def rows_per_thread(M, C, G):
    """col_geom of csrc/bn.hip under the shipped flags -> rows a thread adds one after the other, at most."""
    cdiv = lambda a, b: -(-a // b)
    cb = 4
    while cb < 64 and C % (cb * 2) == 0:
        cb *= 2
    ty, ncb, Mg = 256 // (cb // 4), C // cb, M // G
    want = max(1, min(256 * (2 if G > 1 else 1) // (ncb * G), cdiv(Mg, ty * 8)))
    return cdiv(cdiv(Mg, want), ty)


# ------------------------------------------------------------------------------------------------ float64 restatement
def make_case(Mg, C, G, seed):
    """fp32 inputs on the device and everything float64 says about them."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    M = Mg * G
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    x, xd, dy = rn(M, C) * 2 + 3, rn(M, C) * 1.5 - 1, rn(M, C)
    gam, gam_d = torch.rand(C, generator=g, device=DEV) + 0.5, torch.rand(C, generator=g, device=DEV) + 0.5
    bet, bet_d = rn(C) * 0.3, rn(C) * 0.3
    bet[2] = 0.
    bet_d[2] = 0.
    stat = lambda t: (t.view(G, Mg, C).double().mean(1).float(), t.view(G, Mg, C).double().var(1, unbiased=False).float())
    (mean, var), (mean_d, var_d) = stat(x), stat(xd)
    rows = torch.tensor(sorted({0, 1, Mg // 2, Mg - 2, Mg - 1}), device=DEV)
    planted = torch.zeros(M, C, dtype=torch.bool, device=DEV)
    for k in range(G):
        x.view(G, Mg, C)[k][rows, 2] = mean[k, 2]
        xd.view(G, Mg, C)[k][rows, 2] = mean_d[k, 2]
        planted.view(G, Mg, C)[k][rows, 2] = True
    c = dict(M=M, Mg=Mg, C=C, G=G, x=x, xd=xd, dy=dy, gam=gam, gam_d=gam_d, bet=bet, bet_d=bet_d, mean=mean, var=var,
             mean_d=mean_d, var_d=var_d, planted=planted)
    return c


def ref(c, rows=None, want_planted=True):
    """float64: xhat / xhat_d, z (pre-activation), y, dz for the rows `rows` (all rows: None)."""
    rows = torch.arange(c['M'], device=DEV) if rows is None else rows
    grp = rows // c['Mg']
    istd, istd_d = 1 / torch.sqrt(c['var'].double()[grp] + EPS), 1 / torch.sqrt(c['var_d'].double()[grp] + EPS_D)
    xh = (c['x'][rows].double() - c['mean'].double()[grp]) * istd
    xh_d = (c['xd'][rows].double() - c['mean_d'].double()[grp]) * istd_d
    z = (xh * c['gam'].double() + c['bet'].double()) + (xh_d * c['gam_d'].double() + c['bet_d'].double())
    planted = c['planted'][rows]
    assert bool((z[planted] == 0).all()) and (int(planted.sum()) > 0 or not want_planted)
    doubt = (z.abs() <= 1e-6) & ~planted
    assert int(doubt.sum()) <= 0.01 * doubt.numel()
    dz = c['dy'][rows].double() * (z > 0) * ~doubt                 # doubtful signs carry no gradient (dy is zeroed there)
    return dict(rows=rows, grp=grp, istd=istd, istd_d=istd_d, xh=xh, xh_d=xh_d, z=z, y=z.clamp(min=0), dz=dz, doubt=doubt,
                planted=planted)


def run_fwd(c, tune):
    y = torch.empty_like(c['x'])
    mask = torch.full((c['M'] * c['C'] // 4,), 0xff, dtype=torch.uint8, device=DEV)
    slot = torch.zeros(SLOT, device=DEV)
    p = _lib.ptr
    _lib.query('xas_set_tuning', tune)
    _lib.call('xas_bn_apply_dual_amax', p(c['x']), p(c['mean']), p(c['var']), p(c['gam']), p(c['bet']), EPS, p(c['xd']),
              p(c['mean_d']), p(c['var_d']), p(c['gam_d']), p(c['bet_d']), EPS_D, c['M'], c['C'], c['G'], p(y), p(mask), p(slot))
    torch.cuda.synchronize()
    _lib.query('xas_set_tuning', 0)
    return y, mask, slot


def run_reduce(c, dy, mask, tune, acc=False):
    M, C, G = c['M'], c['C'], c['G']
    sums = torch.full((2, G, 2, C), 1.5e30, device=DEV)
    p = _lib.ptr
    _lib.query('xas_set_tuning', tune)
    ws = torch.empty(2 * _lib.query('xas_bn_workspace_floats', M, C, G), device=DEV)
    accs = [torch.full((C,), float(i + 1), device=DEV) for i in range(4)] if acc else [None] * 4
    _lib.call('xas_bn_bwd_reduce_dual', p(c['x']), p(c['xd']), p(dy), p(mask), p(c['mean']), p(c['var']), EPS, p(c['mean_d']),
              p(c['var_d']), EPS_D, M, C, G, p(sums[0]), p(sums[1]), p(ws), *[p(a) for a in accs])
    torch.cuda.synchronize()
    _lib.query('xas_set_tuning', 0)
    return sums, accs


def run_bwd(c, dy, mask, sums, tune):
    dx, dxd = torch.empty_like(c['x']), torch.empty_like(c['x'])
    slot, slot_d = torch.zeros(SLOT, device=DEV), torch.zeros(SLOT, device=DEV)
    p = _lib.ptr
    _lib.query('xas_set_tuning', tune)
    _lib.call('xas_bn_bwd_apply_dual_amax', p(c['x']), p(c['xd']), p(dy), p(mask), p(c['mean']), p(c['var']), p(c['gam']),
              p(sums[0]), EPS, p(c['mean_d']), p(c['var_d']), p(c['gam_d']), p(sums[1]), EPS_D, c['M'], c['C'], c['G'],
              float(c['Mg']), float(c['Mg']), p(dx), p(dxd), p(slot), p(slot_d))
    torch.cuda.synchronize()
    _lib.query('xas_set_tuning', 0)
    return dx, dxd, slot, slot_d


def check_fwd(c, r):
    rows = r['rows']
    neg = float((r['z'] < 0).double().mean())
    print('pre-activation values below zero: %.1f %%' % (100 * neg))
    assert 0.35 < neg < 0.65
    outs = [run_fwd(c, tune) for _, tune in POLICIES]
    for (name, _), (y, mask, slot) in zip(POLICIES, outs):
        err = float((y[rows].double() - r['y']).abs().max())
        print('%s: y max-abs error %.3e, %d doubtful signs' % (name, err, int(r['doubt'].sum())))
        assert err < 2e-5, name
        assert bool((y[rows][r['planted']] == 0).all()), name
        got = mask.view(c['M'], c['C'] // 4)[rows].reshape(-1)
        keep = pack_signs(~r['doubt'])
        assert torch.equal(got & keep, pack_signs((r['z'] > 0) & ~r['doubt'])), name
        assert bool((got & pack_signs(r['planted']) == 0).all()), name
        assert float(slot.max()) == float(y.abs().max()), name
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1], outs[1][1])


def check_bwd_apply(c, r, dy, mask, sums64):
    rows, grp, Mg = r['rows'], r['grp'], c['Mg']
    s3, sd = sums64
    dx_r = c['gam'].double() * r['istd'] * (r['dz'] - s3[grp, 0] / Mg - r['xh'] * s3[grp, 1] / Mg)
    dxd_r = c['gam_d'].double() * r['istd_d'] * (r['dz'] - sd[grp, 0] / Mg - r['xh_d'] * sd[grp, 1] / Mg)
    sums = torch.stack([s3, sd]).float().contiguous()
    outs = [run_bwd(c, dy, mask, sums, tune) for _, tune in POLICIES]
    for (name, _), (dx, dxd, slot, slot_d) in zip(POLICIES, outs):
        e, e_d = rel(dx[rows], dx_r), rel(dxd[rows], dxd_r)
        print('%s: dx relative error %.3e, dxd %.3e' % (name, e, e_d))
        assert e < 2e-5 and e_d < 2e-5, name
        assert float(slot.max()) == float(dx.abs().max()) and float(slot_d.max()) == float(dxd.abs().max()), name


@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('Mg', [15, 1031])
@pytest.mark.parametrize('C', [8, 12, 64])
def test_dual_kernels_vs_float64(C, Mg, G):
    c = make_case(Mg, C, G, seed=1000 * C + Mg + G)
    r = ref(c)
    check_fwd(c, r)
    # backward operands as float64 decides them: the sign bytes, dy zeroed where the sign is in doubt
    mask = pack_signs(r['z'] > 0)
    dy = torch.where(r['doubt'], torch.zeros_like(c['dy']), c['dy'])
    assert rows_per_thread(c['M'], C, G) <= 64
    terms = {'sum_dz': r['dz'], 'sum_dz_xhat': r['dz'] * r['xh'], 'sum_dz_xhat_d': r['dz'] * r['xh_d']}
    want = {k: grp_sum(t, G) for k, t in terms.items()}
    bar = {k: 128 * U * grp_sum(t.abs(), G) for k, t in terms.items()}
    first = None
    for name, tune in POLICIES + (('lean', _lib.TUNE_COL_REDUCE_LEAN),):
        sums, _ = run_reduce(c, dy, mask, tune)
        got = {'sum_dz': sums[0, :, 0], 'sum_dz_xhat': sums[0, :, 1], 'sum_dz_xhat_d': sums[1, :, 1]}
        for k in got:
            err = (got[k].double() - want[k]).abs()
            print('%s %s: error / bar %.4f' % (name, k, float((err / bar[k].clamp(min=1e-300)).max())))
            assert bool((err <= bar[k]).all()), (name, k)
        assert torch.equal(sums[0, :, 0].view(torch.int32), sums[1, :, 0].view(torch.int32)), name      # the one sum dz, twice
        if name != 'lean':
            first = sums if first is None else first
            assert torch.equal(sums.view(torch.int32), first.view(torch.int32)), name                  # (the policy flag is not the reduction's)
    # the parameter-gradient accumulators: += the sums over the groups, each pair its own norm's
    sums, accs = run_reduce(c, dy, mask, 0, acc=True)
    for i, (n, col) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        exp = sums[n, :, col].double().sum(0) + (i + 1)
        assert bool(((accs[i].double() - exp).abs() <= 4 * U * (exp.abs() + sums[n, :, col].double().abs().sum(0))).all()), i
    check_bwd_apply(c, r, dy, mask, (torch.stack([want['sum_dz'], want['sum_dz_xhat']], 1),
                                     torch.stack([want['sum_dz'], want['sum_dz_xhat_d']], 1)))


def test_dual_apply_kernels_large():
    """525 288 rows x 64 channels, one group: every thread of the capped streaming grid makes one unrolled trip, the first
    16 000 a tail trip.  float64 on rows of every unrolled lane and on the last 2000 rows (element-wise given the sums)."""
    M = 525288
    c = make_case(M, 64, 1, seed=5)
    q = 8192 * 256 // 16
    rows = torch.cat([torch.arange(0, 1000), torch.arange(q + q // 2, q + q // 2 + 1000), torch.arange(M // 2, M // 2 + 1000),
                      torch.arange(M - 2000, M)]).to(DEV)
    r = ref(c, rows)
    check_fwd(c, r)
    # signs and sums over ALL rows, in chunks
    mask = torch.empty(M * 16, dtype=torch.uint8, device=DEV)
    dy = c['dy'].clone()
    s = torch.zeros(3, 1, 64, dtype=torch.float64, device=DEV)
    for r0 in range(0, M, 65536):
        rr = torch.arange(r0, min(r0 + 65536, M), device=DEV)
        part = ref(c, rr, want_planted=False)
        mask.view(M, 16)[rr] = pack_signs(part['z'] > 0).view(len(rr), 16)
        dy[rr] = torch.where(part['doubt'], torch.zeros_like(dy[rr]), dy[rr])
        s[0] += part['dz'].sum(0)
        s[1] += (part['dz'] * part['xh']).sum(0)
        s[2] += (part['dz'] * part['xh_d']).sum(0)
    r = ref(c, rows)
    check_bwd_apply(c, r, dy, mask, (torch.stack([s[0], s[1]], 1), torch.stack([s[0], s[2]], 1)))


@pytest.mark.parametrize('Mg,C,G', [(1031, 64, 3), (525288, 64, 1), (300, 12, 2)], ids=['tail_loops', 'unrolled_loops', 'general'])
def test_dual_kernels_equal_the_single_norm_kernels(Mg, C, G):
    """The claim of xas_hip.h, kernel by kernel and without a tolerance: the dual passes write the bits of the single-norm
    launches they replace (apply act 0 -> apply ReLU + residual + sign bytes; reduce + apply with dres -> reduce + apply
    act 0 on that dres), also where the streaming kernels run their unrolled loops.  The general policy (C/4 = 3) keeps that
    for the forward and the sums; its backward apply is compiled with other fused multiply-adds than the single-norm general
    kernel (as the two policies of the single-norm kernel differ from each other): there the gradients agree to 1e-6
    relative, the bar test_gpu_bn_apply sets for a stored dz."""
    c = make_case(Mg, C, G, seed=77 + C)
    M, p = c['M'], _lib.ptr
    bits = lambda t: t.contiguous().view(torch.int32)
    new = lambda: torch.empty_like(c['x'])
    # forward
    skip, y1, m1, s1 = new(), new(), torch.empty(M * C // 4, dtype=torch.uint8, device=DEV), torch.zeros(SLOT, device=DEV)
    _lib.call('xas_bn_apply_amax', p(c['xd']), p(c['mean_d']), p(c['var_d']), p(c['gam_d']), p(c['bet_d']), None, EPS_D, 0, M, C, G,
              p(skip), None, None)
    _lib.call('xas_bn_apply_amax', p(c['x']), p(c['mean']), p(c['var']), p(c['gam']), p(c['bet']), p(skip), EPS, 1, M, C, G, p(y1),
              p(m1), p(s1))
    y2, m2, s2 = run_fwd(c, 0)
    assert torch.equal(bits(y1), bits(y2)) and torch.equal(m1, m2) and float(s1.max()) == float(s2.max())
    # backward sums
    dy = c['dy']
    ws = torch.empty(_lib.query('xas_bn_workspace_floats', M, C, G), device=DEV)
    sa, sb, dres, dx1, gd1 = torch.empty(G, 2, C, device=DEV), torch.empty(G, 2, C, device=DEV), new(), new(), new()
    t1, t2 = torch.zeros(SLOT, device=DEV), torch.zeros(SLOT, device=DEV)
    _lib.call('xas_bn_bwd_reduce', p(c['x']), None, p(dy), p(c['mean']), p(c['var']), p(c['gam']), p(c['bet']), EPS, 1, M, C, G, p(sa),
              p(ws), None, None, p(m1))
    _lib.call('xas_bn_bwd_apply_amax', p(c['x']), None, p(dy), p(c['mean']), p(c['var']), p(c['gam']), p(c['bet']), p(sa), EPS, 1, M, C,
              G, float(Mg), p(dx1), p(dres), p(m1), p(t1))
    _lib.call('xas_bn_bwd_reduce', p(c['xd']), None, p(dres), p(c['mean_d']), p(c['var_d']), p(c['gam_d']), p(c['bet_d']), EPS_D, 0, M,
              C, G, p(sb), p(ws), None, None, None)
    _lib.call('xas_bn_bwd_apply_amax', p(c['xd']), None, p(dres), p(c['mean_d']), p(c['var_d']), p(c['gam_d']), p(c['bet_d']), p(sb),
              EPS_D, 0, M, C, G, float(2 * Mg), p(gd1), None, None, p(t2))
    torch.cuda.synchronize()
    sums, _ = run_reduce(c, dy, m1, 0)
    assert torch.equal(bits(sums[0]), bits(sa)) and torch.equal(bits(sums[1]), bits(sb))
    # backward apply (the projection norm with a count of its own: a SyncBatchNorm beside a rank-local bn3)
    dx2, gd2 = new(), new()
    u1, u2 = torch.zeros(SLOT, device=DEV), torch.zeros(SLOT, device=DEV)
    _lib.call('xas_bn_bwd_apply_dual_amax', p(c['x']), p(c['xd']), p(dy), p(m1), p(c['mean']), p(c['var']), p(c['gam']), p(sums[0]),
              EPS, p(c['mean_d']), p(c['var_d']), p(c['gam_d']), p(sums[1]), EPS_D, M, C, G, float(Mg), float(2 * Mg), p(dx2), p(gd2),
              p(u1), p(u2))
    torch.cuda.synchronize()
    if C % 16 == 0:
        assert torch.equal(bits(dx1), bits(dx2)) and torch.equal(bits(gd1), bits(gd2))
        assert float(t1.max()) == float(u1.max()) and float(t2.max()) == float(u2.max())
    else:
        assert rel(dx2, dx1) < 1e-6 and rel(gd2, gd1) < 1e-6
        assert float(u1.max()) == float(dx2.abs().max()) and float(u2.max()) == float(gd2.abs().max())


# ------------------------------------------------------------------------------------------------ the block, fused vs separate
def _block(sync3=False):
    from modules.integral_base_modules.resnet import Bottleneck
    from xas_amd import layers as L
    from xas_amd.ops_nn import ACT_NONE
    torch.manual_seed(3)
    proj = torch.nn.Sequential(L.Conv2d(8, 16, 1, stride=2, bias=False, init='kaiming_fan_out'),
                               L.BatchNorm2d(16, act=ACT_NONE, sync=True))
    blk = Bottleneck(8, 4, 2, proj)
    blk.bn3.sync = sync3
    with torch.no_grad():                                  # norms away from their initial (1, 0)
        for bn in (blk.bn1, blk.bn2, blk.bn3, proj[1]):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.3)
    return blk.cuda().train()


def _run_block(fuse, prefix, sync3=False, seed=11):
    """One forward + backward of the block -> dict of everything compared (clones)."""
    from xas_amd import ops_nn as F
    blk = _block(sync3)
    for p in blk.parameters():
        p.grad = torch.zeros_like(p)                       # the norms add their gradients in place where a .grad exists
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = 6 + (2 if prefix else 0)
    buf = F.to_cl(torch.randn(n, 8, 6, 10, generator=g, device=DEV))
    dout = F.to_cl(torch.randn(6, 16, 3, 5, generator=g, device=DEV))
    tags, recording = [], [False]
    orig_tag, was = F.tag_grad_amax, F.FUSE_DS

    def tag(t, slot):
        if recording[0] and t.dim() == 4 and t.shape[1] == 16:
            tags.append(slot)
        return orig_tag(t, slot)

    F.tag_grad_amax, F.FUSE_DS = tag, bool(fuse)
    try:
        F.reset_grad_amax()
        if prefix:
            F.mark_prefix_buffer(buf)
            with F.bn_groups(4, 1, 2):
                x = buf[2:].detach().requires_grad_(True)
                out = blk(x)
        else:
            with F.bn_groups(3):
                x = buf.detach().requires_grad_(True)
                out = blk(x)
        recording[0] = True
        out.backward(dout)
        recording[0] = False
        torch.cuda.synchronize()
    finally:
        F.tag_grad_amax, F.FUSE_DS = orig_tag, was
    assert len(tags) == 2 or not F.f16x3_on(), tags        # dx of bn3, then the projection norm's
    res = {'out': out.detach().clone(), 'dx': x.grad.clone(), 'amax': [float(s.max()) for s in tags]}
    for k, p in blk.named_parameters():
        res['grad.' + k] = p.grad.clone()
    for k in ('bn3.running_mean', 'bn3.running_var', 'downsample.1.running_mean', 'downsample.1.running_var'):
        res[k] = blk.state_dict()[k].clone()
    return res


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == 'amax':
            assert a[k] == b[k] and (len(a[k]) == 0 or min(a[k]) > 0), (k, a[k], b[k])
        else:
            assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize('prefix', [False, True], ids=['plain', 'prefix_pass'])
def test_block_fused_equals_separate(prefix):
    calls = []
    orig = _lib.call
    from xas_amd import ops_nn as F
    F.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        fused = _run_block(True, prefix)
        n_fused = list(calls)
        del calls[:]
        plain = _run_block(False, prefix)
    finally:
        F.call = orig
    assert {'xas_bn_apply_dual_amax', 'xas_bn_bwd_reduce_dual', 'xas_bn_bwd_apply_dual_amax'} <= set(n_fused)
    assert not any('dual' in c for c in calls)
    assert float(fused['out'].abs().max()) > 0 and float(fused['dx'].abs().max()) > 0
    _assert_same(fused, plain)


# ------------------------------------------------------------------------------------------------ two ranks
def _rank_case(rank, world, sync3):
    import torch.distributed as dist
    from _ranks import init_group
    torch.cuda.set_device(0)
    init_group('gloo', rank, world)
    from xas_amd import dp
    res = {}
    for fuse in (True, False):
        dp.comm_stats = {'syncbn_calls': 0, 'syncbn_bytes': 0, 'syncbn_host_ms': 0.0}
        orig = dist.all_reduce
        n = [0]

        def counted(*a, **k):
            n[0] += 1
            return orig(*a, **k)

        dist.all_reduce = counted
        try:
            r = _run_block(fuse, False, sync3, seed=11 + rank)      # identical replicas, different data
        finally:
            dist.all_reduce = orig
            dp.comm_stats = None
        res[fuse] = ({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in r.items()}, n[0])
    dist.destroy_process_group()
    return res


@pytest.mark.multiproc
@pytest.mark.parametrize('sync3', [False, True], ids=['bn3_local', 'bn3_sync'])
def test_block_two_ranks(sync3):
    """bn3_local: the detector's blocks (rank-local bn3, SyncBatchNorm projection norm); bn3_sync: both norms exchange their
    sums - in ONE message where the separate passes send two."""
    from _ranks import run_ranks
    ret = run_ranks(_rank_case, 2, (sync3,))
    for rank in (0, 1):
        (fused, n_fused), (plain, n_plain) = ret[rank][True], ret[rank][False]
        assert n_fused == 1 and n_plain == (2 if sync3 else 1), (n_fused, n_plain)
        _assert_same(fused, plain)
    for k in ('downsample.1.running_mean', 'downsample.1.running_var'):
        assert torch.equal(ret[0][True][0][k], ret[1][True][0][k])
