"""The discriminator and joint-loss kernels of csrc/gcn.hip and csrc/losses.hip alone, through the C ABI, against plain float64 torch on the CPU
computed from the same fp32 inputs: graph_aggregate, the six gln_* kernels (graph LayerNorm + ReLU + residual, both ways),
pose_loss_fwd/bwd (kinds 0, 1, 2) and lsgan_fwd/bwd - at the shapes where each guard, stride loop and grid cap is taken, with
every output buffer filled with NaN before the launch.

Bars.  For every compared quantity the same expression was run in fp32 on the CPU (ATen) against the float64 reference over
all cases of this file (`python tests/test_gpu_gcn_loss_kernels.py` prints the middle column); the bar is 4x the worst such
distance (the kernels sum in another order, over a deeper tree), but never looser than what the suite already asks of the
same kind of quantity: 3e-6 for element-wise outputs and values, 2e-5 for backward sums and dx.  `kernel` is the worst error
the MI355X showed (each test prints its own).  Distances are relative norms |a-b|/|b| unless said otherwise.

  quantity                                   fp32 CPU vs f64    bar = min(4x, cap)    kernel (worst observed)
  graph_aggregate y                          8.12e-8            3.25e-7               8.1e-8
  gln mean   max_g |d|/(|mean|+std)          1.31e-7            5.24e-7               6.3e-8
  gln std    max_g |d|/std                   5.96e-8            2.38e-7               8.4e-8 (3.8e-7 before the statistics fix)
  gln y                                      9.35e-8            3.74e-7               1.4e-7
  gln dx                                     1.17e-7            4.68e-7               2.0e-7
  gln dgamma                                 1.92e-7            7.68e-7               2.5e-7
  gln dbeta                                  1.71e-7            6.84e-7               3.0e-7
  pose_loss values  max_h |d|/|v_h|          3.09e-7            1.24e-6               3.6e-7
  pose_loss grad_pred / grad_aux             2.97e-7            1.19e-6               4.0e-7
  lsgan value  |d|/|v|                       1.10e-7            4.40e-7               1.1e-7
  lsgan grad                                 6.31e-8            2.52e-7               6.3e-8

The shifted-pivot statistics under stress are not held to ATen's two-pass std but to the bound of the one-pass algorithm
(test_gln_statistics_under_stress)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')
EPS = float(np.float32(1e-5))           # the eps the kernel receives, as a double
CAP_VALUE, CAP_BWD = 3e-6, 2e-5
# worst fp32-CPU-vs-float64 distance over this file's cases, as measure_reference_distances() below gave it
MEASURED = {'agg_y': 8.12e-8, 'gln_mean': 1.31e-7, 'gln_std': 5.96e-8, 'gln_y': 9.35e-8, 'gln_dx': 1.17e-7, 'gln_dg': 1.92e-7,
            'gln_db': 1.71e-7, 'pose_v': 3.09e-7, 'pose_g': 2.97e-7, 'lsgan_v': 1.10e-7, 'lsgan_g': 6.31e-8}
CAPS = {k: (CAP_BWD if k in ('gln_dx', 'gln_dg', 'gln_db', 'pose_g', 'lsgan_g') else CAP_VALUE) for k in MEASURED}
BAR = {k: min(4 * MEASURED[k], CAPS[k]) for k in MEASURED}


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def relmax(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b).abs() / b.abs()).max())


def leaf(t, dt):
    """a fresh autograd leaf of dtype dt (never the caller's tensor itself)"""
    return t.detach().to(dt).clone().requires_grad_(True)


def nans(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -12345, dtype=dtype, device='cuda')
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


def check(what, err, bar):
    print('%s: error %.3g, bar %.3g' % (what, err, bar))
    assert err <= bar, '%s: error %.3g above the bar %.3g' % (what, err, bar)


# ----------------------------------------------------------------------------------------------------- graph_aggregate
AGG_CASES = [(1, 1, 1), (2, 18, 128), (3, 17, 5), (2, 18, 130), (33, 18, 128), (500, 18, 128)]


def _adjacencies(N):
    """name -> [N, N] fp32: the row-normalised skeleton with self-loops (a chain where N is not the workload's 18), a dense
    random matrix, one with an all-zero row, and the transpose of each (the backward's operand)."""
    import inputs as gi
    from oracle import geometry as geo
    from oracle import nets as onets
    if N == 18:
        p, c = geo.skeleton_links(gi.HM36_PARENTS, gi.LINE_SELECT, False, False)
    else:
        p, c = list(range(N - 1)), list(range(1, N))
    gen = torch.Generator().manual_seed(40 + N)
    out = {'skeleton': onets.mean_adjacency(N, p, c).float(), 'dense': torch.randn(N, N, generator=gen)}
    z = torch.randn(N, N, generator=gen)
    z[N // 2] = 0.0
    out['zero_row'] = z
    for k in list(out):
        out[k + '.T'] = out[k].t().contiguous()
    return out


def _agg_ref(x, adj, dt):
    return torch.einsum('ij,bjc->bic', adj.to(dt), x.to(dt))


def _agg_x(B, N, C):
    return torch.randn(B, N, C, generator=torch.Generator().manual_seed(B * 1000 + N * 10 + C))


@pytest.mark.parametrize('B,N,C', AGG_CASES)
def test_graph_aggregate(B, N, C):
    """y[b,i,:] = sum_j adj[i,j] x[b,j,:] for every adjacency and its transpose; the last shape has more elements than the
    4096 x 256 threads of the capped grid (grid-stride loop), (33,18,128) a ragged last block."""
    from xas_amd._lib import call, ptr
    x = _agg_x(B, N, C)
    xg = x.cuda()
    worst = 0.0
    for name, adj in _adjacencies(N).items():
        y = nans(B, N, C)
        ag = adj.cuda()
        call('xas_graph_aggregate', ptr(xg), ptr(ag), B, N, C, ptr(y))
        y = y.cpu()
        assert torch.isfinite(y).all(), name
        ref = _agg_ref(x, adj, torch.float64)
        if name.startswith('zero_row'):
            zero = (adj == 0).all(dim=1)
            assert zero.any() == (not name.endswith('.T') or N == 1)
            assert (y[:, zero] == 0).all()
        worst = max(worst, rel(y, ref))
    check('graph_aggregate y (%d,%d,%d)' % (B, N, C), worst, BAR['agg_y'])


# ----------------------------------------------------------------------------------------------------- graph LayerNorm
GLN_CASES = [(1, 3, 1), (36, 128, 1), (576, 128, 5), (15, 63, 2), (17, 65, 3), (100, 130, 2), (7, 300, 2), (2, 5, 65),
             (33, 64, 2), (2049, 64, 1), (2049, 64, 9)]


def _gln_pre(x, gamma, beta):
    """float64: group mean, biased std, x-hat and the pre-activation x-hat * gamma + beta.  x [G, rows, C]."""
    x = x.double()
    flat = x.reshape(x.shape[0], -1)
    mean, std = flat.mean(1)[:, None, None], flat.std(1, unbiased=False)[:, None, None]
    xh = (x - mean) / (std + EPS)
    return mean, std, xh, xh * gamma.double() + beta.double()


def _relu_margins(x, gamma, beta):
    """-> |pre-activation|, the issue's margin 2e-6 (|gamma||x^| + |beta|), and a stronger one that also covers what an
    fp32 kernel cannot avoid: the stored mean is rounded to fp32 (2^-24 |mean| / std in x^) and so is 1 / (std + eps)."""
    mean, std, xh, pre = _gln_pre(x, gamma, beta)
    g, b = gamma.double().abs(), beta.double().abs()
    return pre.abs(), 2e-6 * (g * xh.abs() + b), 2e-6 * (g * (xh.abs() + mean.abs() / std + 1.0) + b)


def _gln_inputs(rows, C, G):
    """Groups with visibly different means and scales; gamma with negative entries, channel 0 with gamma = beta = 0 and
    channel 1 with gamma = 0, beta > 0; beta small and of both signs, so that about half the outputs are clipped.  The
    ReLU mask is the one place where a float64 reference and a correct fp32 kernel may disagree, so every element whose
    pre-activation is too close to zero to call is moved away from it here, on the CPU, before anything is computed (a
    seed search cannot clear 10^6 elements); the tests assert the outcome as a precondition and drop no element."""
    gen = torch.Generator().manual_seed(rows * 100003 + C * 101 + G)
    gi = torch.arange(G)
    mean = (0.2 + (gi % 7).float())[:, None, None]
    scale = (1.0 + 0.5 * (gi % 5).float())[:, None, None]
    x = mean + scale * torch.randn(G, rows, C, generator=gen)
    gamma = torch.randn(C, generator=gen)
    beta = 0.3 * torch.randn(C, generator=gen)
    gamma[0], beta[0] = 0.0, 0.0
    gamma[1], beta[1] = 0.0, 0.5
    res = torch.randn(G, rows, C, generator=gen)
    dy = torch.randn(G, rows, C, generator=gen)
    live = gamma != 0
    for _ in range(100):
        pre, _, strong = _relu_margins(x, gamma, beta)
        bad = (pre <= 4 * strong) & live
        if not bad.any():
            break
        x = torch.where(bad, x + 0.01 * scale, x)
    return x, gamma, beta, res, dy


@functools.lru_cache(maxsize=None)
def _gln_reference(rows, C, G, dt=torch.float64):
    """Inputs (fp32) and the reference in `dt`: stats, y without and with residual, and autograd's dx, dgamma, dbeta."""
    x, gamma, beta, res, dy = _gln_inputs(rows, C, G)
    xd, gd, bd = leaf(x, dt), leaf(gamma, dt), leaf(beta, dt)
    flat = xd.reshape(G, -1)
    mean, std = flat.mean(1), flat.std(1, unbiased=False)
    eps = EPS if dt == torch.float64 else 1e-5
    y = torch.relu((xd - mean[:, None, None]) / (std[:, None, None] + eps) * gd + bd)
    dx, dg, db = torch.autograd.grad(y, (xd, gd, bd), dy.to(dt))
    return dict(x=x, gamma=gamma, beta=beta, res=res, dy=dy, mean=mean.detach(), std=std.detach(), y=y.detach(),
                y_res=(y + res.to(dt)).detach(), dx=dx, dg=dg, db=db)


def _gln_fwd(x, gamma, beta, res, G, rows, C):
    from xas_amd._lib import call, ptr, query
    y, stats = nans(G * rows, C), nans(G, 2)
    ws = nans(query('xas_gln_workspace_floats', rows * C, G, C))
    call('xas_gln_fwd', ptr(x), ptr(gamma), ptr(beta), ptr(res), rows, C, G, 1e-5, ptr(y), ptr(stats), ptr(ws))
    return y, stats


def _gln_bwd(x, gamma, beta, dy, stats, G, rows, C):
    from xas_amd._lib import call, ptr, query
    dx, dg, db = nans(G * rows, C), nans(C), nans(C)
    ws = nans(query('xas_gln_workspace_floats', rows * C, G, C))
    call('xas_gln_bwd', ptr(x), ptr(beta), ptr(dy), ptr(gamma), ptr(stats), rows, C, G, 1e-5, ptr(dx), ptr(dg), ptr(db), ptr(ws))
    return dx, dg, db


def _stat_errors(stats, mean, std):
    stats = stats.cpu().double()
    return (float(((stats[:, 0] - mean.double()).abs() / (mean.double().abs() + std.double())).max()),
            float(((stats[:, 1] - std.double()).abs() / std.double()).max()))


@pytest.mark.parametrize('rows,C,G', GLN_CASES)
def test_gln_forward(rows, C, G):
    """stats[g] = (mean, biased std) of group g's own rows and y = relu((x - mean) / (std + eps) gamma + beta) (+ res):
    C not a multiple of 64, one row, fewer than 16 rows, more than 64 groups (second block of the statistics kernel), n just
    over one partial block, n past the cap of 64 partial blocks, n G past the cap of 4096 apply blocks."""
    r = _gln_reference(rows, C, G)
    x, gamma, beta, res = (r[k].cuda() for k in ('x', 'gamma', 'beta', 'res'))
    x, res = x.reshape(G * rows, C), res.reshape(G * rows, C)
    y, stats = _gln_fwd(x, gamma, beta, None, G, rows, C)
    y2, stats2 = _gln_fwd(x, gamma, beta, res, G, rows, C)
    assert torch.isfinite(y).all() and torch.isfinite(y2).all() and torch.isfinite(stats).all()
    assert torch.equal(stats, stats2)
    em, es = _stat_errors(stats, r['mean'], r['std'])
    clipped = float((r['y'] == 0).double().mean())
    assert rows * C * G < 100 or 0.3 < clipped < 0.7, clipped
    assert (y.cpu().reshape(G, rows, C)[:, :, 0] == 0).all() and (y.cpu().reshape(G, rows, C)[:, :, 1] == 0.5).all()
    tag = '(%d,%d,%d)' % (rows, C, G)
    check('gln mean ' + tag, em, BAR['gln_mean'])
    check('gln std ' + tag, es, BAR['gln_std'])
    check('gln y ' + tag, rel(y, r['y'].reshape(G * rows, C)), BAR['gln_y'])
    check('gln y+res ' + tag, rel(y2, r['y_res'].reshape(G * rows, C)), BAR['gln_y'])
    # group by group as well: a group that borrowed a neighbour's statistics or rows cannot hide in the whole norm
    yg = y.cpu().reshape(G, rows, C)
    check('gln y per group ' + tag, max(rel(yg[g], r['y'][g]) for g in range(G)), BAR['gln_y'])


@pytest.mark.parametrize('rows,C,G', GLN_CASES)
def test_gln_backward(rows, C, G):
    """dx, dgamma, dbeta from the statistics the forward wrote, against float64 autograd of the same expression (dgamma and
    dbeta summed over the groups).  Precondition, asserted: no pre-activation of a channel with gamma != 0 is close enough
    to zero for fp32 and float64 to disagree about the mask (the stronger of the two margins implies the other); in the two
    channels with gamma = 0 the pre-activation is exactly beta on both sides, and relu'(0) = 0 on both."""
    r = _gln_reference(rows, C, G)
    pre, weak, strong = _relu_margins(r['x'], r['gamma'], r['beta'])
    live = r['gamma'] != 0
    assert bool((strong >= weak).all()) and bool((pre > strong)[:, :, live].all())
    assert float(r['dg'][0]) == 0.0 and float(r['db'][0]) == 0.0
    x, gamma, beta, dy = (r[k].cuda() for k in ('x', 'gamma', 'beta', 'dy'))
    x, dy = x.reshape(G * rows, C), dy.reshape(G * rows, C)
    _, stats = _gln_fwd(x, gamma, beta, None, G, rows, C)
    dx, dg, db = _gln_bwd(x, gamma, beta, dy, stats, G, rows, C)
    assert torch.isfinite(dx).all() and torch.isfinite(dg).all() and torch.isfinite(db).all()
    assert float(dg[0]) == 0.0 and float(db[0]) == 0.0
    tag = '(%d,%d,%d)' % (rows, C, G)
    check('gln dx ' + tag, rel(dx, r['dx'].reshape(G * rows, C)), BAR['gln_dx'])
    dxg = dx.cpu().reshape(G, rows, C)
    check('gln dx per group ' + tag, max(rel(dxg[g], r['dx'][g]) for g in range(G)), BAR['gln_dx'])
    check('gln dgamma ' + tag, rel(dg, r['dg']), BAR['gln_dg'])
    check('gln dbeta ' + tag, rel(db, r['db']), BAR['gln_db'])


@pytest.mark.parametrize('rows,C,G', [(36, 128, 1), (17, 65, 3)])
def test_gln_autograd_function_passes_dy_to_the_residual(rows, C, G):
    """ops_misc._GraphLayerNormRelu: the residual's gradient is dy itself, and x, gamma, beta get what the entry point
    wrote."""
    from xas_amd import ops_misc
    r = _gln_reference(rows, C, G)
    x, res, dy = (r[k].reshape(G * rows, C).cuda() for k in ('x', 'res', 'dy'))
    gamma, beta = r['gamma'].cuda(), r['beta'].cuda()
    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta, res)]
    y = ops_misc.graph_layernorm_relu(*leaves, eps=1e-5, groups=G)
    y.backward(dy)
    y2, stats = _gln_fwd(x, gamma, beta, res, G, rows, C)
    dx, dg, db = _gln_bwd(x, gamma, beta, dy, stats, G, rows, C)
    assert torch.equal(y.detach(), y2) and torch.equal(leaves[3].grad, dy)
    assert torch.equal(leaves[0].grad, dx) and torch.equal(leaves[1].grad, dg) and torch.equal(leaves[2].grad, db)


def _stress_group(n, ratio, delta, sigma, gen):
    z = torch.randn(n, generator=gen, dtype=torch.float64)
    z = (z - z.mean()) / z.std(unbiased=False)
    x = (ratio * sigma + sigma * z).float()
    x[0] = float(ratio * sigma + delta * sigma)
    return x


@pytest.mark.parametrize('delta', [0, 4, 8])
@pytest.mark.parametrize('ratio', [0, 1e3, 1e5])
def test_gln_statistics_under_stress(ratio, delta):
    """The one-pass shifted sums (pivot = the group's first element) at mean/std = ratio, with the pivot planted delta
    standard deviations off the mean.  Bound from the algorithm, with d = (x[g n] - mean) / std of the fp32 data: the fp32
    sum of (x - pivot)^2 carries terms of size (d std)^2 next to the variance, so the relative error of the variance is
    <= 8 * 2^-23 * (1 + d^2); the sum of (x - pivot) carries terms of size |d| std, so the mean is off by at most
    8 * 2^-23 * std * (1 + |d|), plus half an ulp of the mean itself for storing it as a float."""
    rows, C, G = 36, 128, 2
    n = rows * C
    gen = torch.Generator().manual_seed(int(ratio) + 17 * delta)
    x = torch.stack([_stress_group(n, ratio, delta, s, gen) for s in (1.0, 3.0)])
    xd = x.double()
    mean, std = xd.mean(1), xd.std(1, unbiased=False)
    d = (xd[:, 0] - mean) / std
    assert bool(((d - delta).abs() < 0.1).all())          # planting the pivot itself widens std a little
    gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
    _, stats = _gln_fwd(x.reshape(G * rows, C).cuda(), gamma, beta, None, G, rows, C)
    stats = stats.cpu().double()
    u = 2.0 ** -23
    for g in range(G):
        var_err = abs(float(stats[g, 1]) ** 2 - float(std[g]) ** 2) / float(std[g]) ** 2
        var_bar = 8 * u * (1 + float(d[g]) ** 2)
        mean_err = abs(float(stats[g, 0]) - float(mean[g]))
        mean_bar = 8 * u * float(std[g]) * (1 + abs(float(d[g]))) + 0.5 * u * abs(float(mean[g]))
        print('gln stats mean/std=%g delta=%g group %d: variance rel. error %.3g (bound %.3g), mean error %.3g (bound %.3g)'
              % (ratio, delta, g, var_err, var_bar, mean_err, mean_bar))
        assert var_err <= var_bar and mean_err <= mean_bar


def test_gln_constant_group_is_exact():
    """A constant group: every intermediate is exact, so stats are exactly (c, 0) and y is exactly relu(beta) + res; the
    backward's own reference is NaN there (0/0), so only finiteness of dx is asked for std = 0.  The group next to it keeps
    its own statistics."""
    rows, C, G = 36, 128, 2
    r = _gln_reference(rows, C, 1)
    c = float(np.float32(1.7))
    x = torch.cat([torch.full((1, rows, C), c), r['x']]).reshape(G * rows, C).cuda()
    res = torch.cat([r['res'], r['res']]).reshape(G * rows, C).cuda()
    dy = torch.cat([r['dy'], r['dy']]).reshape(G * rows, C).cuda()
    gamma, beta = r['gamma'].cuda(), r['beta'].cuda()
    y, stats = _gln_fwd(x, gamma, beta, res, G, rows, C)
    assert torch.equal(stats[0].cpu(), torch.tensor([c, 0.0]))
    assert torch.equal(y[:rows].cpu(), torch.relu(r['beta'])[None, :] + r['res'][0])
    em, es = _stat_errors(stats[1:], r['mean'], r['std'])
    check('gln mean next to a constant group', em, BAR['gln_mean'])
    check('gln std next to a constant group', es, BAR['gln_std'])
    check('gln y next to a constant group', rel(y[rows:], r['y_res'][0]), BAR['gln_y'])
    dx, dg, db = _gln_bwd(x, gamma, beta, dy, stats, G, rows, C)
    assert torch.isfinite(dx).all() and torch.isfinite(dg).all() and torch.isfinite(db).all()
    check('gln dx next to a constant group', rel(dx[rows:], r['dx'][0]), BAR['gln_dx'])


# ----------------------------------------------------------------------------------------------------- pose_loss
POSE_CASES = [(1, 1, 17), (32, 3, 18), (257, 6, 18), (5, 2, 24)]
POSE_FORMS = ['sup', 'sym', 'sym+2d', 'kp2d']           # kind 0, kind 1 without / with the 2-D term and grad_aux, kind 2
KIND = {'sup': 0, 'sym': 1, 'sym+2d': 1, 'kp2d': 2}
WEIGHTS = {'sup': [(1.0, 0.0, 0.0)], 'kp2d': [(0.7, 0.0, 0.0)], 'sym': [(0.3, 0.05, 0.0), (0.0, 0.05, 0.0), (0.3, 0.0, 0.0)],
           'sym+2d': [(0.3, 0.05, 50.0), (0.0, 0.05, 50.0), (0.3, 0.0, 50.0), (0.3, 0.05, 0.0)]}
UPSTREAM = 1.7
_FAR, _NEAR = [16, 15, 13, 12, 3, 2, 6, 5], [15, 14, 12, 11, 2, 1, 5, 4]


def _bone_sym_guarded(kp):
    """oracle.losses.bone_sym with a limb of zero length detached: it contributes its (zero) length and no gradient."""
    sq = ((kp[:, _FAR] - kp[:, _NEAR]) ** 2).sum(dim=2)
    bone = torch.where(sq > 0, sq.clamp_min(1e-300).sqrt(), torch.zeros_like(sq)) * 1e-3
    return ((bone[:, 0::2] - bone[:, 1::2]) ** 2).mean()


def _pose_values(form, pred, aux, w, guarded=False):
    """[Hy] values of every hypothesis in pred's dtype, from the oracle's loss functions."""
    from oracle import losses as L
    vs = []
    for h in range(pred.shape[1]):
        p = pred[:, h]
        if form == 'sup':
            v = L.supervision(p, aux)
        elif form == 'kp2d':
            v = w[0] * L.kp_sym(p[:, :, :2], False)
        else:
            v = w[0] * (_bone_sym_guarded(p) if guarded else L.bone_sym(p)) + w[1] * L.kp_sym(p)
            if form == 'sym+2d':
                v = v + w[2] * L.kp_sym(aux[:, h, :, :2], False)
        vs.append(v)
    return torch.stack(vs)


def _pose_inputs(form, B, Hy, K, h_min, seed=0):
    """fp32 pred [B,Hy,K,3] and aux (gt [B,K,3] for the supervision, patch joints [B,Hy,K,3] for the 2-D term), with the
    minimum placed at hypothesis h_min by scaling: mm-scale joints for the 3-D symmetry, patch scale otherwise."""
    gen = torch.Generator().manual_seed(7 + seed + B * 31 + Hy * 5 + K + 1000 * POSE_FORMS.index(form))
    s = torch.tensor([0.2 if h == h_min else 1.0 + 0.1 * h for h in range(Hy)])[None, :, None, None]
    base = torch.randn(B, Hy, K, 3, generator=gen)
    if form == 'sup':
        gt = torch.randn(B, K, 3, generator=gen) * 0.5
        return (gt[:, None] + 0.3 * base * s).contiguous(), gt
    if form == 'kp2d':
        return (0.5 * base * s).contiguous(), None
    pred = (400.0 * base * s).contiguous()
    if form == 'sym':
        return pred, None
    return pred, (0.5 * torch.randn(B, Hy, K, 3, generator=gen) * s).contiguous()


def _pose_gpu(form, pred, aux, w, with_grad_aux=None):
    """-> out [2+Hy], grad_pred, grad_aux (or None) on the CPU, every buffer NaN before the launch."""
    from xas_amd._lib import call, ptr
    B, Hy, K, _ = pred.shape
    kind = KIND[form]
    pg = pred.cuda()
    ag = aux.cuda() if aux is not None else None
    out, gp = nans(2 + Hy), nans(B, Hy, K, 3)
    if with_grad_aux is None:
        with_grad_aux = form == 'sym+2d'
    ga = nans(B, Hy, K, 3) if with_grad_aux else None
    up = torch.tensor([UPSTREAM], device='cuda')
    call('xas_pose_loss_fwd', ptr(pg), ptr(ag), B, Hy, K, kind, w[0], w[1], w[2], ptr(out))
    call('xas_pose_loss_bwd', ptr(pg), ptr(ag), B, Hy, K, kind, w[0], w[1], w[2], ptr(out), ptr(up), ptr(gp), ptr(ga))
    return out.cpu(), gp.cpu(), (ga.cpu() if ga is not None else None)


def _pose_reference(form, pred, aux, w, dt=torch.float64, pick=None, guarded=False):
    """values [Hy] and the gradients of UPSTREAM * min_h v_h (torch.min over the stack, as the reference model takes it) or,
    with `pick`, of UPSTREAM * v_pick."""
    p = leaf(pred, dt)
    a = None if aux is None else (leaf(aux, dt) if form == 'sym+2d' else aux.to(dt))
    v = _pose_values(form, p, a, w, guarded)
    top = v.min() if pick is None else v[pick]
    leaves = (p, a) if form == 'sym+2d' and w[2] != 0 else (p,)
    g = torch.autograd.grad(top * UPSTREAM, leaves)
    return v.detach(), g[0], (g[1] if len(g) > 1 else (torch.zeros_like(p) if form == 'sym+2d' else None))


def _check_pose(tag, out, gp, ga, v, rp, ra, best):
    Hy = v.numel()
    assert float(out[1]) == best, (tag, out)
    assert float(out[0]) == float(out[2 + best])
    check('pose values ' + tag, relmax(out[2:], v), BAR['pose_v'])
    check('pose grad_pred ' + tag, rel(gp, rp), BAR['pose_g'])
    others = [h for h in range(Hy) if h != best]
    assert (gp[:, others] == 0).all(), tag
    if ga is not None:
        assert (ga[:, others] == 0).all(), tag
        if float(ra.abs().max()) == 0.0:
            assert (ga == 0).all(), tag
        else:
            check('pose grad_aux ' + tag, rel(ga, ra), BAR['pose_g'])


@pytest.mark.parametrize('form', POSE_FORMS)
@pytest.mark.parametrize('B,Hy,K', POSE_CASES)
def test_pose_loss(B, Hy, K, form):
    """Minimum, argmin, every hypothesis's value, grad_pred and grad_aux with the minimum at each hypothesis in turn, one
    weight zero at a time and an upstream gradient of 1.7; B = 257 takes the stride loops, B = 1 and Hy = 1, 6 the ends."""
    for h_min in range(Hy):
        pred, aux = _pose_inputs(form, B, Hy, K, h_min)
        for w in WEIGHTS[form]:
            if w[0] == 0.0 and w[1] == 0.0:
                continue
            v, rp, ra = _pose_reference(form, pred, aux, w)
            best = int(v.argmin())
            assert best == h_min
            if Hy > 1:          # a clear minimum: fp32 and float64 agree on it
                lo = v.sort()[0]
                assert float(lo[1] - lo[0]) > 1e-3 * float(lo[1])
            out, gp, ga = _pose_gpu(form, pred, aux, w)
            assert torch.isfinite(out).all() and torch.isfinite(gp).all()
            _check_pose('%s (%d,%d,%d) min at %d w=%s' % (form, B, Hy, K, h_min, w), out, gp, ga, v, rp, ra, best)
    if form == 'sym+2d':
        # the 2-D term in the value, its gradient not asked for: grad_pred is what it was
        w = WEIGHTS[form][0]
        out2, gp2, ga2 = _pose_gpu(form, pred, aux, w, with_grad_aux=False)
        out1, gp1, _ = _pose_gpu(form, pred, aux, w)
        assert ga2 is None and torch.equal(out1, out2) and torch.equal(gp1, gp2)


@pytest.mark.parametrize('form', POSE_FORMS)
@pytest.mark.parametrize('B,Hy,K', [c for c in POSE_CASES if c[1] > 1])
def test_pose_loss_exact_tie(B, Hy, K, form):
    """Hypothesis 1 a copy of hypothesis 0, both the minimum: equal values, argmin 0, and the whole gradient goes to
    hypothesis 0 (the reference's full-reduction torch.min would split it evenly between the two: checked below)."""
    pred, aux = _pose_inputs(form, B, Hy, K, 0)
    pred[:, 1] = pred[:, 0]
    if form == 'sym+2d':
        aux[:, 1] = aux[:, 0]
    w = WEIGHTS[form][0]
    v, rp, ra = _pose_reference(form, pred, aux, w, pick=0)
    assert float(v[0]) == float(v[1]) == float(v.min())
    split = _pose_reference(form, pred, aux, w)[1]
    assert torch.equal(split[:, 0], split[:, 1]) and rel(2 * split[:, 0], rp[:, 0]) < 1e-12
    out, gp, ga = _pose_gpu(form, pred, aux, w)
    assert float(out[2]) == float(out[3])
    _check_pose('%s (%d,%d,%d) tie' % (form, B, Hy, K), out, gp, ga, v, rp, ra, 0)


@pytest.mark.parametrize('form', ['sym', 'sym+2d'])
@pytest.mark.parametrize('B,Hy,K', POSE_CASES)
def test_pose_loss_limb_of_zero_length(B, Hy, K, form):
    """Joint 16 on top of joint 15 in one sample of the winning hypothesis: the limb's length is exactly 0, the kernel's
    `len > 0` guard gives it no gradient; everything is finite and equals the reference with that limb's length detached."""
    h_min = Hy - 1
    pred, aux = _pose_inputs(form, B, Hy, K, h_min, seed=1)
    pred[0, h_min, 16] = pred[0, h_min, 15]
    w = WEIGHTS[form][0]
    v, rp, ra = _pose_reference(form, pred, aux, w, guarded=True)
    assert int(v.argmin()) == h_min and torch.isfinite(rp).all()
    out, gp, ga = _pose_gpu(form, pred, aux, w)
    assert torch.isfinite(out).all() and torch.isfinite(gp).all()
    _check_pose('%s (%d,%d,%d) zero limb' % (form, B, Hy, K), out, gp, ga, v, rp, ra, h_min)


@pytest.mark.parametrize('form', POSE_FORMS)
@pytest.mark.parametrize('B,Hy,K', POSE_CASES)
def test_pose_loss_nan_wins_the_minimum(B, Hy, K, form):
    """A NaN in one hypothesis - the first, a middle one, the last - is the minimum, as torch.min gives: out[0] is NaN, the
    argmin names that hypothesis, its gradient is not finite, the clean hypotheses keep finite values and zero gradient.
    With two NaN hypotheses the first one is named."""
    w = WEIGHTS[form][0]
    for planted in sorted({(0,), (Hy // 2,), (Hy - 1,), (min(1, Hy - 1), Hy - 1)}):
        pred, aux = _pose_inputs(form, B, Hy, K, 0, seed=2)
        for h in planted:
            pred[B // 2, h, 11, 0] = NAN
        v = _pose_reference(form, pred.nan_to_num(0.0), aux, w)[0]
        ref_min = _pose_values(form, pred.double(), aux.double() if aux is not None else None, w).min()
        assert bool(torch.isnan(ref_min))
        out, gp, ga = _pose_gpu(form, pred, aux, w)
        tag = '%s (%d,%d,%d) NaN in %s' % (form, B, Hy, K, planted)
        assert bool(torch.isnan(out[0])) and float(out[1]) == planted[0], (tag, out)
        clean = [h for h in range(Hy) if h not in planted]
        assert bool(torch.isnan(out[2:][list(planted)]).all()), (tag, out)
        if clean:
            check('pose values of the clean hypotheses, ' + tag, relmax(out[2:][clean], v[clean]), BAR['pose_v'])
        assert not bool(torch.isfinite(gp[:, planted[0]]).all()), tag
        rest = [h for h in range(Hy) if h != planted[0]]
        assert (gp[:, rest] == 0).all(), tag
        if ga is not None:
            assert (ga[:, rest] == 0).all(), tag


# ----------------------------------------------------------------------------------------------------- lsgan
LSGAN_CASES = [(1, 1), (32, 1), (32, 3), (257, 6)]


def _lsgan_inputs(B, Hy, target, place):
    gen = torch.Generator().manual_seed(B * 10 + Hy + int(target))
    x = torch.randn(B, Hy, generator=gen)
    if place:           # per-sample minimum at h = b % Hy: that logit close to the target, the others at least 1 away
        far = target + (1.0 + torch.rand(B, Hy, generator=gen)) * torch.where(torch.rand(B, Hy, generator=gen) < 0.5, -1.0, 1.0)
        near = target + 0.2 * torch.randn(B, Hy, generator=gen)
        x = torch.where(torch.arange(Hy)[None, :] == (torch.arange(B) % Hy)[:, None], near, far)
    return x.contiguous()


def _lsgan_reference(x, target, dt=torch.float64):
    from oracle import losses as L
    xd = leaf(x, dt)
    v = L._lsgan_term(xd.unsqueeze(2), target)
    (g,) = torch.autograd.grad(v * UPSTREAM, xd)
    return v.detach(), ((xd.detach() - target) ** 2).argmin(dim=1), g


def _lsgan_gpu(x, target):
    from xas_amd._lib import call, ptr
    B, Hy = x.shape
    xg = x.cuda()
    out, idx, gx = nans(1), nans(B, dtype=torch.int32), nans(B, Hy)
    up = torch.tensor([UPSTREAM], device='cuda')
    call('xas_lsgan_fwd', ptr(xg), B, Hy, float(target), ptr(out), ptr(idx))
    call('xas_lsgan_bwd', ptr(xg), B, Hy, float(target), ptr(idx), ptr(up), ptr(gx))
    return out.cpu(), idx.cpu(), gx.cpu()


@pytest.mark.parametrize('place', [False, True], ids=['random', 'min_at_each_h'])
@pytest.mark.parametrize('target', [0.0, 1.0])
@pytest.mark.parametrize('B,Hy', LSGAN_CASES)
def test_lsgan(B, Hy, target, place):
    """mean_b min_h (x - t)^2, the per-sample argmin and the gradient, also with an exact tie inside sample 0 (first index
    wins and alone gets gradient); B = 257 takes the stride loops."""
    x = _lsgan_inputs(B, Hy, target, place)
    if Hy > 1 and not place:
        x[0] = target + 2.0
        x[0, Hy - 2] = x[0, Hy - 1] = target + 0.125
    v, ridx, rg = _lsgan_reference(x, target)
    e = ((x.double() - target) ** 2).sort(dim=1)[0]
    if Hy > 1:          # no near-ties other than the planted one: fp32 and float64 agree on every argmin
        gap = (e[:, 1] - e[:, 0]) / e[:, 1]
        assert bool((gap[0 if place else 1:] > 1e-5).all())
    out, idx, gx = _lsgan_gpu(x, target)
    assert torch.equal(idx.long(), ridx)
    if place:
        assert torch.equal(idx.long(), torch.arange(B) % Hy)
    elif Hy > 1:
        assert int(idx[0]) == Hy - 2 and float(gx[0, Hy - 1]) == 0.0 and float(gx[0, Hy - 2]) != 0.0
    tag = '(%d,%d) t=%g %s' % (B, Hy, target, 'placed' if place else 'random')
    check('lsgan value ' + tag, abs(float(out[0]) - float(v)) / abs(float(v)), BAR['lsgan_v'])
    check('lsgan grad ' + tag, rel(gx, rg), BAR['lsgan_g'])
    assert ((gx != 0).sum(dim=1) <= 1).all()


@pytest.mark.parametrize('target', [0.0, 1.0])
@pytest.mark.parametrize('B,Hy', LSGAN_CASES)
def test_lsgan_nan_wins_the_minimum(B, Hy, target):
    """One NaN logit in sample 0 (not in front where there is a choice) and, where there is a second sample, all NaN in the
    last: the value is NaN as min(dim=1)[0].mean() gives, the gradient is not finite in those samples and only there."""
    x = _lsgan_inputs(B, Hy, target, False)
    clean_ref = _lsgan_reference(x, target)[2]
    x[0, Hy - 1] = NAN
    sick = [0]
    if B > 1:
        x[B - 1] = NAN
        sick.append(B - 1)
    v, ridx, _ = _lsgan_reference(x, target)
    assert bool(torch.isnan(v))
    out, idx, gx = _lsgan_gpu(x, target)
    assert bool(torch.isnan(out[0]))
    assert int(idx[0]) == Hy - 1 == int(ridx[0]) and int(idx[B - 1]) == int(ridx[B - 1])
    for b in sick:
        assert bool(torch.isnan(gx[b, int(idx[b])])) and int((gx[b] == 0).sum()) == Hy - 1
    well = [b for b in range(B) if b not in sick]
    if well:
        assert torch.isfinite(gx[well]).all()
        check('lsgan grad of the clean samples (%d,%d) t=%g' % (B, Hy, target), rel(gx[well], clean_ref[well]), BAR['lsgan_g'])


# ----------------------------------------------------------------------------------------------------- how the bars were measured
def measure_reference_distances():
    """fp32 CPU (ATen) against float64 on the inputs of every case above -> {quantity: worst distance}."""
    worst = {k: 0.0 for k in BAR}

    def up(k, e):
        worst[k] = max(worst[k], e)

    for B, N, C in AGG_CASES:
        x = _agg_x(B, N, C)
        for adj in _adjacencies(N).values():
            up('agg_y', rel(_agg_ref(x, adj, torch.float32), _agg_ref(x, adj, torch.float64)))
    for rows, C, G in GLN_CASES:
        a, b = _gln_reference(rows, C, G, torch.float32), _gln_reference(rows, C, G)
        up('gln_mean', float(((a['mean'].double() - b['mean']).abs() / (b['mean'].abs() + b['std'])).max()))
        up('gln_std', float(((a['std'].double() - b['std']).abs() / b['std']).max()))
        up('gln_y', max(rel(a['y'], b['y']), rel(a['y_res'], b['y_res'])))
        up('gln_dx', rel(a['dx'], b['dx']))
        up('gln_dg', rel(a['dg'], b['dg']))
        up('gln_db', rel(a['db'], b['db']))
    for B, Hy, K in POSE_CASES:
        for form in POSE_FORMS:
            for h_min in range(Hy):
                pred, aux = _pose_inputs(form, B, Hy, K, h_min)
                for w in WEIGHTS[form]:
                    a, b = _pose_reference(form, pred, aux, w, torch.float32), _pose_reference(form, pred, aux, w)
                    up('pose_v', relmax(a[0], b[0]))
                    up('pose_g', rel(a[1], b[1]))
                    if b[2] is not None and float(b[2].abs().max()) > 0:
                        up('pose_g', rel(a[2], b[2]))
    for B, Hy in LSGAN_CASES:
        for target in (0.0, 1.0):
            for place in (False, True):
                x = _lsgan_inputs(B, Hy, target, place)
                a, b = _lsgan_reference(x, target, torch.float32), _lsgan_reference(x, target)
                up('lsgan_v', abs(float(a[0]) - float(b[0])) / abs(float(b[0])))
                up('lsgan_g', rel(a[2], b[2]))
    return worst


if __name__ == '__main__':
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, 'tests', 'golden')]
    for k, e in measure_reference_distances().items():
        print('%-10s fp32 CPU vs float64 %.3g   4x = %.3g   cap %.0e   bar %.3g' % (k, e, 4 * e, CAPS[k], min(4 * e, CAPS[k])))
