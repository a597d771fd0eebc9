"""The column-reduction kernel of csrc/bn.hip (col_reduce_body: one template, modes 0-6, two builds, four slab targets,
1-64 groups, finalize folded into the launch behind a ticket counter) ALONE against float64, through the C ABI.

Naming: mode 0 xas_bn_stats; 1 xas_bn_bwd_reduce with x and y ('xy') or the sign bytes ('xm'); 3 without x ('y'); 4 without y
('x'); 2 xas_col_sum / xas_col_sum_acc; 5 xas_bn_stats_from_partials; 6 xas_bn_bwd_sums_from_partials.

Two kinds of input.
  exact : small integers, every fp32 partial sum an integer below 2^24 (asserted from the float64 reference before the launch:
          sum |term| < 2^24 bounds every partial sum).  The kernel's sums then carry no rounding: they EQUAL float64, and are
          the same bits under every slab target and both builds.  The backward's exact inputs put every pre-activation value
          at least 0.4 standard deviations from 0 (beta = gamma * rstd * (k + 1/2), x - mean an integer), so no sign is in doubt.
  real  : the inputs of test_gpu_bn_apply.make_case (x = 2 randn + 3, planted exact zeros in a beta = 0 channel).  Every sum S
          against the float64 sum S64 of the same per-element terms formed from the fp32 inputs:
              |S - S64| <= 128 * 2^-24 * sum |term64|                                                              (BAR)
          derived, not measured: a thread adds at most 64 rows one after the other (asserted per launch from the geometry
          rule), the tree in shared memory adds log2(TY) <= 8 levels, a term carries at most 5 roundings (subtract, rsqrt at
          2 ulp, two products) - about 77 units of 2^-24 against 128; the finalize adds the slab partials in double.
          mode 0: the terms are d = x - (first row of the group) and d^2; the kernel hands out mean and var, not the sums, so
              the bar of each sum is carried through the finalize's formulas mean = x_first + S1/n, var = S2/n - (S1/n)^2:
              |mean - mean64| <= BAR(S1)/n + 2^-24 |mean|,
              |var - var64|  <= BAR(S2)/n + 2 |S1/n| BAR(S1)/n + 2^-24 var  - a multiple of mean(d^2), NOT of var: that is
              what the cancellation of this algorithm is bounded by.  Mode 5 likewise around its pivot.
          mode 3: y (fp32) is an input: the reference recovers xhat = (act^-1(y) - beta) / gamma from y in float64; the bar gains
              4 * 2^-24 * sum |dz| |z| / |gamma| for the x100 un-scaling of negative outputs (rounded before the subtraction).
  Sign decisions that float64 does not settle for fp32 (|z64| <= 1e-6, not a planted zero; at most 1 % of a case, asserted)
  are taken out of the sums: dy is 0 on those elements.

Every output and workspace buffer ends in sentinel floats that must be unchanged after the call, the workspace is sized by
xas_bn_workspace_floats under the launch's own tuning flags, and every test puts xas_set_tuning(0) back in a finalizer.

Sizes: the shapes are the smallest that reach each branch of col_geom and of the finalize (SHAPES).  Two inputs are larger
than 16 MB because what they reach is not reachable below: (4000, 2048, 4) is 33 MB, and abs_max_kernel's unrolled loop runs
only once the 4096-block cap binds, from 3 * 4096 * 256 float4 = 48 MiB (test_abs_max)."""
import pytest
import torch

from xas_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = float(torch.tensor(1e-5, dtype=torch.float32))          # the float the kernels are handed
SENT, SENT_V, FILL = 16, -62500000.0, 1.5e30                   # sentinel floats behind every buffer; pre-fill of the outputs
SLABS = (('slab256', 0), ('slab512', _lib.TUNE_SLAB_512), ('slab128', _lib.TUNE_SLAB_128), ('slab64', _lib.TUNE_SLAB_64))
BUILDS = (('shipped', 0), ('lean', _lib.TUNE_COL_REDUCE_LEAN))
WANT = {0: 256, _lib.TUNE_SLAB_512: 512, _lib.TUNE_SLAB_128: 128, _lib.TUNE_SLAB_64: 64}
FORMS = ('xy', 'xm', 'y', 'x')                                # operands of xas_bn_bwd_reduce: modes 1, 1 + mask, 3, 4
DEV = 'cuda'
NEG = float(torch.tensor(0.01, dtype=torch.float32))          # the kernels' leaky slope

# (M rows, C channels, G groups) and what each reaches of col_geom and of the finalize:
SHAPES = [
    (1, 4, 1), (2, 4, 1), (255, 4, 1),      # CB = 4: one channel quadruple per block, 256 row lanes, fewer rows than lanes; Mg = 1
    (2049, 4, 1),                           # the 1 -> 2 slab boundary at TY * 8 rows
    (7, 24, 1), (300, 24, 2),               # CB = 8, three channel blocks, C/4 no power of two
    (129, 64, 1),                           # two slabs, the last one short
    (8200, 64, 1),                          # 65 slabs: the finalize's unrolled loads (> 4 * 16 slabs) AND its tail; last slab 72 rows
    (16384, 256, 1),                        # slab targets -> 64 / 128 / 32 / 16 slabs = 16 / 8 / 32 / 64 rows per thread
    (8193, 192, 3),                         # 3 groups, 3 channel blocks, short last slab
    (4000, 2048, 4),                        # 32 channel blocks, 4 groups, 4 / 8 / 2 / 1 slabs
    (192, 8, 64),                           # the 64-group limit, 3 rows per group
    (5, 260, 1),                            # 65 channel blocks of 4 channels
]
SHAPE_IDS = ['%dx%dx%d' % s for s in SHAPES]


@pytest.fixture(autouse=True)
def _tuning_back(request):
    request.addfinalizer(lambda: _lib.query('xas_set_tuning', 0))


# ------------------------------------------------------------------------------------------------ plumbing
def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def cdiv(a, b):
    return -(-a // b)


def geom(M, C, G, tune):
    """col_geom of csrc/bn.hip -> (TY, nslab, rows per thread at most)."""
    cb = 4
    while cb < 64 and C % (cb * 2) == 0:
        cb *= 2
    ty, ncb, Mg = 256 // (cb // 4), C // cb, M // G
    want = WANT[tune & (_lib.TUNE_SLAB_MASK << _lib.TUNE_SLAB_SHIFT)] * (2 if G > 1 else 1) // (ncb * G)
    want = max(1, min(want, cdiv(Mg, ty * 8)))
    rps = cdiv(Mg, want)
    return ty, cdiv(Mg, rps), cdiv(rps, ty)


class Buf:
    """n floats (pre-filled) followed by SENT sentinel floats."""

    def __init__(self, n, fill=FILL, src=None):
        self.n = n
        self.all = torch.full((n + SENT,), fill, device=DEV)
        self.all[n:] = SENT_V
        if src is not None:
            self.all[:n] = src.reshape(-1).float()
        self.t = self.all[:n]

    def ptr(self, off=0):
        return self.all.data_ptr() + 4 * off

    def intact(self):
        assert bool((self.all[self.n:] == SENT_V).all()), 'floats behind a buffer of %d were written' % self.n


def workspace(M, C, G, tune):
    """Sized under the launch's own flags (the geometry depends on them)."""
    _lib.query('xas_set_tuning', tune)
    n = _lib.query('xas_bn_workspace_floats', M, C, G)
    _lib.query('xas_set_tuning', 0)
    assert n > 0 and geom(M, C, G, tune)[2] <= 64, 'a thread would add more than 64 rows: the bar is derived for 64'
    assert n == G * geom(M, C, G, tune)[1] * 2 * C + C
    return Buf(n)


def launch(tune, name, *args):
    _lib.query('xas_set_tuning', tune)
    try:
        _lib.call(name, *args)
    finally:
        _lib.query('xas_set_tuning', 0)
    torch.cuda.synchronize()


def P(t):
    return None if t is None else t.data_ptr()


class StatOut:
    """mean / var [G][C] dense, or the message form mean | var | count | 3 padding floats (out_stride = 2C + 4)."""
    PAD = 4.25e9

    def __init__(self, G, C, message):
        self.G, self.C, self.message = G, C, message
        if message:
            self.stride = 2 * C + 4
            self.msg = Buf(G * self.stride, fill=self.PAD)
            self.args = (self.msg.ptr(0), self.msg.ptr(C), self.stride, self.msg.ptr(2 * C))
        else:
            self.stride = C
            self.m, self.v = Buf(G * C), Buf(G * C)
            self.args = (self.m.ptr(), self.v.ptr(), C, None)

    def read(self, count):
        G, C = self.G, self.C
        if not self.message:
            self.m.intact(), self.v.intact()
            return self.m.t.view(G, C).clone(), self.v.t.view(G, C).clone()
        self.msg.intact()
        m = self.msg.t.view(G, self.stride)
        assert bool((m[:, 2 * C + 1:] == self.PAD).all()), 'padding floats of the message were written'
        assert bool((m[:, 2 * C] == float(count)).all()), 'count slot'
        return m[:, :C].clone(), m[:, C:2 * C].clone()


def running_bufs(running, C):
    return (None, None) if running is None else (Buf(C, src=running[0]), Buf(C, src=running[1]))


def run_stats(x, M, C, G, tune=0, running=None, momentum=0.1, count=None, message=False):
    """mode 0 -> mean, var [G][C] (, running mean, running var)."""
    ws, out = workspace(M, C, G, tune), StatOut(G, C, message)
    rm, rv = running_bufs(running, C)
    pm, pv, st, pc = out.args
    launch(tune, 'xas_bn_stats', P(x), M, C, G, pm, pv, st, pc, ws.ptr(), rm and rm.ptr(), rv and rv.ptr(), momentum,
           M // G if count is None else count)
    ws.intact()
    res = out.read(M // G)
    if running is not None:
        rm.intact(), rv.intact()
        res += (rm.t.clone(), rv.t.clone())
    return res


def run_stats_partials(part, rows, C, G, rows_real, pivot, tune=0, running=None, momentum=0.1, message=False):
    """mode 5: part [rows][C][2] -> mean, var [G][C] (, running)."""
    ws, out = workspace(rows, 2 * C, G, tune), StatOut(G, C, message)
    rm, rv = running_bufs(running, C)
    pm, pv, st, pc = out.args
    launch(tune, 'xas_bn_stats_from_partials', P(part), rows, C, G, rows_real, P(pivot), pm, pv, st, pc, ws.ptr(),
           rm and rm.ptr(), rv and rv.ptr(), momentum)
    ws.intact()
    res = out.read(rows_real)
    if running is not None:
        rm.intact(), rv.intact()
        res += (rm.t.clone(), rv.t.clone())
    return res


def run_sums_partials(part, rows, C, G, tune=0, acc=None):
    """mode 6: part [rows][2][C] -> sums [G][2][C] (, dbeta, dgamma)."""
    ws, sums = workspace(rows, 2 * C, G, tune), Buf(G * 2 * C)
    a1, a2 = running_bufs(acc, C)
    launch(tune, 'xas_bn_bwd_sums_from_partials', P(part), rows, C, G, sums.ptr(), ws.ptr(), a1 and a1.ptr(), a2 and a2.ptr())
    ws.intact(), sums.intact()
    res = (sums.t.view(G, 2, C).clone(),)
    if acc is not None:
        a1.intact(), a2.intact()
        res += (a1.t.clone(), a2.t.clone())
    return res if acc is not None else res[0]


def run_col_sum(x, M, C, tune=0):
    ws, out = workspace(M, C, 1, tune), Buf(C)
    launch(tune, 'xas_col_sum', P(x), M, C, out.ptr(), ws.ptr())
    ws.intact(), out.intact()
    return out.t.clone()


def run_col_sum_acc(x, M, C, acc, tune=0):
    """acc: a Buf, added to in place."""
    ws = workspace(M, C, 1, tune)
    launch(tune, 'xas_col_sum_acc', P(x), M, C, acc.ptr(), ws.ptr())
    ws.intact(), acc.intact()
    return acc.t.clone()


def run_bwd(c, form, tune=0, acc=None):
    """xas_bn_bwd_reduce on the operands `form` names -> sums [G][2][C] (, dbeta, dgamma)."""
    M, C, G = c['M'], c['C'], c['G']
    ws, sums = workspace(M, C, G, tune), Buf(G * 2 * C)
    a1, a2 = running_bufs(acc, C)
    x = c['x'] if form[0] == 'x' else None
    y = c['y'] if 'y' in form else None
    mask = c['mask'] if 'm' in form else None
    launch(tune, 'xas_bn_bwd_reduce', P(x), P(y), P(c['dy']), P(c['mean']), P(c['var']), P(c['gam']), P(c['bet']), EPS, c['act'],
           M, C, G, sums.ptr(), ws.ptr(), a1 and a1.ptr(), a2 and a2.ptr(), P(mask))
    ws.intact(), sums.intact()
    s = sums.t.view(G, 2, C).clone()
    if acc is None:
        return s
    a1.intact(), a2.intact()
    return s, a1.t.clone(), a2.t.clone()


# ------------------------------------------------------------------------------------------------ inputs and float64
def pack_signs(pos):
    """[rows, C] bool -> one byte per float4, bit e = lane e."""
    p = pos.reshape(pos.shape[0], -1, 4).to(torch.uint8)
    return (p[..., 0] | (p[..., 1] << 1) | (p[..., 2] << 2) | (p[..., 3] << 3)).reshape(-1).contiguous()


def act_f64(z, act):
    return z if act == 0 else (z.clamp(min=0) if act == 1 else torch.where(z > 0, z, 0.01 * z))


def grp_sum(t, G):
    return t.view(G, -1, t.shape[-1]).sum(1)


def finish_case(c):
    """z (float64, from the fp32 inputs), y, sign bytes; doubtful signs -> dy = 0 there (module docstring)."""
    G, Mg, C = c['G'], c['Mg'], c['C']
    m, v = c['mean'].double().repeat_interleave(Mg, 0), c['var'].double().repeat_interleave(Mg, 0)
    c['xhat'] = (c['x'].double() - m) * torch.rsqrt(v + EPS)
    z = c['xhat'] * c['gam'].double() + c['bet'].double()
    planted = c.get('planted')
    if planted is None:
        planted = torch.zeros_like(z, dtype=torch.bool)
    assert bool((z[planted] == 0).all())
    d = (z.abs() <= 1e-6) & ~planted
    assert int(d.sum()) <= 0.01 * d.numel(), '%d of %d pre-activation values within 1e-6 of 0' % (int(d.sum()), d.numel())
    c['dy'][d] = 0.
    c['doubtful'] = int(d.sum())
    c['z'], c['pos'] = z, z > 0
    c['y'] = act_f64(z, c['act']).float()
    c['mask'] = pack_signs(c['pos'])
    return c


def real_case(M, C, G, act, seed, gam=None):
    """make_case of test_gpu_bn_apply (same recipe; the planted rows are clamped for groups of fewer than 5 rows)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, C, generator=g, device=DEV) * 2 + 3
    dy = torch.randn(M, C, generator=g, device=DEV)
    gm = torch.rand(C, generator=g, device=DEV) + 0.5 if gam is None else gam.to(DEV)
    bet = torch.randn(C, generator=g, device=DEV)
    bet[2] = 0.
    Mg = M // G
    xg = x.view(G, Mg, C)
    mean = xg.double().mean(1).float()
    var = xg.double().var(1, unbiased=False).float()
    rows = torch.tensor(sorted({0, min(1, Mg - 1), Mg // 2, max(Mg - 2, 0), Mg - 1}), device=DEV)
    planted = torch.zeros(M, C, dtype=torch.bool, device=DEV)
    for k in range(G):
        xg[k][rows, 2] = mean[k, 2]
        planted.view(G, Mg, C)[k][rows, 2] = True
    return finish_case(dict(M=M, C=C, G=G, Mg=Mg, act=act, x=x, dy=dy, gam=gm, bet=bet, mean=mean, var=var, planted=planted))


def exact_case(M, C, G, act, seed):
    """Integers: x = mean_g + D, |D| <= 16, dy a non-zero integer in [-8, 8]; beta puts the sign change of channel c at
    D = -(k_c + 1/2) (the groups' rstd differ by at most 2 %: the change stays between two integers for every group)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    Mg = M // G
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=DEV)
    mean = (ri(-1000, 1000, 1, C) + 7 * torch.arange(G, device=DEV).view(G, 1)).float()
    D = ri(-16, 16, M, C)
    x = (mean.repeat_interleave(Mg, 0) + D).float()
    dy = (ri(1, 8, M, C) * (2 * ri(0, 1, M, C) - 1)).float()
    v0 = torch.rand(1, C, generator=g, device=DEV) + 0.5
    var = (v0 * (1 + 0.02 * (torch.rand(G, C, generator=g, device=DEV) - 0.5))).float()
    gam = (torch.rand(C, generator=g, device=DEV) + 0.5) * (2 * ri(0, 1, C) - 1).float()
    k = ri(-3, 3, C).double() + 0.5
    bet = (gam.double() * torch.rsqrt(v0[0].double() + EPS) * k).float()
    c = finish_case(dict(M=M, C=C, G=G, Mg=Mg, act=act, x=x, dy=dy, gam=gam, bet=bet, mean=mean, var=var))
    assert c['doubtful'] == 0 and float(c['z'].abs().min()) > 0.1
    return c


def sign_of(c, form):
    """The sign the launch is handed: y > 0 of the fp32 y, the mask bits, or (y-free) the float64 decision."""
    return c['y'] > 0 if 'y' in form else c['pos']


def bwd_terms(c, form):
    """float64 per-element terms dz, dz * xhat (mode 3: xhat recovered from the fp32 y) and the mode-3 extra bar term."""
    act = c['act']
    one = torch.ones((), dtype=torch.float64, device=DEV)
    dz = c['dy'].double() * torch.where(sign_of(c, form), one, one * {1: 0., 2: NEG}[act]) if act else c['dy'].double()
    extra = None
    if form == 'y':
        y = c['y'].double()
        z = torch.where(y > 0, y, y * (0. if act == 1 else 100.))
        g = c['gam'].double()
        ok = g != 0
        xh = torch.where(ok, (z - c['bet'].double()) / torch.where(ok, g, torch.ones_like(g)), torch.zeros_like(z))
        extra = torch.where(ok, dz.abs() * z.abs() / torch.where(ok, g.abs(), torch.ones_like(g)), torch.zeros_like(z))
    else:
        xh = c['xhat']
    return dz, dz * xh, extra


def ratio(err, bar):
    """max err / bar; a zero bar demands a zero error."""
    r = torch.where(bar > 0, err / torch.where(bar > 0, bar, torch.ones_like(bar)), torch.where(err > 0, float('inf'), 0.).to(err))
    return float(r.max())


def sum_ratio(S, t, G, extra=None):
    """Kernel sums S [G][C] against the float64 sum of terms t [M][C] -> error / BAR, worst channel."""
    bar = 128 * U * grp_sum(t.abs(), G)
    if extra is not None:
        bar = bar + 4 * U * grp_sum(extra, G)
    return ratio((S.double() - grp_sum(t, G)).abs(), bar)


def stat_ratios(mean, var, piv, s1, a1, s2, n):
    """mean / var from sums around `piv` (float64 [G][C]: s1 = sum d, a1 = sum |d|, s2 = sum d^2 (terms >= 0), n rows) ->
    error / bar of mean and of var (module docstring, mode 0)."""
    m = s1 / n
    mean64, var64 = piv + m, (s2 / n - m * m).clamp(min=0)
    b1 = 128 * U * a1 / n
    r_mean = ratio((mean.double() - mean64).abs(), b1 + U * mean64.abs())
    r_var = ratio((var.double() - var64).abs(), 128 * U * s2 / n + 2 * m.abs() * b1 + U * var64)
    return r_mean, r_var


def assert_exact(t, G):
    """Every fp32 partial sum of the integer terms t is an integer below 2^24."""
    assert bool((t == t.round()).all()) and float(grp_sum(t.abs(), G).max()) < 2 ** 24


def partials_stats(M, C, G, t, pivot_off, seed, exact):
    """Mode-5 input: activations v [M * t][C] (M partial rows, each over t activation rows), pivot p -> part [M][C][2] in
    float64 -> fp32, with the float64 v.  exact: v - p integers, |v - p| <= 16."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if exact:
        d = torch.randint(-16, 17, (M * t, C), generator=g, device=DEV).double()
        p = torch.randint(-500, 501, (C,), generator=g, device=DEV).double() if pivot_off else torch.zeros(C, device=DEV, dtype=torch.float64)
    else:
        p = (torch.randn(C, generator=g, device=DEV) + 3).float().double() if pivot_off else torch.zeros(C, device=DEV, dtype=torch.float64)
        d = (torch.randn(M * t, C, generator=g, device=DEV) * 2 + 3).double() - p
    part = torch.stack([d.view(M, t, C).sum(1), (d * d).view(M, t, C).sum(1)], dim=2)        # [M][C][2]
    return part.float().contiguous(), p, d


REPORT = {}


def report(key, r):
    REPORT[key] = max(REPORT.get(key, 0.), r)
    print('RATIO %-28s %.4f (largest so far %.4f)' % (key, r, REPORT[key]))


# ------------------------------------------------------------------------------------------------ exact cases
def p56_channels(C):
    """Modes 5 / 6 reduce a matrix of 2 x channels columns: C columns where C / 2 channels are allowed, else C channels."""
    return C // 2 if C % 8 == 0 else C


@pytest.mark.parametrize('M,C,G', SHAPES, ids=SHAPE_IDS)
def test_exact_sums(M, C, G):
    """Modes 2 and 6 and sum dz of modes 1 / 3 / 4 under ReLU on integers: EQUAL to float64, same bits under every flag."""
    c = exact_case(M, C, G, 1, seed=M + C)
    assert_exact(c['dy'].double(), G)
    for form in FORMS:
        dz, _, _ = bwd_terms(c, form)
        want = grp_sum(dz, G)
        outs = [run_bwd(c, form, slab | build) for _, slab in SLABS for _, build in BUILDS]
        for s in outs:
            assert torch.equal(s[:, 0].double(), want), form
            assert same_bits(s[:, 0], outs[0][:, 0]) and bool(torch.isfinite(s).all()), form
    # mode 2 has no groups: the rows of group 0
    x = c['dy'][:c['Mg']]
    assert_exact(x.double(), 1)
    for _, slab in SLABS:
        assert torch.equal(run_col_sum(x, c['Mg'], C, slab).double(), x.double().sum(0))
    # mode 6: integer partials [M][2][Ch]
    Ch = p56_channels(C)
    part = torch.randint(-8, 9, (M, 2 * Ch), generator=torch.Generator(device=DEV).manual_seed(C), device=DEV).float()
    assert_exact(part.double(), G)
    want = grp_sum(part.double(), G).view(G, 2, Ch)
    for _, slab in SLABS:
        assert torch.equal(run_sums_partials(part, M, Ch, G, slab).double(), want)


@pytest.mark.parametrize('M,C,G', SHAPES, ids=SHAPE_IDS)
def test_exact_stats(M, C, G):
    """Mode 0 on x = integer pivot row + integer deviations: mean EQUALS the float64 mean rounded to fp32, var within 1 ulp,
    same bits under every slab target, dense and message form.  Mode 5 on integer partials, pivot NULL and given."""
    c = exact_case(M, C, G, 0, seed=3 * M + C)
    x, Mg = c['x'], c['Mg']
    xg = x.double().view(G, Mg, C)
    d = (xg - xg[:, :1]).reshape(M, C)
    assert_exact(d, G), assert_exact(d * d, G)
    mean64, var64 = xg.mean(1), xg.var(1, unbiased=False)
    ulp = lambda v: torch.maximum(2 * U * v.abs(), torch.full_like(v, 2.0 ** -149))
    first = None
    for _, slab in SLABS:
        for message in (False, True):
            mean, var = run_stats(x, M, C, G, slab, message=message)
            assert torch.equal(mean, mean64.float())
            assert bool(((var.double() - var64).abs() <= ulp(var64)).all())
            first = first or (mean, var)
            assert same_bits(mean, first[0]) and same_bits(var, first[1])
    Ch = p56_channels(C)
    for pivot_off in (False, True):
        part, p, dv = partials_stats(M, Ch, G, 2, pivot_off, seed=M + 7, exact=True)
        assert_exact(part.double().view(M, 2 * Ch), G)
        v = (dv + p).view(G, -1, Ch)
        mean64, var64 = v.mean(1), v.var(1, unbiased=False)
        first = None
        for _, slab in SLABS:
            mean, var = run_stats_partials(part, M, Ch, G, 2 * Mg, p.float() if pivot_off else None, slab, message=slab != 0)
            assert torch.equal(mean, mean64.float())
            assert bool(((var.double() - var64).abs() <= ulp(var64)).all())
            first = first or (mean, var)
            assert same_bits(mean, first[0]) and same_bits(var, first[1])


@pytest.mark.parametrize('rows_g', [1, 3, 40])
@pytest.mark.parametrize('G', [1, 3])
def test_exact_stats_from_partials_rows(rows_g, G):
    """Mode 5 with 1, 3 and 40 partial rows per group of 5 activation rows each: rows_per_group is NOT rows / groups."""
    Ch, t = 12, 5
    rows = rows_g * G
    for pivot_off in (False, True):
        part, p, dv = partials_stats(rows, Ch, G, t, pivot_off, seed=rows, exact=True)
        assert_exact(part.double().view(rows, 2 * Ch), G)
        v = (dv + p).view(G, -1, Ch)
        mean64, var64 = v.mean(1), v.var(1, unbiased=False)
        rm0, rv0 = torch.linspace(-1, 1, Ch, device=DEV), torch.linspace(0.5, 2, Ch, device=DEV)
        mean, var, rm, rv = run_stats_partials(part, rows, Ch, G, rows_g * t, p.float() if pivot_off else None, running=(rm0, rv0),
                                               momentum=0.1, message=True)
        assert torch.equal(mean, mean64.float())
        assert bool(((var.double() - var64).abs() <= 2 * U * var64).all())
        n = rows_g * t
        rm64, rv64, bm, bv = rm0.double(), rv0.double(), 0., 0.
        for k in range(G):                                     # 4 roundings per update at most
            bm, bv = bm + 4 * U * (rm64.abs() + mean64[k].abs()), bv + 4 * U * (rv64.abs() + var64[k] * n / (n - 1))
            rm64, rv64 = 0.9 * rm64 + 0.1 * mean64[k], 0.9 * rv64 + 0.1 * var64[k] * n / (n - 1)
        mo = float(torch.tensor(0.1, dtype=torch.float32))
        bm, bv = bm + abs(mo - 0.1) * 40, bv + abs(mo - 0.1) * 400          # momentum is handed over as a float
        assert bool(((rm.double() - rm64).abs() <= bm).all()) and bool(((rv.double() - rv64).abs() <= bv).all())


# ------------------------------------------------------------------------------------------------ real-valued cases
@pytest.mark.parametrize('act', [1, 2], ids=['relu', 'leaky'])
@pytest.mark.parametrize('M,C,G', SHAPES, ids=SHAPE_IDS)
def test_real_backward_sums(M, C, G, act):
    """Modes 1 (y and mask), 3 and 4 on real values, four slab targets x two builds, against the bar."""
    c = real_case(M, C, G, act, seed=11 * M + C + act)
    lean_same = True
    for form in FORMS:
        dz, dzx, extra = bwd_terms(c, form)
        for _, slab in SLABS:
            outs = [run_bwd(c, form, slab | build) for _, build in BUILDS]
            for s in outs:
                r1, r2 = sum_ratio(s[:, 0], dz, G), sum_ratio(s[:, 1], dzx, G, extra)
                mode = {'xy': '1', 'xm': '1 (mask)', 'y': '3', 'x': '4'}[form]
                report('mode%s sum_dz' % mode, r1), report('mode%s sum_dz_xhat' % mode, r2)
                assert r1 <= 1 and r2 <= 1, form
            lean_same &= same_bits(outs[0], outs[1])
    print('LEAN_BIT_IDENTICAL %s %s' % ((M, C, G, act), lean_same))


@pytest.mark.parametrize('bad_pivot', [False, True], ids=['pivot_typical', 'pivot_50_sigma'])
@pytest.mark.parametrize('M,C,G', SHAPES, ids=SHAPE_IDS)
def test_real_stats(M, C, G, bad_pivot):
    """Modes 0, 2, 5, 6 on real values.  bad pivot: the first row of every group lies 50 sigma from the channel means."""
    c = real_case(M, C, G, 0, seed=5 * M + C)
    x, Mg = c['x'], c['Mg']
    if bad_pivot:
        x.view(G, Mg, C)[:, 0] += 100.
    xg = x.double().view(G, Mg, C)
    d = (xg - xg[:, :1])
    for _, slab in SLABS:
        mean, var = run_stats(x, M, C, G, slab, message=slab == 0)
        rm, rv = stat_ratios(mean, var, xg[:, 0], d.sum(1), d.abs().sum(1), (d * d).sum(1), Mg)
        report('mode0 mean', rm), report('mode0 var', rv)
        assert rm <= 1 and rv <= 1
        if Mg == 1:
            assert torch.equal(mean, x.view(G, C)) and bool((var == 0).all())
    if bad_pivot:
        return
    for _, slab in SLABS:                                        # mode 2 has no groups: the rows of group 0
        r = sum_ratio(run_col_sum(x, Mg, C, slab).view(1, C), x[:Mg].double(), 1)
        report('mode2 sum', r)
        assert r <= 1
    Ch = p56_channels(C)
    for pivot_off in (False, True):
        part, p, dv = partials_stats(M, Ch, G, 2, pivot_off, seed=M + 9, exact=False)
        pd = part.double().view(G, Mg, Ch, 2)
        for _, slab in SLABS:
            mean, var = run_stats_partials(part, M, Ch, G, 2 * Mg, p.float() if pivot_off else None, slab)
            rm, rv = stat_ratios(mean, var, p, pd[..., 0].sum(1), pd[..., 0].abs().sum(1), pd[..., 1].sum(1), 2 * Mg)
            report('mode5 mean', rm), report('mode5 var', rv)
            assert rm <= 1 and rv <= 1
    part = torch.randn(M, 2 * Ch, generator=torch.Generator(device=DEV).manual_seed(M), device=DEV)
    for _, slab in SLABS:
        s = run_sums_partials(part, M, Ch, G, slab)
        r = sum_ratio(s.view(G, 2 * Ch), part.double(), G)
        report('mode6 sum', r)
        assert r <= 1


# ------------------------------------------------------------------------------------------------ the x-free form at small gamma
def test_x_free_form_at_small_gamma():
    """Mode 3, leaky ReLU, beta ~ N(0, 1), whole channels at gamma = 1, 1e-2, 1e-4 and one at gamma = 0.  Asserted: the mode-3
    bar with xhat recovered from y in float64.  gamma = 0: the x-free form cannot know xhat - sum dz xhat is 0, sum dz is right,
    nothing is non-finite.  Printed, not asserted: the distance of sum dz xhat from the float64 value computed FROM X, relative
    to sum |dz xhat| (what the physique net's dgamma is worth when a gamma shrinks).  Measured on an MI355X (largest / median
    channel): gamma 1: 4.2e-9 / 1.4e-9; gamma 1e-2: 1.1e-7 / 2.2e-8; gamma 1e-4: 4.9e-6 / 1.4e-6 - the error grows as 1 / gamma
    (y carries z = gamma xhat + beta at the precision of |beta|); relative to the sum itself 2.9e-6, 5.4e-5, 7.9e-4 at most."""
    M, C, G = 8200, 64, 1
    gam = torch.tensor([1., 1e-2, 1e-4])[torch.arange(C) % 3]
    gam[5] = 0.
    c = real_case(M, C, G, 2, seed=77, gam=gam)
    dz, dzx, extra = bwd_terms(c, 'y')
    from_x = grp_sum(dz * c['xhat'], G)
    scale = grp_sum((dz * c['xhat']).abs(), G)
    for _, slab in SLABS:
        for _, build in BUILDS:
            s = run_bwd(c, 'y', slab | build)
            assert bool(torch.isfinite(s).all())
            assert sum_ratio(s[:, 0], dz, G) <= 1 and sum_ratio(s[:, 1], dzx, G, extra) <= 1
            assert float(s[0, 1, 5]) == 0. and float(dzx[:, 5].abs().max()) == 0.
            report('mode3 small-gamma sum_dz_xhat', sum_ratio(s[:, 1], dzx, G, extra))
    s = run_bwd(c, 'y', 0)
    for gv in (1., 1e-2, 1e-4):
        ch = (c['gam'] == gv).nonzero().flatten()
        dist = ((s[0, 1].double() - from_x[0]).abs() / scale[0])[ch]
        rel = ((s[0, 1].double() - from_x[0]).abs() / from_x[0].abs())[ch]
        print('SMALL_GAMMA gamma %g: |S - S64(x)| / sum|dz xhat| max %.3e median %.3e ; / |S64(x)| max %.3e median %.3e' % (
            gv, float(dist.max()), float(dist.median()), float(rel.max()), float(rel.median())))


# ------------------------------------------------------------------------------------------------ cross-checks without a tolerance
@pytest.mark.parametrize('M,C,G', [(8200, 64, 1), (8193, 192, 3), (300, 24, 2)], ids=['8200x64x1', '8193x192x3', '300x24x2'])
def test_one_forward_three_sign_sources(M, C, G):
    """xas_bn_apply with mask_out on real x, integer non-zero dy: sum dz from the mask bytes, from y > 0 and re-derived from x
    are the same bits (an element the three disagree on changes an exact integer sum).  Leaky ReLU: sum dz is not exact,
    y against x under the bar."""
    for act in (1, 2):
        c = real_case(M, C, G, act, seed=M + act)
        g = torch.Generator(device=DEV).manual_seed(M)
        c['dy'] = (torch.randint(1, 9, (M, C), generator=g, device=DEV) * (2 * torch.randint(0, 2, (M, C), generator=g, device=DEV) - 1)).float()
        y, mask = Buf(M * C), torch.full((M * C // 4 + 64,), 0xa5, dtype=torch.uint8, device=DEV)
        res = torch.zeros(M, C, device=DEV)                      # (the sign bytes are written for layers WITH a residual: a zero one)
        launch(0, 'xas_bn_apply', P(c['x']), P(c['mean']), P(c['var']), P(c['gam']), P(c['bet']), P(res), EPS, act, M, C, G, y.ptr(),
               P(mask))
        y.intact()
        assert bool((mask[M * C // 4:] == 0xa5).all())
        c['y'], c['mask'] = y.t.view(M, C), mask
        assert_exact(c['dy'].double(), G)
        for _, slab in SLABS:
            for _, build in BUILDS:
                sy, sm, sx = (run_bwd(c, f, slab | build) for f in ('xy', 'xm', 'x'))
                if act == 1:
                    assert same_bits(sy[:, 0], sm[:, 0]) and same_bits(sy[:, 0], sx[:, 0])
                    assert torch.equal(sy[:, 0].double(), grp_sum(c['dy'].double() * (c['y'] > 0), G))
                else:
                    dz, _, _ = bwd_terms(c, 'xy')
                    assert sum_ratio(sy[:, 0], dz, G) <= 1 and sum_ratio(sx[:, 0], dz, G) <= 1 and sum_ratio(sm[:, 0], dz, G) <= 1


def rows_of(c, k):
    """Group k of a case as a one-group case."""
    Mg, C = c['Mg'], c['C']
    r = slice(k * Mg, (k + 1) * Mg)
    o = dict(c, M=Mg, G=1, x=c['x'][r].contiguous(), dy=c['dy'][r].contiguous(), y=c['y'][r].contiguous(),
             mean=c['mean'][k:k + 1].contiguous(), var=c['var'][k:k + 1].contiguous(),
             mask=c['mask'][k * Mg * C // 4:(k + 1) * Mg * C // 4].contiguous())
    return o


@pytest.mark.parametrize('M,C,G,kind', [(300, 24, 2, 'real'), (192, 8, 64, 'real'), (8193, 192, 3, 'exact'), (4000, 2048, 4, 'exact')],
                         ids=['300x24x2_real', '192x8x64_real', '8193x192x3_exact', '4000x2048x4_exact'])
def test_groups_equal_separate_launches(M, C, G, kind):
    """A G-group launch = G one-group launches on the row ranges, bit for bit: statistics, running statistics after the G
    updates in group order (modes 0 and 5), backward sums.  real: shapes with ONE slab per group in both launches (the same
    rows meet the same thread: every output, rounding included); exact: integers, where the split does not matter (the
    outputs without rounding: mean, var, sum dz)."""
    c = (real_case if kind == 'real' else exact_case)(M, C, G, 1, seed=M)
    Mg = c['Mg']
    if kind == 'real':
        assert geom(M, C, G, 0)[1] == 1 and geom(Mg, C, 1, 0)[1] == 1
    run0 = (torch.linspace(-2, 2, C, device=DEV), torch.linspace(0.5, 3, C, device=DEV))
    mean, var, rm, rv = run_stats(c['x'], M, C, G, running=run0, momentum=0.1)
    run = run0
    for k in range(G):
        m1, v1, r1, r2 = run_stats(c['x'][k * Mg:(k + 1) * Mg].contiguous(), Mg, C, 1, running=run, momentum=0.1)
        run = (r1, r2)
        assert same_bits(m1[0], mean[k]) and same_bits(v1[0], var[k])
    assert same_bits(run[0], rm) and same_bits(run[1], rv)
    for form in FORMS:
        s = run_bwd(c, form)
        for k in range(G):
            s1 = run_bwd(rows_of(c, k), form)
            assert same_bits(s1[0, 0], s[k, 0]), form
            if kind == 'real':
                assert same_bits(s1[0], s[k]), form
    # modes 5 and 6
    Ch = p56_channels(C)
    part, p, _ = partials_stats(M, Ch, G, 2, True, seed=M + 1, exact=kind == 'exact')
    run0 = (run0[0][:Ch].contiguous(), run0[1][:Ch].contiguous())
    mean, var, rm, rv = run_stats_partials(part, M, Ch, G, 2 * Mg, p.float(), running=run0)
    run = run0
    for k in range(G):
        m1, v1, r1, r2 = run_stats_partials(part[k * Mg:(k + 1) * Mg].contiguous(), Mg, Ch, 1, 2 * Mg, p.float(), running=run)
        run = (r1, r2)
        assert same_bits(m1[0], mean[k]) and same_bits(v1[0], var[k])
    assert same_bits(run[0], rm) and same_bits(run[1], rv)
    part6 = part.view(M, 2 * Ch) if kind == 'real' else torch.randint(-8, 9, (M, 2 * Ch), device=DEV,
                                                                    generator=torch.Generator(device=DEV).manual_seed(3)).float()
    s = run_sums_partials(part6, M, Ch, G)
    for k in range(G):
        assert same_bits(run_sums_partials(part6[k * Mg:(k + 1) * Mg].contiguous(), Mg, Ch, 1)[0], s[k])


@pytest.mark.parametrize('M,C,G', [(300, 24, 2), (8193, 192, 3), (192, 8, 64)], ids=['300x24x2', '8193x192x3', '192x8x64'])
def test_accumulators(M, C, G):
    """dbeta_acc / dgamma_acc start non-zero and end at start + sum over groups of `sums` (one fp32 rounding per group added);
    a NULL pair leaves `sums` the same bits; mode 6 sends the first half of the columns to dbeta, the second to dgamma;
    xas_col_sum_acc twice adds twice."""
    c = real_case(M, C, G, 1, seed=M + 2)
    a0 = (torch.linspace(-3, 3, C, device=DEV), torch.linspace(5, -5, C, device=DEV))
    for form in FORMS:
        for _, build in BUILDS:
            s, a1, a2 = run_bwd(c, form, build, acc=a0)
            assert same_bits(s, run_bwd(c, form, build)), form
            for k, a in enumerate((a1, a2)):
                want = a0[k].double() + s[:, k].double().sum(0)
                assert bool(((a.double() - want).abs() <= U * G * (a0[k].abs() + s[:, k].abs().sum(0)).double()).all()), form
    Ch = p56_channels(C)
    part = torch.randn(M, 2 * Ch, generator=torch.Generator(device=DEV).manual_seed(M), device=DEV)
    part[:, Ch:] += 10.                                          # the two halves cannot be taken for one another
    a0 = (a0[0][:Ch].contiguous(), a0[1][:Ch].contiguous())
    s, a1, a2 = run_sums_partials(part, M, Ch, G, acc=a0)
    assert same_bits(s, run_sums_partials(part, M, Ch, G))
    for k, a in enumerate((a1, a2)):
        want = a0[k].double() + s[:, k].double().sum(0)
        assert bool(((a.double() - want).abs() <= U * G * (a0[k].abs() + s[:, k].abs().sum(0)).double()).all())
    xi = torch.randint(-8, 9, (M, C), generator=torch.Generator(device=DEV).manual_seed(1), device=DEV).float()
    acc = Buf(C, src=torch.arange(C, device=DEV) - 7.)
    once = run_col_sum_acc(xi, M, C, acc)
    twice = run_col_sum_acc(xi, M, C, acc)
    S = xi.double().sum(0)
    start = (torch.arange(C, device=DEV) - 7.).double()
    assert torch.equal(once.double(), start + S) and torch.equal(twice.double(), start + 2 * S)


@pytest.mark.parametrize('M,C,G', [(8200, 64, 1), (8193, 192, 3)], ids=['8200x64x1', '8193x192x3'])
def test_reproducible(M, C, G):
    """Every mode, 20 repeats: which block arrives last varies, the result may not."""
    c = real_case(M, C, G, 2, seed=M + 3)
    Ch = p56_channels(C)
    part, p, _ = partials_stats(M, Ch, G, 2, True, seed=M, exact=False)
    run0 = (torch.linspace(-2, 2, C, device=DEV), torch.linspace(0.5, 3, C, device=DEV))
    a0 = (torch.linspace(-3, 3, C, device=DEV), torch.linspace(5, -5, C, device=DEV))
    runs = {'mode0': lambda: run_stats(c['x'], M, C, G, running=run0, message=True),
            'mode2': lambda: (run_col_sum(c['x'], M, C),),
            'mode5': lambda: run_stats_partials(part, M, Ch, G, 2 * c['Mg'], p.float(), running=(run0[0][:Ch].contiguous(), run0[1][:Ch].contiguous())),
            'mode6': lambda: run_sums_partials(part.view(M, 2 * Ch), M, Ch, G, acc=(a0[0][:Ch].contiguous(), a0[1][:Ch].contiguous()))}
    for form in FORMS:
        for bname, build in BUILDS:
            runs['bwd_%s_%s' % (form, bname)] = lambda form=form, build=build: run_bwd(c, form, build, acc=a0)
    for name, f in runs.items():
        first = f()
        for _ in range(19):
            assert all(same_bits(a, b) for a, b in zip(f(), first)), name


def test_ticket_pool_wraps():
    """1 100 xas_col_sum launches of 65 ticket words each (the 65 536-word pool wraps after 1 008) with a 3-group xas_bn_stats
    every 50 launches: every result the bits of the first of its kind."""
    M, C = 5, 260
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, C, generator=g, device=DEV)
    M2, C2, G2 = 8193, 192, 3
    x2 = torch.randn(M2, C2, generator=g, device=DEV) * 2 + 3
    N = 1100
    ws, out = workspace(M, C, 1, 0), Buf(N * C)
    ws2, m2, v2 = workspace(M2, C2, G2, 0), Buf((N // 50) * G2 * C2), Buf((N // 50) * G2 * C2)
    for i in range(N):
        _lib.call('xas_col_sum', P(x), M, C, out.ptr(i * C), ws.ptr())
        if i % 50 == 49:
            j = i // 50
            _lib.call('xas_bn_stats', P(x2), M2, C2, G2, m2.ptr(j * G2 * C2), v2.ptr(j * G2 * C2), C2, None, ws2.ptr(), None, None, 0.1, M2 // G2)
    torch.cuda.synchronize()
    for b in (ws, out, ws2, m2, v2):
        b.intact()
    o = out.t.view(N, C)
    assert torch.equal(bits(o), bits(o[:1]).expand(N, C))
    assert sum_ratio(o[:1], x.double(), 1) <= 1
    for b in (m2, v2):
        t = b.t.view(N // 50, G2 * C2)
        assert torch.equal(bits(t), bits(t[:1]).expand_as(t))
    xg = x2.double().view(G2, -1, C2)
    d = xg - xg[:, :1]
    rm, rv = stat_ratios(m2.t.view(-1, G2, C2)[0], v2.t.view(-1, G2, C2)[0], xg[:, 0], d.sum(1), d.abs().sum(1), (d * d).sum(1), M2 // G2)
    assert rm <= 1 and rv <= 1


@pytest.mark.parametrize('M,C,G', [(8200, 64, 1), (300, 24, 2)], ids=['8200x64x1', '300x24x2'])
def test_non_finite_stays_in_its_channel(M, C, G):
    """One NaN in dy (modes 1 / 3 / 4) or x (modes 0 / 2): both outputs of that channel (of that group) are NaN, every other
    one the bits of the clean run.  The guarded optimizer's non-finite skip depends on it."""
    c = real_case(M, C, G, 2, seed=M + 4)
    r, ch, k = c['Mg'] + 1 if G > 1 else M // 2 + 1, 9, 1 if G > 1 else 0

    def check(clean, dirty, name):
        for a, b in zip(clean, dirty):                           # a, b: [G][C] (or [C] for the one-group column sum)
            a, b = a.view(-1, C), b.view(-1, C)
            assert bool(torch.isnan(b[k, ch])), name
            keep = torch.ones_like(a, dtype=torch.bool)
            keep[k, ch] = False
            assert torch.equal(bits(a)[keep], bits(b)[keep]), name

    for form in FORMS:
        for _, build in BUILDS:
            clean = run_bwd(c, form, build)
            d = dict(c, dy=c['dy'].clone())
            d['dy'][r, ch] = float('nan')
            dirty = run_bwd(d, form, build)
            check((clean[:, 0], clean[:, 1]), (dirty[:, 0], dirty[:, 1]), form)
    xn = c['x'].clone()
    xn[r, ch] = float('nan')
    check(run_stats(c['x'], M, C, G), run_stats(xn, M, C, G), 'mode0')
    k = 0
    check((run_col_sum(c['x'], M, C),), (run_col_sum(xn, M, C),), 'mode2')


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections_launch_nothing():
    """Status 1, and outputs pre-filled with a sentinel stay unchanged."""
    M, C, G = 300, 24, 2
    x = torch.randn(M, C, device=DEV)
    bufs = {n: Buf(G * (2 * C + 4)) for n in ('mean', 'var', 'ws', 'rm', 'rv', 'sums', 'a1', 'a2')}
    bufs['ws'] = Buf(4 * M * C)
    b = {n: v.ptr() for n, v in bufs.items()}
    st = _lib.stream()

    def stats(M=M, C=C, G=G, mean=b['mean'], stride=C, rm=b['rm'], rv=b['rv']):
        return _lib.fn('xas_bn_stats')(P(x), M, C, G, mean, b['var'], stride, None, b['ws'], rm, rv, 0.1, max(1, M // max(G, 1)), st)

    def bwd(M=M, C=C, G=G, a1=b['a1'], a2=b['a2']):
        return _lib.fn('xas_bn_bwd_reduce')(P(x), P(x), P(x), b['mean'], b['var'], b['rm'], b['rv'], EPS, 1, M, C, G, b['sums'], b['ws'],
                                            a1, a2, None, st)

    def part6(M=M, C=C // 2, G=G, a1=b['a1'], a2=b['a2']):
        return _lib.fn('xas_bn_bwd_sums_from_partials')(P(x), M, C, G, b['sums'], b['ws'], a1, a2, st)

    def part5(M=M, C=C // 2, G=G, rm=b['rm'], rv=b['rv'], stride=C // 2):
        return _lib.fn('xas_bn_stats_from_partials')(P(x), M, C, G, 2 * M // max(G, 1), None, b['mean'], b['var'], stride, None, b['ws'],
                                                     rm, rv, 0.1, st)

    assert stats() == 0 and bwd() == 0 and part6() == 0 and part5() == 0             # the accepted forms of the calls below
    torch.cuda.synchronize()
    for v in bufs.values():
        v.all[:v.n] = FILL
    torch.cuda.synchronize()
    cases = {
        'C=6': lambda: (stats(C=6), bwd(C=6), part6(C=6), part5(C=6, stride=8), _lib.fn('xas_col_sum')(P(x), M, 6, b['sums'], b['ws'], st),
                        _lib.fn('xas_col_sum_acc')(P(x), M, 6, b['sums'], b['ws'], st)),
        'C=0': lambda: (stats(C=0), bwd(C=0), part6(C=0), part5(C=0), _lib.fn('xas_col_sum')(P(x), M, 0, b['sums'], b['ws'], st)),
        'G=65': lambda: (stats(M=260, G=65), bwd(M=260, G=65), part6(M=260, G=65), part5(M=260, G=65)),
        'M % G != 0': lambda: (stats(G=7), bwd(G=7), part6(G=7), part5(G=7)),
        'misaligned mean': lambda: (stats(mean=b['mean'] + 4), stats(mean=b['mean'] + 8)),
        'out_stride % 4 != 0': lambda: (stats(stride=C + 2), part5(stride=C // 2 + 2)),
        'half a pointer pair': lambda: (stats(rm=None), stats(rv=None), bwd(a1=None), bwd(a2=None), part6(a1=None), part6(a2=None),
                                        part5(rm=None), part5(rv=None)),
    }
    for name, f in cases.items():
        rcs = f()
        torch.cuda.synchronize()
        assert all(rc == 1 for rc in rcs), '%s: status %s' % (name, rcs)
        for n, v in bufs.items():
            v.intact()
            assert bool((v.t == FILL).all()), '%s wrote %s' % (name, n)
    assert _lib.query('xas_bn_workspace_floats', M, 6, G) == 0 and _lib.query('xas_bn_workspace_floats', M, C, 65) == 0


# ------------------------------------------------------------------------------------------------ small related items
def test_stats_of_single_rows():
    """Mg = 1: mean = the row, var = 0, running_var becomes (1 - momentum) * running_var (the unbias factor falls back to 1)."""
    M, C, G = 3, 24, 3
    x = torch.randn(M, C, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV) * 2 + 3
    rm0, rv0 = torch.linspace(-2, 2, C, device=DEV), torch.linspace(0.5, 3, C, device=DEV)
    mo = torch.tensor(0.1, dtype=torch.float32, device=DEV)
    mean, var, rm, rv = run_stats(x, M, C, G, running=(rm0, rv0), momentum=0.1, message=True)
    assert torch.equal(mean, x) and bool((var == 0).all())
    want_v = rv0
    for _ in range(G):
        want_v = (1 - mo) * want_v
    assert same_bits(rv, want_v)
    rm64, bar = rm0.double(), 0.
    for k in range(G):
        bar = bar + 4 * U * (rm64.abs() + x[k].double().abs())
        rm64 = (1 - mo.double()) * rm64 + mo.double() * x[k].double()
    assert bool(((rm.double() - rm64).abs() <= bar).all())


def test_stats_unbias_follows_count():
    M, C, G = 300, 24, 2
    x = torch.randn(M, C, generator=torch.Generator(device=DEV).manual_seed(2), device=DEV) * 2 + 3
    rv0 = torch.linspace(0.5, 3, C, device=DEV)
    mo = float(torch.tensor(0.1, dtype=torch.float32))
    for count in (150, 77, 1):
        mean, var, rm, rv = run_stats(x, M, C, G, running=(torch.zeros(C, device=DEV), rv0), momentum=0.1, count=count)
        ub = count / (count - 1) if count > 1 else 1.
        rv64, bar = rv0.double(), 0.
        for k in range(G):
            bar = bar + 5 * U * (rv64.abs() + var[k].double() * ub)
            rv64 = (1 - mo) * rv64 + mo * var[k].double() * ub
        assert bool(((rv.double() - rv64).abs() <= bar).all()), count


def test_update_running_direct():
    """xas_bn_update_running: G = 3 updates in group order against float64; count = 1; C no multiple of 64."""
    C, G = 70, 3
    g = torch.Generator(device=DEV).manual_seed(3)
    mean, var = torch.randn(G, C, generator=g, device=DEV), torch.rand(G, C, generator=g, device=DEV) + 0.1
    rm0, rv0 = torch.randn(C, generator=g, device=DEV), torch.rand(C, generator=g, device=DEV) + 0.5
    mo = float(torch.tensor(0.1, dtype=torch.float32))
    for count in (1, 2, 150):
        rm, rv = Buf(C, src=rm0), Buf(C, src=rv0)
        launch(0, 'xas_bn_update_running', P(mean), P(var), rm.ptr(), rv.ptr(), 0.1, count, C, G)
        rm.intact(), rv.intact()
        ub = count / (count - 1) if count > 1 else 1.
        m64, v64, bm, bv = rm0.double(), rv0.double(), 0., 0.
        for k in range(G):
            bm, bv = bm + 5 * U * (m64.abs() + mean[k].double().abs()), bv + 5 * U * (v64.abs() + var[k].double() * ub)
            m64, v64 = (1 - mo) * m64 + mo * mean[k].double(), (1 - mo) * v64 + mo * var[k].double() * ub
        assert bool(((rm.t.double() - m64).abs() <= bm).all()) and bool(((rv.t.double() - v64).abs() <= bv).all()), count
        order = (1 - mo) * ((1 - mo) * ((1 - mo) * rm0.double() + mo * mean[2].double()) + mo * mean[1].double()) + mo * mean[0].double()
        assert float((order - m64).abs().max()) > 1e-3                        # (the reversed order is another number)


@pytest.mark.parametrize('n', [1, 3, 5, 4 * 256 * 1 + 3, 4 * 256 * 3 + 3, 4 * 256 * (3 * 4096 + 1) + 3],
                         ids=['n1', 'n3', 'n5', 'k1', 'k3', 'unrolled_loop'])
def test_abs_max(n):
    """xas_abs_max: the (negative) maximum planted in the unaligned tail, in the last float4 the 4-way unrolled loop reads and
    in the first float4 of the remainder loop.  The unrolled loop runs only where the 4096-block cap binds: n / 4 >
    3 * 4096 * 256 float4 (block 0's threads then make one unrolled trip whose fourth load is the last float4).  The result is
    the maximum over the slot's 32 sub-maxima; the other floats of the slot are untouched."""
    x = torch.rand(n, generator=torch.Generator(device=DEV).manual_seed(n % 1000), device=DEV) * 2 - 1
    n4 = n // 4
    spots = {n - 1, 0}
    if n4:
        spots |= {4 * n4 - 1, 4 * n4 - 4}                       # the last float4
    if n4 > 256:
        spots |= {1024, 4 * (n4 // 2) + 1}                      # first float4 of thread 256 (the remainder loop where the unrolled one ran)
    sub = torch.zeros(1024, dtype=torch.bool, device=DEV)
    sub[::32] = True
    for i, s in enumerate(sorted(spots)):
        old = float(x[s])
        x[s] = -(5. + i)
        slot = Buf(1024, fill=SENT_V)
        slot.t[sub] = 0.
        launch(0, 'xas_abs_max', P(x), n, slot.ptr())
        slot.intact()
        assert float(slot.t[sub].max()) == 5. + i, 'maximum planted at %d of %d' % (s, n)
        assert bool((slot.t[~sub] == SENT_V).all())
        x[s] = old
