"""xas_track_resolve alone on the GPU against the float64 oracle (tests/_resolve_track_oracle.py) on the cases of
tests/_resolve_track_inputs.py: labels, status and sel exactly, the cost to 1e-12 (a few hundred positive double terms, no
cancellation; differences of fp32 inputs are exact in double).  Units a case declares tied by construction are compared by
cost: the oracle's evaluation of the kernel's own labelling is the optimum.  tests/test_resolve_track_abi.py asserts that every
other unit is far from a tie at every frame, so nothing is excluded here.  Two runs over differently poisoned workspace and
outputs give the same bits and leave the inputs alone; ops_track.track_resolve sorts, scatters and names."""
import ctypes

import numpy as np
import pytest
import torch

import _resolve_track_inputs as ri
import _resolve_track_oracle as ro

pytestmark = pytest.mark.gpu
COST_RTOL = 1e-12
_ref = {}


def reference(name):
    if name not in _ref:
        _ref[name] = ro.resolve(ri.make(name))
    return _ref[name]


def run(c, poison=0xAB):
    """One call over the C ABI, every output and the workspace filled with `poison` first -> (outputs as numpy, inputs after)."""
    from xas_amd._lib import call, ptr, query
    N, Hy, K, S = c['N'], c['Hy'], c['K'], c['S']
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ins = {'kps': dev(c['kps']), 'world': dev(c['world']), 'unary': dev(c['unary']), 'frame': dev(c['frame'])}
    nbytes = query('xas_track_resolve_workspace_bytes', N, Hy, K)
    assert nbytes > 0 and nbytes % 16 == 0
    fill = lambda *shape: torch.full(shape, poison, dtype=torch.uint8, device='cuda')
    ws = fill(nbytes)
    out = {'sel': fill(N, K, 12).view(torch.float32), 'hyp': fill(N, K), 'swap': fill(N, K), 'status': fill(N, K),
           'cost': fill(S, K * 8).view(torch.float64)}
    call('xas_track_resolve', ptr(ins['kps']), ptr(ins['world']), ptr(ins['unary']), (ctypes.c_int * K)(*c['perm']),
         (ctypes.c_int * (S + 1))(*c['start']), ptr(ins['frame']), N, Hy, K, S, c['vel_w'], c['hyp_w'], c['swap_w'],
         ptr(out['sel']), ptr(out['hyp']), ptr(out['swap']), ptr(out['status']), ptr(out['cost']), ptr(ws))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, {k: v.cpu().numpy() for k, v in ins.items() if v is not None}


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check(c, got, ref):
    K = c['K']
    tied = sorted(k for unit in c['ties'] for k in unit)
    rest = [k for k in range(K) if k not in tied]
    assert got['sel'].shape == (c['N'], K, 3)
    for key in ('hyp', 'swap', 'status'):
        assert np.array_equal(got[key][:, rest], ref[key][:, rest]), key
    assert same_bits(got['sel'][:, rest], ref['sel'][:, rest])
    assert np.array_equal(got['status'], ref['status'])                  # usable or not: not a matter of ties
    err = np.abs(got['cost'] - ref['cost'])
    print('cost: largest relative difference %.3g' % (err / np.maximum(ref['cost'], 1e-300))[ref['cost'] > 0].max(initial=0.0))
    assert (err <= COST_RTOL * ref['cost']).all()
    for s in range(c['S']):
        for unit in sorted(c['ties']):                                   # tied: the kernel's labelling costs the optimum
            u = ro.unit_of(c, s, unit)
            labels = ro.labels_of(c, s, unit, got['hyp'], got['swap'], got['status'])
            assert labels.max() < len(u.st)
            if u.resolved:
                C = u.evaluate(labels)
                assert abs(C - ref['cost'][s, unit[0]]) <= COST_RTOL * ref['cost'][s, unit[0]]
            hyp, swap, status, sel = ro.decode(c, s, unit, labels)       # and sel is what those labels read from kps
            lo, hi = c['start'][s], c['start'][s + 1]
            for i, k in enumerate(sorted(set(unit))):
                assert same_bits(got['sel'][lo:hi, k], sel[:, i]) and np.array_equal(got['swap'][lo:hi, k], swap[:, i])


@pytest.mark.parametrize('name', list(ri.CASES))
def test_kernel_matches_the_oracle(name):
    c = ri.make(name)
    before = {k: c[k].copy() for k in ('kps', 'world', 'frame')}
    got, after = run(c, 0xAB)
    check(c, got, reference(name))
    again, _ = run(c, 0x5C)                                              # other poison in the workspace and the outputs
    for k in got:
        assert same_bits(got[k], again[k]), k
    for k in before:
        assert same_bits(after[k], before[k]) and same_bits(c[k], before[k]), k
    if c['unary'] is not None:
        assert same_bits(after['unary'], c['unary'])


def test_passed_through_is_bit_for_bit():
    """T = 1, and units with one or no usable frame: hypothesis 0 of the joint's own channel, NaN and all."""
    for name in ('T1', 'one_usable'):
        c = ri.make(name)
        got, _ = run(c)
        units = ro.units_of(c['perm']) if name == 'T1' else [(0, 0), (1, 4), (7, 7)]
        for k in sorted({k for u in units for k in u}):
            assert same_bits(got['sel'][:, k], c['kps'][:, 0, k]) and (got['status'][:, k] == 1).all()
            assert not got['hyp'][:, k].any() and not got['swap'][:, k].any() and (got['cost'][:, k] == 0).all()
    c = ri.make('one_usable')
    assert (run(c)[0]['status'][:, [2, 3, 5, 6]] == 0).all()            # its neighbours are resolved


def test_optional_outputs_may_be_null():
    from xas_amd._lib import call, ptr, query
    c = ri.make('K2_pair')
    N, Hy, K, S = c['N'], c['Hy'], c['K'], c['S']
    kps, world, frame = (torch.from_numpy(c[k]).cuda() for k in ('kps', 'world', 'frame'))
    sel = torch.empty(N, K, 3, device='cuda')
    ws = torch.empty(query('xas_track_resolve_workspace_bytes', N, Hy, K), dtype=torch.uint8, device='cuda')
    call('xas_track_resolve', ptr(kps), ptr(world), None, (ctypes.c_int * K)(*c['perm']), (ctypes.c_int * (S + 1))(*c['start']),
         ptr(frame), N, Hy, K, S, c['vel_w'], c['hyp_w'], c['swap_w'], ptr(sel), None, None, None, None, ptr(ws))
    assert same_bits(sel.cpu().numpy(), reference('K2_pair')['sel'])


def test_op_sorts_scatters_and_names():
    """ops_track.track_resolve on samples in shuffled order with scattered track numbers: the oracle's results in the order
    given; with labels, a track planted fully exchanged is named, one bit per (track, pair)."""
    from xas_amd import ops_track
    c = ri.make('several')
    ref = reference('several')
    N, K, S = c['N'], c['K'], c['S']
    rng = np.random.Generator(np.random.PCG64(5))
    order = rng.permutation(N)
    ids = np.array([7, 3, 11, 20, 5])                                    # the tracks' numbers: any integers
    rank = np.argsort(np.argsort(ids))                                   # the op lists the tracks ascending
    track = np.repeat(ids, np.diff(c['start']))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r = ops_track.track_resolve(dev(c['kps'][order]), dev(c['world'][order]), track[order], c['frame'][order], pairs=c['pairs'])
    assert r['tracks'].tolist() == sorted(ids.tolist()) and 'named' not in r
    for key in ('hyp', 'swap', 'status'):
        assert np.array_equal(r[key].cpu().numpy(), ref[key][order]), key
    assert same_bits(r['sel'].cpu().numpy(), ref['sel'][order])
    cost = r['cost'].cpu().numpy()
    assert (np.abs(cost[rank] - ref['cost']) <= COST_RTOL * ref['cost']).all()
    with pytest.raises(RuntimeError, match='twice'):
        ops_track.track_resolve(dev(c['kps'][:3]), dev(c['world'][:3]), [0, 0, 0], [1, 2, 1], pairs=c['pairs'])
    # naming: the labels are the chosen kps themselves, in patch pixels; in track 3 (65 frames) the pair (1, 4) is planted
    # fully exchanged, so there the labels of joint 1 are what the kernel gave joint 4
    S_img = 256.0
    gt = ((ref['sel'].astype(np.float64)[..., :2] + 1) / 2 * (S_img - 1))
    lo, hi = c['start'][3], c['start'][4]
    gt[lo:hi, [1, 4]] = gt[lo:hi, [4, 1]]
    r = ops_track.track_resolve(dev(c['kps'][order]), dev(c['world'][order]), track[order], c['frame'][order], pairs=c['pairs'],
                                gt=dev(gt.astype(np.float32)[order]), image_size=S_img)
    named = np.zeros((S, K), np.uint8)
    named[3, [1, 4]] = 1
    assert np.array_equal(r['named'].cpu().numpy()[rank], named)
    want_swap, want_sel = ref['swap'].copy(), ref['sel'].copy()
    want_swap[lo:hi, [1, 4]] ^= 1
    want_sel[lo:hi, [1, 4]] = ref['sel'][lo:hi, [4, 1]]
    assert np.array_equal(r['swap'].cpu().numpy(), want_swap[order]) and same_bits(r['sel'].cpu().numpy(), want_sel[order])
    want_hyp = ref['hyp'].copy()
    want_hyp[lo:hi, [1, 4]] = ref['hyp'][lo:hi, [4, 1]]                  # the two curves trade their names, hypotheses and all
    assert np.array_equal(r['hyp'].cpu().numpy(), want_hyp[order])
