"""xas_track_resolve without a GPU: the two symbols are exported, declared and bound with matching argument lists; every
argument rule answers 1 with its message before any launch; the workspace grows with N, Hy and K; and the oracle
(tests/_resolve_track_oracle.py): its Viterbi pass is the brute-force minimum on every tiny case, the planted effect holds for
it alone, and every unit that tests/test_gpu_resolve_track.py compares label by label is far from a tie at every frame."""
import ctypes

import numpy as np
import pytest

import _resolve_track_inputs as ri
import _resolve_track_oracle as ro

NAMES = {'xas_track_resolve_workspace_bytes': ('iii', 'z'),
         'xas_track_resolve': ('pppppp' 'iiii' 'ddd' 'ppppp' 'pp', 'i')}
MIN_GAP = 1e-9


def test_symbols_are_exported_declared_and_bound():
    from test_abi import header_prototypes
    from xas_amd import _lib, ops_track
    lib = _lib.load()
    protos = header_prototypes()
    for name, sig in NAMES.items():
        assert hasattr(lib, name), 'library does not export %s' % name
        assert protos.get(name) == sig == _lib.SIGNATURES[name]
    assert len(_lib.fn('xas_track_resolve').argtypes) == 20
    assert lib.xas_abi_version() == 3
    src = open(_lib.os.path.join(_lib.os.path.dirname(ri.__file__), '..', 'include', 'xas_hip.h')).read()
    assert '#define XAS_TRACK_MAX_HYPO %d\n' % ops_track.TRACK_MAX_HYPO in src and 2 * ops_track.TRACK_MAX_HYPO ** 2 <= 64
    assert (ops_track.TRACK_VEL_W, ops_track.TRACK_HYP_W, ops_track.TRACK_SWAP_W) == (1.0, 400.0, 400.0)
    assert ri.SHIPPED_PAIRS == ops_track.SWITCH_PAIRS and ri.WEIGHTS == dict(vel_w=1.0, hyp_w=400.0, swap_w=400.0)


def test_workspace_size_is_monotone_and_aligned():
    from xas_amd import _lib
    ws = _lib.fn('xas_track_resolve_workspace_bytes')
    for sizes in ([ws(N, 3, 18) for N in (1, 2, 15, 64, 4096)], [ws(64, Hy, 18) for Hy in (1, 2, 3, 4, 5)],
                  [ws(64, 3, K) for K in (1, 2, 18, 64)]):
        assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 and s > 0 for s in sizes), sizes
    assert ws(130, 5, 4) >= 130 * 4 * 50                                 # a back-pointer byte per frame and state
    for bad in ((0, 3, 18), (4, 0, 18), (4, 6, 18), (4, 3, 0), (4, 3, 65), (-1, 3, 3), (1 << 26, 3, 64)):
        assert ws(*bad) == 0, bad


def test_argument_errors_return_without_a_gpu():
    from xas_amd import _lib
    lib = _lib.load()
    f = _lib.fn('xas_track_resolve')
    one = ctypes.c_void_p(64)                 # an aligned non-null pointer: never dereferenced on these paths
    out = lambda i: ctypes.c_void_p((1 << 30) + (i << 20))
    err = lambda: lib.xas_last_error().decode()

    def call(N=4, Hy=3, K=5, S=2, start=(0, 3, 4), perm=(0, 2, 1, 3, 4), w=(1.0, 400.0, 400.0), workspace=one, outs=None,
             kps=one, world=one, unary=one, frame=one, null=None):
        table = (ctypes.c_int * len(start))(*start)
        ptab = (ctypes.c_int * len(perm))(*perm)
        outs = [out(i) for i in range(5)] if outs is None else outs
        get = lambda n, v: None if n == null else v
        return f(get('kps', kps), get('world', world), unary, get('perm', ptab), get('table', table), get('frame', frame),
                 N, Hy, K, S, *w, *outs, workspace, None)
    for n in ('kps', 'world', 'perm', 'table', 'frame'):
        assert call(null=n) == 1 and 'null buffer' in err(), n
    assert call(workspace=None) == 1 and 'null buffer' in err()
    assert call(outs=[None] + [out(i) for i in range(1, 5)]) == 1 and 'null buffer' in err()       # sel is required,
    assert call(unary=None, outs=[out(0), None, None, None, None], N=0, start=(0, 0, 0)) == 1 and 'bad shape' in err()   # the rest is not
    assert call(K=0) == 1 and 'bad shape' in err()
    assert call(K=65) == 1 and 'bad shape' in err()
    assert call(Hy=0) == 1 and 'Hy=0' in err()
    assert call(Hy=6) == 1 and 'Hy=6' in err()
    assert call(S=0, start=(0,)) == 1 and 'S=0' in err()
    assert call(S=5, start=(0, 1, 2, 3, 4, 4)) == 1 and 'S=5' in err()
    assert call(start=(1, 3, 4)) == 1 and 'start runs' in err()
    assert call(start=(0, 3, 5)) == 1 and 'start runs' in err()
    assert call(S=3, start=(0, 3, 2, 4)) == 1 and 'increasing' in err()
    assert call(S=3, start=(0, 2, 2, 4)) == 1 and 'increasing' in err()
    for bad in ((0, 2, 3, 1, 4), (0, 1, 2, 3, 5), (0, 1, 2, 3, -1), (1, 1, 2, 3, 4)):
        assert call(perm=bad) == 1 and 'involution' in err(), bad
    for i, name in enumerate(('vel_w', 'hyp_w', 'swap_w')):
        for v in (-1.0, float('nan'), float('inf')):
            w = [1.0, 400.0, 400.0]
            w[i] = v
            assert call(w=w) == 1 and name in err(), (name, v)
    assert call(workspace=ctypes.c_void_p(72)) == 1 and 'aligned' in err()
    # no output may lie on an input: N Hy K 3 floats of kps and world, N Hy K of unary, N ints of frame
    far = ctypes.c_void_p(1 << 31)
    for n, name in enumerate(('sel', 'hyp', 'swap', 'status', 'cost')):
        for inp in ('kps', 'world', 'unary', 'frame'):
            outs = [out(i) for i in range(5)]
            outs[n] = ctypes.c_void_p(far.value + 8)
            assert call(outs=outs, **{inp: far}) == 1 and '%s must not overlap %s' % (name, inp) in err(), (name, inp)
    outs = [out(i) for i in range(5)]
    outs[0] = ctypes.c_void_p(far.value + 4 * 3 * 5 * 3 * 4)              # sel starts where kps ends: no overlap, the next rule speaks
    assert call(outs=outs, kps=far, workspace=ctypes.c_void_p(72)) == 1 and 'aligned' in err()


TINY = list(ri.tiny_cases())


@pytest.mark.parametrize('name,c', TINY, ids=[n for n, _ in TINY])
def test_viterbi_is_the_brute_force_minimum(name, c):
    seen = set()
    for unit in ro.units_of(c['perm']):
        u = ro.unit_of(c, 0, unit)
        labels, C = u.viterbi()
        seen.add(u.resolved)
        if not u.resolved:
            assert (labels == ro.PASSED).all() and C == 0.0
            continue
        best, Cb, second = u.brute()
        assert abs(C - Cb) <= 1e-12 * Cb and abs(u.evaluate(labels) - Cb) <= 1e-12 * Cb
        assert np.array_equal(labels == ro.PASSED, ~u.usable)
        if second - Cb > 1e-12 * Cb:
            assert np.array_equal(labels, best)
            if len(u.st) > 1:                                            # the min-marginal gap never exceeds the runner-up's
                assert u.gaps().min() * Cb <= (second - Cb) * (1 + 1e-9) + 1e-9
    assert (True in seen) == (c['N'] > 2 or 'None' in name)               # two frames and a hole: one usable frame, passed


def test_oracle_tie_rule_takes_the_smallest_index():
    c = ri.make('tie')
    u = ro.unit_of(c, 0, (2, 2))
    labels, C = u.viterbi()
    assert (labels == 0).all() and u.gaps().max() == 0.0
    other = labels.copy()
    other[3:9] = 1
    assert u.evaluate(other) == C == u.evaluate(labels)


@pytest.mark.parametrize('T', [40, 130])
def test_planted_effect_holds_for_the_oracle_alone(T):
    """On every seed the exact minimum labels every frame of every pair as planted, where hypothesis 0 without exchange is
    right on fewer than half of them, and the best end state that differs costs visibly more."""
    for seed in range(6):
        c = ri.planted(seed, T)
        for a, b in c['pairs'][:3] if T > 40 else c['pairs']:
            a, b = min(a, b), max(a, b)
            u = ro.unit_of(c, 0, (a, b))
            labels, C = u.viterbi()
            hyp, swap, _, _ = ro.decode(c, 0, (a, b), labels)
            truth = c['truth']
            right = (hyp[:, 0] == truth['hyp'][:, a]) & (hyp[:, 1] == truth['hyp'][:, b]) & (swap[:, 0] == truth['swap'][:, a])
            naive = (truth['hyp'][:, a] == 0) & (truth['hyp'][:, b] == 0) & (truth['swap'][:, a] == 0)
            assert right.all(), (seed, a, b, int(right.sum()), T)
            assert naive.sum() < T / 2, (seed, a, b, int(naive.sum()))
            alpha, _ = u.forward()
            end = np.sort(alpha[-1])
            assert end[1] > 1.05 * end[0]


@pytest.mark.parametrize('name', list(ri.CASES))
def test_gpu_cases_are_far_from_a_tie_at_every_frame(name):
    """A condition on the inputs, asserted here so that the GPU test never has to exclude a case: outside the units a case
    declares tied by construction, the best and the second-best state of every frame differ by more than 1e-9 of the cost."""
    c = ri.make(name)
    for s in range(c['S']):
        for unit in ro.units_of(c['perm']):
            u = ro.unit_of(c, s, unit)
            if unit in c['ties'] or not u.resolved:
                continue
            assert u.gaps().min() > MIN_GAP, (name, s, unit, u.gaps().min())
    if name in ('tie', 'no_priors'):
        assert c['ties']
        for unit in c['ties']:
            assert ro.unit_of(c, 0, unit).gaps().min() <= MIN_GAP      # declared a tie, and one
    if name == 'one_usable':
        assert [ro.unit_of(c, 0, u).usable.sum() for u in ((0, 0), (1, 4), (7, 7))] == [1, 1, 0]
    if name == 'unusable':
        assert [int((~ro.unit_of(c, 0, u).usable).sum()) for u in ((0, 0), (1, 4), (2, 5), (7, 7), (9, 9))] == [2, 5, 1, 1, 1]
    if name == 'unary_null':                                             # the values are part of the cost
        assert (ro.resolve(c)['cost'] < ro.resolve(ri.make('unary'))['cost']).all()
