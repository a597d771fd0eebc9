"""Seeded inputs of xas_track_resolve for tests/test_resolve_track_abi.py and tests/test_gpu_resolve_track.py.  A case is a
dict of numpy arrays, the samples sorted by track and frame: kps, world [N,Hy,K,3] fp32, unary [N,Hy,K] fp32 or None, perm [K],
start [S+1], frame [N] int32, the weights; `truth` = the planted labels (hyp, swap [N,K]); `ties` = the units whose optimum
is not unique BY CONSTRUCTION (compared by cost, not by label).
The planted scene: every joint moves on a smooth curve (a few mm per frame); its true candidate carries 5 mm of noise and sits at
rank 0 in 60 % of the frames, the other ranks hold decoys 250-600 mm away along the joint's ray, drawn afresh per frame; a pair
is exchanged (its two channels' contents traded) in 30 % of the frames, chosen at random."""
import numpy as np

SHIPPED_PAIRS = ((1, 4), (2, 5), (3, 6), (14, 11), (15, 12), (16, 13))      # ops_eval.SWITCH_PAIRS
WEIGHTS = dict(vel_w=1.0, hyp_w=400.0, swap_w=400.0)                       # ops_track.TRACK_*_W


def perm_of(K, pairs):
    perm = list(range(K))
    for a, b in pairs:
        perm[a], perm[b] = b, a
    return perm


def scene(seed, lengths, K=18, Hy=3, pairs=SHIPPED_PAIRS, gaps=False, p_rank0=0.6, p_swap=0.3, offset=0.0, unary=False,
          **weights):
    rng = np.random.Generator(np.random.PCG64(seed))
    N, perm = int(sum(lengths)), perm_of(K, pairs)
    start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    frame = np.zeros(N, np.int32)
    world = np.zeros((N, Hy, K, 3))
    hyp, swap = np.zeros((N, K), np.uint8), np.zeros((N, K), np.uint8)
    for s, T in enumerate(lengths):
        lo = start[s]
        f = np.cumsum(rng.integers(1, 6, T)) if gaps else np.arange(T) + 3
        frame[lo:lo + T] = f
        centre, amp = rng.uniform(-800, 800, (K, 3)) + offset, rng.uniform(50, 250, (K, 3))
        rate, phase = rng.uniform(0.02, 0.06, (K, 3)), rng.uniform(0, 6.28, (K, 3))
        true = centre + amp * np.sin(rate * f[:, None, None] + phase)                   # [T,K,3]
        ray = rng.normal(size=(K, 3))
        ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
        rank = np.where(rng.random((T, K)) < p_rank0, 0, np.minimum(rng.integers(1, max(Hy, 2), (T, K)), Hy - 1))   # of the true candidate
        cand = np.zeros((T, Hy, K, 3))
        for h in range(Hy):
            decoy = true + ray * (rng.uniform(250, 600, (T, K, 1)) * rng.choice([-1.0, 1.0], (T, K, 1)))
            cand[:, h] = np.where((rank == h)[..., None], true + rng.normal(0, 5.0, (T, K, 3)), decoy)
        ex = np.zeros((T, K), bool)
        for a, b in pairs:
            ex[:, a] = ex[:, b] = rng.permutation(T) < min(round(p_swap * T), (T - 1) // 2)   # never half: the mirror would cost the same
        world[lo:lo + T] = np.where(ex[:, None, :, None], cand[:, :, perm], cand)
        hyp[lo:lo + T], swap[lo:lo + T] = rank, ex
    c = dict(WEIGHTS)
    c.update(weights)
    c.update(kps=rng.uniform(-1, 1, (N, Hy, K, 3)).astype(np.float32), world=world.astype(np.float32), perm=perm, pairs=tuple(pairs),
             unary=rng.uniform(0, 300, (N, Hy, K)).astype(np.float32) if unary else None, start=[int(v) for v in start], frame=frame,
             N=N, Hy=Hy, K=K, S=len(lengths), truth={'hyp': hyp, 'swap': swap}, ties=set())
    return c


def _unusable(c):
    w = c['world']
    w[0:2, 0, 0] = np.nan                     # a single joint: the first two frames
    w[0, 1, 1, 2] = np.inf                    # a pair through one coordinate of one hypothesis of its first channel: the start,
    w[10:13, 2, 4] = np.nan                   # three frames in the middle through its second channel,
    w[29, 0, 4, 0] = -np.inf                  # and the end
    w[29, :, 7] = np.nan                      # a single joint: the end
    w[5, 0, 2] = np.nan                       # another pair: one frame
    c['unary'][17, 1, 9] = np.nan             # a single joint through its unary alone
    return c


def _one_usable(c):
    c['world'][[0, 1, 2, 4, 5], 0, 1] = np.nan       # the pair (1, 4) and the joint 0 keep frame 3 alone; the joint 7 keeps none
    c['world'][[0, 1, 2, 4, 5], 1, 0] = np.nan
    c['world'][:, 2, 7] = np.nan
    return c


def _tie(c):
    c['world'][:, 1] = c['world'][:, 0]              # hypothesis 1 repeats hypothesis 0, and no rank prior tells them apart
    c['ties'] = {(k, c['perm'][k]) for k in range(c['K']) if k <= c['perm'][k]}
    return c


def _no_priors(c):
    # without swap_w a pair's labelling and its mirror (every bit flipped, the two hypotheses traded) assign the same
    # candidates to the same two curves: an exact tie, whatever the data
    c['ties'] = {(0, 1)}
    return c


CASES = {
    'T1': lambda: scene(1, [1]),
    'T2': lambda: scene(2, [2]),
    'Hy1': lambda: scene(3, [7, 20], Hy=1),
    'Hy3_K18': lambda: scene(4, [40]),
    'Hy5': lambda: scene(5, [33], K=4, Hy=5, pairs=((0, 1),)),
    'identity': lambda: scene(6, [25], K=5, pairs=()),
    'K2_pair': lambda: scene(7, [30], K=2, Hy=2, pairs=((0, 1),)),
    'unusable': lambda: _unusable(scene(8, [30], K=10, pairs=((1, 4), (2, 5)), unary=True)),
    'one_usable': lambda: _one_usable(scene(9, [6], K=8, pairs=((1, 4),))),
    'frame_gaps': lambda: scene(10, [40], K=6, pairs=((1, 4),), gaps=True),
    'several': lambda: scene(11, [1, 2, 7, 65, 130], K=6, pairs=((1, 4), (2, 5))),
    'unary': lambda: scene(12, [24], K=6, pairs=((1, 4),), unary=True),
    'unary_null': lambda: dict(make('unary'), unary=None),              # the same inputs without: null means zero
    'vel0': lambda: scene(13, [12], K=6, pairs=((1, 4),), unary=True, vel_w=0.0),
    'no_priors': lambda: _no_priors(scene(14, [30], K=5, pairs=((0, 1),), hyp_w=0.0, swap_w=0.0)),
    'far': lambda: scene(15, [30], K=6, pairs=((1, 4),), offset=1e4),
    'tie': lambda: _tie(scene(16, [20], K=4, Hy=2, pairs=((0, 1),), hyp_w=0.0)),
}
_made = {}


def make(name):
    """The case, built once and shared: callers leave it unchanged."""
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def planted(seed, T):
    """One track of the planted scene with the shipped pairs and weights (the experiment of the issue)."""
    return scene(100 + seed, [T])


def tiny_cases():
    """Every small shape the brute force can enumerate: T <= 4, Hy <= 2, a pair and a single joint, with and without an
    unusable frame."""
    for T in (2, 3, 4):
        for Hy in (1, 2):
            for hole in (None, 0, 1, T - 1):
                c = scene(1000 + 10 * T + Hy, [T], K=3, Hy=Hy, pairs=((0, 2),), gaps=True)
                if hole is not None:
                    c['world'][hole, Hy - 1, 0, 1] = np.nan
                    c['world'][hole, 0, 1, 0] = np.nan
                yield 'T%d_Hy%d_hole%s' % (T, Hy, hole), c
