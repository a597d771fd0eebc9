"""float64 numpy oracle of xas_track_resolve (include/xas_hip.h states the cost): per (track, unit) the Viterbi pass with the
stated tie rule, a brute-force enumeration of all paths, the min-marginal gap of every frame and the cost of any labelling; and
the whole call over a case of tests/_resolve_track_inputs.py."""
import itertools

import numpy as np

PASSED = -1          # a label: the frame is not usable


def units_of(perm):
    """-> [(a, b)]: pairs a < b = perm[a] and single joints (k, k), ascending in the first joint."""
    return [(k, int(perm[k])) for k in range(len(perm)) if k <= perm[k]]


def states_of(Hy, pair):
    """-> [ns, 3] (e, h0, h1) in index order e Hy^2 + h0 Hy + h1; a single joint's state is (0, h, 0)."""
    if not pair:
        return np.array([(0, h, 0) for h in range(Hy)])
    return np.array([(e, h0, h1) for e in range(2) for h0 in range(Hy) for h1 in range(Hy)])


class Unit:
    """One (track, unit): world [T,Hy,K,3], unary [T,Hy,K] or None, frame [T]; everything float64 from the fp32 inputs."""

    def __init__(self, world, unary, frame, unit, vel_w, hyp_w, swap_w):
        a, b = unit
        self.pair = a != b
        T, Hy = world.shape[:2]
        self.st = states_of(Hy, self.pair)
        e, h0, h1 = self.st.T
        world = world.astype(np.float64)
        un = np.zeros(world.shape[:3]) if unary is None else unary.astype(np.float64)
        chans = [a, b] if self.pair else [a]
        self.usable = np.isfinite(world[:, :, chans]).all(axis=(1, 2, 3)) & np.isfinite(un[:, :, chans]).all(axis=(1, 2))
        self.idx = np.nonzero(self.usable)[0]
        ca, cb = np.where(e == 1, b, a), np.where(e == 1, a, b)          # the channel either joint reads
        self.XA, self.XB = world[:, h0, ca], world[:, h1, cb]           # [T,ns,3]
        self.local = hyp_w * (h0 + h1) + swap_w * e + un[:, h0, ca] + (un[:, h1, cb] if self.pair else 0.0)   # [T,ns]
        self.frame, self.vel_w, self.T = np.asarray(frame, np.float64), float(vel_w), T
        self.resolved = len(self.idx) >= 2

    def trans(self, tp, t):
        """[ns (before), ns (now)]"""
        d = ((self.XA[t][None] - self.XA[tp][:, None]) ** 2).sum(-1)
        if self.pair:
            d = d + ((self.XB[t][None] - self.XB[tp][:, None]) ** 2).sum(-1)
        return self.vel_w / (self.frame[t] - self.frame[tp]) * d

    def evaluate(self, labels):
        """C of a labelling [T] (PASSED on the unusable frames)."""
        labels = np.asarray(labels)
        assert np.array_equal(labels != PASSED, self.usable)
        C, tp = 0.0, None
        for t in self.idx:
            C += self.local[t, labels[t]]
            if tp is not None:
                C += self.trans(tp, t)[labels[tp], labels[t]]
            tp = t
        return C

    def forward(self):
        alpha, back = [self.local[self.idx[0]]], [np.zeros(len(self.st), np.int64)]
        for tp, t in zip(self.idx[:-1], self.idx[1:]):
            M = alpha[-1][:, None] + self.trans(tp, t)
            back.append(M.argmin(0))                                     # the first minimum: the smallest predecessor
            alpha.append(M.min(0) + self.local[t])
        return np.array(alpha), np.array(back)

    def viterbi(self):
        """-> (labels [T], C); passed through (all PASSED, 0) with fewer than two usable frames."""
        labels = np.full(self.T, PASSED)
        if not self.resolved:
            return labels, 0.0
        alpha, back = self.forward()
        s = int(alpha[-1].argmin())                                      # the first minimum: the smallest end state
        C = float(alpha[-1][s])
        for i in range(len(self.idx) - 1, -1, -1):
            labels[self.idx[i]] = s
            s = int(back[i][s])
        return labels, C

    def brute(self):
        """-> (labels, C, C of the best labelling that differs): every path enumerated."""
        best, second, arg = np.inf, np.inf, None
        for path in itertools.product(range(len(self.st)), repeat=len(self.idx)):
            labels = np.full(self.T, PASSED)
            labels[self.idx] = path
            C = self.evaluate(labels)
            if C < best:
                best, second, arg = C, best, labels
            elif C < second:
                second = C
        return arg, best, second

    def gaps(self):
        """Per usable frame (second-best min-marginal - best) / C: how far the frame's label is from flipping."""
        alpha, _ = self.forward()
        beta = [np.zeros(len(self.st))]
        for tp, t in zip(self.idx[:-1][::-1], self.idx[1:][::-1]):
            beta.append((self.trans(tp, t) + (self.local[t] + beta[-1])[None]).min(1))
        mm = np.sort(alpha + np.array(beta[::-1]), axis=1)
        if mm.shape[1] == 1:                                             # one state: nothing to choose
            return np.full(len(self.idx), np.inf)
        return (mm[:, 1] - mm[:, 0]) / np.maximum(mm[:, 0], 1e-300)


def unit_of(c, s, unit):
    lo, hi = c['start'][s], c['start'][s + 1]
    un = None if c['unary'] is None else c['unary'][lo:hi]
    return Unit(c['world'][lo:hi], un, c['frame'][lo:hi], unit, c['vel_w'], c['hyp_w'], c['swap_w'])


def decode(c, s, unit, labels):
    """A unit's labelling -> (hyp, swap, status [T,2 or 1] for its joints, sel [T,2 or 1,3] from kps)."""
    a, b = unit
    lo = c['start'][s]
    st = states_of(c['Hy'], a != b)
    joints = [a, b] if a != b else [a]
    hyp, swap, status = (np.zeros((len(labels), len(joints)), np.uint8) for _ in range(3))
    sel = np.zeros((len(labels), len(joints), 3), np.float32)
    for t, l in enumerate(labels):
        e, h0, h1 = (0, 0, 0) if l == PASSED else st[l]
        for i, k in enumerate(joints):
            hyp[t, i], swap[t, i], status[t, i] = (h1 if i else h0), e, l == PASSED
            sel[t, i] = c['kps'][lo + t, hyp[t, i], (joints[1 - i] if e else k)]
    return hyp, swap, status, sel


def resolve(c):
    """The whole call on a case (samples sorted by track and frame) -> dict of sel, hyp, swap, status [N,K] and cost [S,K]."""
    N, K, S = c['N'], c['K'], c['S']
    out = {'sel': np.zeros((N, K, 3), np.float32), 'hyp': np.zeros((N, K), np.uint8), 'swap': np.zeros((N, K), np.uint8),
           'status': np.zeros((N, K), np.uint8), 'cost': np.zeros((S, K))}
    for s in range(S):
        lo, hi = c['start'][s], c['start'][s + 1]
        for unit in units_of(c['perm']):
            labels, C = unit_of(c, s, unit).viterbi()
            hyp, swap, status, sel = decode(c, s, unit, labels)
            for i, k in enumerate(sorted(set(unit))):
                out['hyp'][lo:hi, k], out['swap'][lo:hi, k], out['status'][lo:hi, k] = hyp[:, i], swap[:, i], status[:, i]
                out['sel'][lo:hi, k] = sel[:, i]
                out['cost'][s, k] = C
    return out


def labels_of(c, s, unit, hyp, swap, status):
    """The labelling that per-sample outputs [N,K] give a unit of track s (for the oracle's evaluate)."""
    a, b = unit
    lo, hi = c['start'][s], c['start'][s + 1]
    Hy = c['Hy']
    h0, h1, e = hyp[lo:hi, a].astype(np.int64), hyp[lo:hi, b].astype(np.int64), swap[lo:hi, a].astype(np.int64)
    lab = e * Hy * Hy + h0 * Hy + h1 if a != b else h0
    return np.where(status[lo:hi, a] == 1, PASSED, lab)
