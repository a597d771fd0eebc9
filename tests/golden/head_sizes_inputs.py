"""Seeded inputs and the float64 restatement for the soft-argmax head at cube sides other than 16/32/64
(tests/test_gpu_head_sizes.py, tests/test_head_sizes_abi.py, tests/golden/make_golden_head_sizes.py).

Logits are never stored: every case is rebuilt from its seed.  The generator uses only operations that give the same bits
on every machine - PCG64 integers for the noise and float64 + - * / for the smooth part (no exp / log), one rounding to
float32 at the end - so the CRC-32 of the logits stored in head_sizes.npz pins the input exactly.

Per joint: a rational bump over (h, w), three depth peaks of the shape a / (1 + (d - c)^2)^2 (at distance 4 a peak has
fallen to 0.35 % of its height, so peaks four bins apart are separate maxima), and uniform noise of standard deviation 0.05.
Planted on purpose:
  * joint 0 of image 0: peaks at bin 1 and at bin D-2 (the outermost bins the peak pick accepts); at D = 128 instead
    peaks at 62 and 66, whose windows (radius 7) straddle bins 63/64;
  * joint 1 of image 0: two EXACTLY equal peaks.  Depth bins 4a..4a+3 are copied, noise included, over bins 4b..4b+3, so
    the two peaks see identical numbers in identical order in any implementation that treats depth bins alike per aligned
    group of four (the HIP kernels hold four bins per thread; the reference reduces every bin by the same schedule) and the
    marginals tie bit for bit: the order of the two hypotheses is then the tie rule alone (lower bin first).  At D = 96
    the pair is bins 61 and 65: the tie crosses the 63/64 boundary of the two-bins-per-lane finalize kernel.  D = 128 has
    no tie joint: there torch.topk (whose order among equal values is unspecified) returns the HIGHER bin first, so the
    reference cannot serve as the yardstick of the rule at that size.
"""
import zlib

import numpy as np

# name -> (D, K, B, num_hypo, neighbor, seed)
CASES = {
    'd12': (12, 3, 2, 3, 5, 1201),       # G = 3, non-power-of-two rows, tiny HW
    'd24': (24, 18, 2, 3, 15, 1202),     # full joint count at a small cube (input 96^2)
    'd40': (40, 2, 2, 1, 0, 1203),       # single-hypothesis form, G = 10
    'd96': (96, 18, 2, 3, 15, 1204),     # D > 64 with the full joint count (input 384^2)
    'd128': (128, 2, 1, 3, 15, 1205),    # upper limit; peaks at 62 / 66
}
GRAD_STRIDE = 4099                        # prime: the strided sample of grad_logits walks through every axis
NOISE_STD = 0.05


def tie_quads(D):
    """(a, b): depth bins 4a..4a+3 are copied over 4b..4b+3 for the tie joint."""
    return (15, 16) if D >= 96 else (0, D // 4 - 1)


def planted(name):
    """-> {(b, k): (centres, amplitudes)} of the joints with hand-placed peaks."""
    D, K, B, hy, nb, seed = CASES[name]
    out = {}
    out[(0, 0)] = ([62, 66, 20], [6.0, 5.0, 4.0]) if D == 128 else ([1, D // 2, D - 2], [5.0, 6.0, 4.0])
    if K >= 2 and D != 128:
        a, _ = tie_quads(D)
        third = 20 if D >= 96 else 4 * (D // 8) + 2
        out[(0, 1)] = ([4 * a + 1, third], [6.0, 4.0])
    return out


def logits(name):
    """float32 [B, K*D, D, D] (the reference's NCHW order: channel k*D + d)."""
    D, K, B, hy, nb, seed = CASES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    g = np.arange(D, dtype=np.float64)
    special = planted(name)
    out = np.empty((B, K, D, D, D), np.float32)
    noise_scale = NOISE_STD * 12.0 ** 0.5 / 65536.0
    for b in range(B):
        for k in range(K):
            if (b, k) in special:
                cz, amp = special[(b, k)]
            else:
                # three centres at least D/5 apart, away from the borders, in a random order
                jitter = rng.integers(-1, 2, 3) if D >= 24 else np.zeros(3, np.int64)
                cz = (np.array([D // 5, D // 2, D - 1 - D // 5]) + jitter)[rng.permutation(3)]
                amp = [6.0, 5.0, 4.0]
            cx, cy = (D // 4 + rng.integers(0, D // 2 + 1, 2)).astype(np.float64)
            sxy = D / 10.0
            fz = sum(a / (1.0 + (g - float(c)) ** 2) ** 2 for a, c in zip(amp, cz))
            fxy = 3.0 / (1.0 + ((g[None, :] - cx) ** 2 + (g[:, None] - cy) ** 2) / (sxy * sxy))
            u = rng.integers(0, 65536, (D, D, D), dtype=np.uint16)
            vol = fz[:, None, None] + fxy[None, :, :] + (u.astype(np.float64) - 32767.5) * noise_scale
            out[b, k] = vol.astype(np.float32)
            if (b, k) == (0, 1) and (b, k) in special:
                qa, qb = tie_quads(D)
                out[b, k, 4 * qb:4 * qb + 4] = out[b, k, 4 * qa:4 * qa + 4]
    return out.reshape(B, K * D, D, D)


# ---- second table: the launch paths the first one does not reach ----------------------------------------------------------
# Same construction (PCG64 integers, float64 rational bumps, one rounding to float32), stored in head_edges.npz.
# name -> (D, K, B, num_hypo, neighbor, seed).  Geometry of the general policy: G = D/4 lanes per joint, at most 1024 / G
# joints per block, else equal joint tiles over gridDim.z; 128 pixels per block.
EDGES = {
    't12a': (12, 341, 2, 3, 5, 1301),     # G = 3: 341 joints = 1023 threads, the widest single tile (not a whole number of waves)
    't12b': (12, 342, 2, 3, 5, 1302),     # two exact tiles of 171 joints
    't12c': (12, 343, 2, 3, 5, 1303),     # ragged: tiles of 172 with 172 + 171 live; chunks of 128 + 16 pixels
    't68': (68, 61, 1, 3, 15, 1304),      # G = 17: tiles of 31 + 30 joints (527 threads), two depth bins per lane (D > 64)
    'e68': (68, 3, 2, 3, 15, 1305),       # planted peaks on both sides of bins 63/64, tie pair 61 / 65, maxima on bins 0 and 67
    'w16': (16, 257, 1, 3, 7, 1306),      # power-of-two side too wide for one block: general policy, tiles of 129 + 128
    'tie128': (128, 2, 1, 3, 15, 1307),   # the tie rule at the upper limit: joint 1 ties bins 61 / 65
    'h6': (24, 3, 2, 6, 5, 1308),         # six hypotheses: joints 0 and 2 carry six peaks, joint 1 ONE peak and five zero-score fill-ins
}
# D = 4 (G = 1, HW = 16, two inner bins): both forms for every K; K = 4 is the only one on the power-of-two policy
for _k in (1, 2, 3, 4, 5):
    EDGES['e4k%ds' % _k] = (4, _k, 2, 1, 0, 1310 + _k)
    EDGES['e4k%dm' % _k] = (4, _k, 2, 2, 3, 1310 + _k)
E4 = [n for n in EDGES if n.startswith('e4')]


def spec(name):
    return CASES[name] if name in CASES else EDGES[name]


def edge_planted(name):
    """-> {(b, k): (centres, amplitudes, tie quads or None, noise)} of the joints with hand-placed peaks.  A tie joint has
    one peak at bin 4a + 1 whose quad a is copied over quad b (see the module docstring)."""
    D, K, B, hy, nb, seed = EDGES[name]
    out = {}
    if D == 12:                                            # first joint, both sides of every tile boundary, last joint
        for b, k, cz in ((0, 0, [1, 6, 10]), (0, 170, [10, 1, 5]), (0, 171, [6, 10, 1]), (0, 172, [1, 10, 5]), (1, K - 1, [10, 6, 1])):
            out[(b, k)] = (cz, [6.0, 5.0, 4.0], None, True)
    elif name == 't68':                                    # tile boundary 30 / 31; peaks on bins 63, 64 and 66 = D - 2
        for k, cz in ((0, [1, 64, 66]), (30, [63, 30, 2]), (31, [64, 20, 66]), (60, [66, 63, 1])):
            out[(0, k)] = (cz, [6.0, 5.0, 4.0], None, True)
    elif name == 'e68':
        out[(0, 0)] = ([1, 64, 66], [6.0, 5.0, 4.0], None, True)
        out[(0, 1)] = ([63, 30, 2], [6.0, 5.0, 4.0], None, True)
        out[(0, 2)] = ([61, 20], [6.0, 4.0], (15, 16), True)          # tie across the lane boundary: bins 61 and 65
        out[(1, 0)] = ([66, 1, 64], [6.0, 5.0, 4.0], None, True)
        out[(1, 1)] = ([67, 30, 10, 50], [6.0, 5.0, 4.0, 3.0], None, True)    # the highest maximum on bin D - 1: never a peak
        out[(1, 2)] = ([0, 20, 40, 60], [6.0, 5.0, 4.0, 3.0], None, True)     # ... and on bin 0
    elif name == 'w16':                                    # tile boundary 128 / 129
        for k, cz in ((0, [1, 8, 14]), (128, [14, 1, 8]), (129, [8, 14, 1]), (256, [1, 14, 7])):
            out[(0, k)] = (cz, [6.0, 5.0, 4.0], None, True)
    elif name == 'tie128':
        out[(0, 0)] = ([127, 62, 66, 20], [7.0, 6.0, 5.0, 4.0], None, True)   # bin 127 = D - 1 (lane 63's second bin) is no peak
        out[(0, 1)] = ([61, 20], [6.0, 4.0], (15, 16), True)
    elif name == 'h6':
        out[(0, 0)] = ([9, 1, 22, 17, 5, 13], [6.0, 5.5, 5.0, 4.5, 4.0, 3.5], None, True)
        out[(1, 0)] = ([22, 6, 14, 1, 18, 10], [6.0, 5.5, 5.0, 4.5, 4.0, 3.5], None, True)
        out[(0, 2)] = ([13, 21, 1, 9, 17, 5], [6.0, 5.5, 5.0, 4.5, 4.0, 3.5], None, True)
        out[(1, 2)] = ([2, 18, 10, 22, 6, 14], [6.0, 5.5, 5.0, 4.5, 4.0, 3.5], None, True)
        out[(0, 1)] = ([9], [6.0], None, False)            # noise-free, one peak: the marginal is strictly monotone on either side
        out[(1, 1)] = ([14], [6.0], None, False)
    return out


def edge_unordered(name):
    """Joints (b, k) whose hypothesis ORDER the reference leaves to torch.topk's handling of equal scores: the exact tie at
    D = 128 (higher bin first there, see the module docstring) and the zero-score fill-ins of the one-peak joints of h6 (five
    equal zeros).  The rule of the HIP head and of restate() - lower bin first - is asserted against literal lists instead."""
    return {'tie128': [(0, 1)], 'h6': [(0, 1), (1, 1)]}.get(name, [])


def edge_expected(name):
    """-> {(b, k): literal peak-index list} for the planted joints whose order follows from the construction alone."""
    out = {}
    for (b, k), (cz, amp, tie, noise) in edge_planted(name).items():
        if tie:
            out[(b, k)] = [4 * tie[0] + 1, 4 * tie[1] + 1, cz[1]]
        elif len(cz) == 1:                                 # the peak, then the lowest remaining inner bins
            n = EDGES[name][3]
            out[(b, k)] = [cz[0]] + [d for d in range(1, EDGES[name][0] - 1) if d != cz[0]][:n - 1]
        else:
            out[(b, k)] = [c for _, c in sorted(zip(amp, cz), reverse=True) if 1 <= c <= EDGES[name][0] - 2][:EDGES[name][3]]
    return out


def edge_logits(name):
    """float32 [B, K*D, D, D] of a case of EDGES."""
    D, K, B, hy, nb, seed = EDGES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    g = np.arange(D, dtype=np.float64)
    special = edge_planted(name)
    out = np.empty((B, K, D, D, D), np.float32)
    noise_scale = NOISE_STD * 12.0 ** 0.5 / 65536.0
    for b in range(B):
        for k in range(K):
            tie, noise = None, True
            if (b, k) in special:
                cz, amp, tie, noise = special[(b, k)]
            elif D == 4:                                   # one peak on either inner bin (a border peak leaves no inner maximum)
                cz, amp = [1 + int(rng.integers(0, 2))], [4.0 + float(rng.integers(0, 3))]
            else:
                jitter = rng.integers(-1, 2, 3) if D >= 24 else np.zeros(3, np.int64)
                cz = (np.array([D // 5, D // 2, D - 1 - D // 5]) + jitter)[rng.permutation(3)]
                amp = [6.0, 5.0, 4.0]
            cx, cy = (D // 4 + rng.integers(0, D // 2 + 1, 2)).astype(np.float64)
            sxy = D / 10.0
            fz = sum(a / (1.0 + (g - float(c)) ** 2) ** 2 for a, c in zip(amp, cz))
            fxy = 3.0 / (1.0 + ((g[None, :] - cx) ** 2 + (g[:, None] - cy) ** 2) / (sxy * sxy))
            vol = fz[:, None, None] + fxy[None, :, :]
            if noise:
                u = rng.integers(0, 65536, (D, D, D), dtype=np.uint16)
                vol = vol + (u.astype(np.float64) - 32767.5) * noise_scale
            out[b, k] = vol.astype(np.float32)
            if tie:
                qa, qb = tie
                out[b, k, 4 * qb:4 * qb + 4] = out[b, k, 4 * qa:4 * qa + 4]
    return out.reshape(B, K * D, D, D)


def checksum(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def grad_kps(name):
    """The fixed upstream gradient [B, num_hypo, K, 3]."""
    D, K, B, hy, nb, seed = spec(name)
    rng = np.random.Generator(np.random.PCG64(seed + 5000))
    return ((rng.integers(0, 65536, (B, hy, K, 3)).astype(np.float64) - 32767.5) / 16384.0).astype(np.float32)


def restate(lg, K, num_hypo, neighbor):
    """The head restated on a torch tensor of any float type and device (float64 in the tests): softmax over D*H*W per
    joint, marginals, expectation along w and h, depth peaks (>= both neighbours, interior bins, value descending, lower bin
    first among equals), windowed expectation along depth; neighbor == 0: the plain expectation.
    -> kps [B,num_hypo,K,3], pz [B,K,D], z_idx [B,K,num_hypo] (zeros for neighbor == 0)."""
    import torch
    B, C, H, W = lg.shape
    D = C // K
    p = torch.softmax(lg.reshape(B, K, -1), dim=2).reshape(B, K, D, H, W)
    ar = torch.arange(D, dtype=lg.dtype, device=lg.device)
    X = (p.sum(dim=(2, 3)) * ar).sum(-1)
    Y = (p.sum(dim=(2, 4)) * ar).sum(-1)
    pz = p.sum(dim=(3, 4))
    if neighbor == 0:
        Z = (pz * ar).sum(-1).unsqueeze(-1)                                  # [B,K,1]
        idx = torch.zeros(B, K, 1, dtype=torch.int64, device=lg.device)
    else:
        mid = pz[..., 1:-1]
        peak = (mid >= pz[..., :-2]) & (mid >= pz[..., 2:])
        score = torch.where(peak, mid, torch.zeros_like(mid)).detach()
        idx = torch.sort(score, dim=-1, descending=True, stable=True).indices[..., :num_hypo] + 1
        win = ((ar.view(1, 1, 1, D) - idx.unsqueeze(-1).to(lg.dtype)).abs() <= neighbor // 2).to(lg.dtype)
        pw = pz.unsqueeze(2) * win
        Z = (pw * ar).sum(-1) / pw.sum(-1)                                   # [B,K,Hy]
    x = (X / H * 2 - 1).unsqueeze(1).expand(B, num_hypo, K)
    y = (Y / W * 2 - 1).unsqueeze(1).expand(B, num_hypo, K)
    z = (Z / D * 2 - 1).permute(0, 2, 1)
    return torch.stack([x, y, z], dim=-1), pz, idx
