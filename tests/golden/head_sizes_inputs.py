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


def checksum(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def grad_kps(name):
    """The fixed upstream gradient [B, num_hypo, K, 3]."""
    D, K, B, hy, nb, seed = CASES[name]
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
