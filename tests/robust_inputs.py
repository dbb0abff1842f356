"""Inputs of the robust-accumulation tests (tests/test_robust_mirror.py without a GPU, tests/test_gpu_robust.py on the device): families of
one-sample images, each a list of N images (h, w, 4) that are folded in order, with the gains the resolve is run with.  Every family is
deterministic in (family, h, w, K).

Values the exact families use are multiples of 2^-6 below 4 (8 significant bits) or such a value times a power of two, so that every sum of
up to 16 of them, every product with a count up to 16 and the luminance (0.25 r + 0.5 g) + 0.25 b are exact in binary32: what the
family states about its result then holds bit for bit, not just approximately."""
import zlib

import numpy as np

f32 = np.float32
SIZES = [(1, 1), (7, 5), (8, 8), (17, 17), (70, 53)]              # (w, h)
GPU_SIZES = SIZES + [(200, 131)]
BUCKETS = (4, 8, 16)
FAMILIES = ("equal", "outlier", "ties", "integer_u", "short", "full", "ragged", "gain_zero", "gain_huge", "specials", "overflow", "nonfinite")
ONE_BELOW = float(np.nextafter(f32(1), f32(0)))


def rng_of(family, h, w, K):
    return np.random.default_rng(zlib.crc32(f"{family} {h} {w} {K}".encode()))


def short(rng, shape, lo=1, hi=256):
    """multiples of 2^-6 in [lo / 64, hi / 64)"""
    return (rng.integers(lo, hi, shape).astype(f32) / f32(64)).astype(f32)


def equal_lum_colours(rng, h, w, count):
    """`count` colours per pixel with one luminance and different hues: (g + d_j, g, g - d_j), d_j = j / 64: 0.25 (r + b) = 0.5 g exactly"""
    g = short(rng, (h, w), 64, 128)                                # [1, 2)
    out = []
    for j in range(count):
        d = f32(j) / f32(64)
        out.append(np.stack([g + d, g, g - d, np.ones_like(g)], -1).astype(f32))
    return out


def noisy(rng, h, w, N, firefly=0.02):
    """a smooth picture with multiplicative noise and, in `firefly` of the samples, a value a thousand times as bright"""
    base = rng.random((h, w, 3), f32) * f32(2) + f32(0.05)
    out = []
    for _ in range(N):
        s = base * (f32(0.5) + rng.random((h, w, 3), f32))
        s = np.where(rng.random((h, w, 1)) < firefly, s * f32(1000), s)
        out.append(np.concatenate([s, np.ones((h, w, 1), f32)], -1).astype(f32))
    return out


def make(family, h, w, K):
    """dict(samples = the N images in the order they are folded, gains = the gains to resolve with)"""
    assert family in FAMILIES and K in BUCKETS
    rng = rng_of(family, h, w, K)
    gains = [1.0]
    if family == "equal":                                          # every sample the same picture: the result is that picture, G = 0
        v = short(rng, (h, w, 4), 0, 256)                          # (zeros among them: S = 0 is "not S > 0")
        samples = [v.copy() for _ in range(2 * K)]
    elif family == "outlier":                                      # one bucket 2^20 times the constant others: the result is the constant
        c = short(rng, (h, w, 4))
        who = rng.integers(0, K, (h, w, 1))
        samples = [np.where(who == j, c * f32(2.0 ** 20), c).astype(f32) for j in range(K)]
    elif family == "ties":                                         # m tied keys of different hue below K - m far brighter buckets
        cols = equal_lum_colours(rng, h, w, K)
        m = rng.integers(1, K + 1, (h, w, 1))                      # (m = K: every key equal, G = 0)
        order = np.argsort(rng.random((h, w, K)), -1)              # which buckets are the tied ones: the first m of a permutation
        samples = []
        for j in range(K):
            tied = (np.argsort(order, -1)[..., j:j + 1] < m)
            samples.append(np.where(tied, cols[j], cols[j] * f32(4096)).astype(f32))
    elif family == "integer_u":                                    # half the buckets black, half of one luminance: G = 0.5, u = K / 4 exactly
        cols = equal_lum_colours(rng, h, w, K)
        dark = np.argsort(rng.random((h, w, K)), -1) < K // 2
        black = np.zeros((h, w, 4), f32)
        black[..., 3] = 1
        samples = [np.where(dark[..., j:j + 1], black, cols[j]).astype(f32) for j in range(K)]
        gains = [1.0, ONE_BELOW]
    elif family in ("short", "full", "ragged", "gain_zero", "gain_huge"):
        N = {"short": max(K - 3, 1), "full": K, "ragged": 2 * K + 3}.get(family, K + 1)
        samples = noisy(rng, h, w, N)
        gains = {"gain_zero": [0.0], "gain_huge": [1e30], "short": [1.0, 1e30]}.get(family, [1.0, 0.25])
    elif family == "specials":
        samples = noisy(rng, h, w, 2 * K + 1, firefly=0.05)
        values = (np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0e-40, -1.0e-42, 3.0e38, -3.0e38, -1.5)
        for s in samples:
            flat = s.reshape(-1, 4)
            for k, v in enumerate(values):
                flat[rng.integers(0, len(flat), 1 + len(flat) // 61), rng.integers(0, 4)] = v
            flat[rng.integers(0, len(flat), 1 + len(flat) // 61), :3] = f32(-0.75)      # negative luminance
        gains = [1.0, 3.0]
    elif family == "overflow":                                     # finite keys whose sum is +inf: G = 1, t at its cap
        v = (short(rng, (h, w, 1), 64, 128) * f32(2.0 ** 126)) * np.ones((1, 1, 4), f32)
        samples = [(v * f32(1 + (j % 3) * 0.25)).astype(f32) for j in range(K)]
    else:                                                          # "nonfinite": more non-finite buckets than the cap trims: the NaN comes out
        samples = noisy(rng, h, w, K, firefly=0.0)
        bad = np.argsort(rng.random((h, w, K)), -1) < rng.integers(0, K + 1, (h, w, 1))
        for j in range(K):
            samples[j][..., 0] = np.where(bad[..., j], f32(np.nan) if j % 2 else f32(np.inf), samples[j][..., 0])
    for s in samples:
        s.setflags(write=False)
    return dict(samples=samples, gains=gains)


def listed_cases():
    """(family, (w, h), K): every case of the CPU module; the GPU module adds 200 x 131"""
    return [(f, s, K) for f in FAMILIES for s in SIZES for K in BUCKETS]
