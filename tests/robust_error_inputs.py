"""Inputs of the robust-error-estimate tests (tests/test_robust_error_mirror.py without a GPU, tests/test_gpu_robust_error.py on the
device): the families of tests/robust_inputs.py that fill every bucket, plus those the estimate needs, each a dict(samples = the N images
folded in order, params = the parameter sets the estimate is run with).  Deterministic in (family, h, w, K)."""
import functools

import numpy as np

import robust_inputs as ri

f32 = np.float32
SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 17), (24, 40), (70, 53)]      # (w, h)
GPU_SIZES = SIZES + [(200, 131)]
BUCKETS = ri.BUCKETS
# of robust_inputs: everything but "short" (N < K: refused).  N = K: "full", "outlier", ...; N = K + 1: "gain_zero", "gain_huge"; N = 2 K + 3: "ragged"
BORROWED = tuple(f for f in ri.FAMILIES if f != "short")
OWN = ("negative", "edge", "edge_above")
FAMILIES = BORROWED + OWN
EDGE_FLOOR = 2.0 ** -5


def grey(v):
    """planes of colour (v, v, v, 1): the luminance is v exactly"""
    v = np.asarray(v, f32)
    return np.stack([v, v, v, np.ones_like(v)], -1).astype(f32)


def edge_keys(K):
    """K keys, bucket order = rank order, for a huge gain (t at its cap, h = 2): the two middle keys 0.9375 and 1, so that with floor 2^-5
    mw = mu = 0.96875, den = 1, D = K / 4 * 2^-8, v = D / 2 and e = K / 8 * 2^-8; the others are dropped and winsorized"""
    half = K // 2
    return [f32(0.25 + j / 64) for j in range(half - 1)] + [f32(0.9375), f32(1.0)] + [f32(2 + j) for j in range(half - 1)]


def moved(v, ulps):
    return (f32(v).view(np.uint32).astype(np.int64) + np.asarray(ulps, np.int64)).astype(np.uint32).view(f32)


@functools.lru_cache(maxsize=None)
def edge_solution(K):
    """((m_lo, m_hi), (m_lo', m_hi'), threshold): the two middle keys moved by m ulps give a pixel error e0 that is threshold threshold
    exactly (binary32), moved by m' ulps they give e0 + 256 ulps: 256 pixels of e0 make a tile's mse e0, 255 of e0 and one of the other
    make it one ulp more, every partial sum of the tree being exact.  Found by search through the mirror, the nearest such pair."""
    import robust_error_mirror as rem
    span = np.arange(-48, 49)
    n = len(span)
    planes = np.zeros((K, n, n, 4), f32)
    for j, k in enumerate(edge_keys(K)):
        planes[j] = grey(np.full((n, n), k, f32))
    planes[K // 2 - 1] = grey(np.broadcast_to(moved(0.9375, span)[:, None], (n, n)))
    planes[K // 2] = grey(np.broadcast_to(moved(1.0, span)[None, :], (n, n)))
    e, _ = rem.pixel_error(planes, K, gain=1e30, floor=EDGE_FLOOR)
    root = np.sqrt(e.astype(np.float64)).astype(f32)
    cost = np.abs(span)[:, None] + np.abs(span)[None, :]
    bits = e.view(np.uint32)
    T = np.stack([moved(root, -1), root, moved(root, 1)])
    square = (T * T == e)                                          # (3, n, n): a binary32 whose square is e exactly
    exact = square.any(0) & ((bits + 256) >> 23 == bits >> 23)     # ... and e0 + 256 ulps in e0's binade
    reachable = set(bits.ravel().tolist())
    hits = [(int(cost[a, b]), int(a), int(b)) for a, b in np.argwhere(exact) if int(bits[a, b]) + 256 in reachable]
    assert hits, "no nudge of the middle keys puts a tile on the threshold"
    _, a, b = min(hits)
    above = np.argwhere(bits == bits[a, b] + 256)
    c, d = above[np.argmin(cost[above[:, 0], above[:, 1]])]
    threshold = float(T[np.argmax(square[:, a, b]), a, b])
    return (int(span[a]), int(span[b])), (int(span[c]), int(span[d])), threshold


def make(family, h, w, K):
    assert family in FAMILIES and K in BUCKETS
    if family in BORROWED:
        case = ri.make(family, h, w, K)
        params = [dict(gain=g) for g in case["gains"]]
        if family == "outlier":                                    # at gain 1 the outlier is winsorized to the rest: e = 0; at gain 0 it is not
            params = [dict(gain=1.0), dict(gain=0.0)]
        if family == "specials":
            params = [dict(gain=1.0), dict(gain=3.0, threshold=0.5, floor=0.25, quantile_permille=500)]
        return dict(samples=case["samples"], params=params)
    rng = ri.rng_of(family, h, w, K)
    if family == "negative":                                       # every key negative, mu <= 0: den is the floor alone
        samples = ri.noisy(rng, h, w, K + 1, firefly=0.0)
        samples = [np.concatenate([-s[..., :3], s[..., 3:]], -1).astype(f32) for s in samples]
        samples[0][h // 2, w // 2, :3] = 0                         # (mu == 0 somewhere: every bucket black)
        for s in samples[1:]:
            s[h // 2, w // 2, :3] = 0
        params = [dict(gain=1.0), dict(gain=0.0, floor=0.5)]
    else:                                                          # "edge": every pixel's e is threshold^2 exactly; "edge_above": one pixel per tile 256 ulps more
        at, above, threshold = edge_solution(K)
        keys = edge_keys(K)
        keys[K // 2 - 1], keys[K // 2] = moved(0.9375, at[0]), moved(1.0, at[1])
        samples = [grey(np.full((h, w), k, f32)) for k in keys]
        if family == "edge_above":
            for y in range(3, h, 16):
                for x in range(5, w, 16):
                    samples[K // 2 - 1][y, x, :3] = moved(0.9375, above[0])
                    samples[K // 2][y, x, :3] = moved(1.0, above[1])
        params = [dict(gain=1e30, floor=EDGE_FLOOR, threshold=threshold)]
    for s in samples:
        s.setflags(write=False)
    return dict(samples=samples, params=params)


def listed_cases():
    """(family, (w, h), K): every case of the CPU module; the GPU module adds 200 x 131"""
    return [(f, s, K) for f in FAMILIES for s in SIZES for K in BUCKETS]
