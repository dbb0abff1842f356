"""Inputs of the robust-adaptive tests (tests/test_robust_adaptive_mirror.py without a GPU, tests/test_gpu_robust_adaptive.py on the device):
named cases, each a list of steps a session is driven through, deterministic in (name, h, w, K).

A step is one of
    ("mask", tiles)     an explicit mask (ty, tx)
    ("fold", image)     the fold with `image` (h, w, 4) as the source: rtgl_write_image_f32 + rtgl_robust_adaptive_accumulate on the device
    ("update",)         rtgl_robust_adaptive_update: records, mask and summary are compared
    ("tamper",)         every tile record is overwritten with SENTINEL behind the session's back (on the device through
                        rtgl_device_robust_adaptive_tiles): a tile with n == m must keep it
    ("resolve",)        the resolve into both destinations with every gain of the case
and run(case, session) drives tests/robust_adaptive_mirror.py's Session through them (the CPU module, and the expected values of the GPU
module).  `injected` (h, w) marks the pixels that received values of a special family of tests/robust_inputs.py: at most a quarter."""
import zlib

import numpy as np

import adaptive_mirror as am
import robust_inputs as ri

f32 = np.float32
SIZES = [(1, 1), (7, 7), (8, 8), (16, 16), (24, 40), (70, 53), (130, 9)]      # (w, h)
BUCKETS = (4, 8, 16)
GAINS = (0.0, 1.0, 1e30)
UNIFORM = ("uniform-1", "uniform-K-1", "uniform-K", "uniform-K+1", "uniform-2K+3")
MASKED = ("counts", "checker", "one", "none", "stale")
SPECIAL = ("specials", "nonfinite", "ties", "equal", "outlier", "integer_u", "overflow", "negative_subnormal")
NAMES = UNIFORM + MASKED + SPECIAL
SENTINEL = (f32(-7.5), f32(3.25), 0xABCD, 7, 0x1234, 0x4321)      # sum, mse, count, converged, samples, samples_snapshot

# the seeded defects of tests/test_robust_adaptive_mirror.py and the case that catches each
DEFECT_CASES = {
    "k_is_n": "counts",                  # k = n div K replaced by n
    "j_from_frame_count": "counts",      # j from the number of folds of the session, not from n[t]
    "nj_from_largest_n": "counts",       # the resolve's n_j from the largest n of the picture
    "t_not_zeroed": "counts",            # t not zeroed while N < K
    "outside_is_nan": "counts",          # a pixel outside the footprint (or of a tile without a sample) resolved as 0 / 0
    "m_not_updated": "stale",            # m stays what it was: the tile is estimated again by the next update
    "stale_reestimated": "stale",        # a tile with n == m estimated again
    "short_marked_valid": "counts",      # the n < K record marked valid
}


def uniform_count(name, K):
    return {"uniform-1": 1, "uniform-K-1": K - 1, "uniform-K": K, "uniform-K+1": K + 1, "uniform-2K+3": 2 * K + 3}[name]


def params_of(K):
    """a threshold the noisy pictures straddle, min_samples = K and a cap the longest case reaches"""
    return dict(buckets=K, threshold=0.25, floor=0.01, gain=1.0, min_samples=K, max_samples=2 * K + 3)


def rng_of(name, h, w, K):
    return np.random.default_rng(zlib.crc32(f"robust adaptive {name} {h} {w} {K}".encode()))


def named_masks(h, w):
    s = am.shape(h, w)
    ty, tx = s["ty"], s["tx"]
    checker = (np.add.outer(np.arange(ty), np.arange(tx)) % 2).astype(np.uint8)
    one = np.zeros((ty, tx), np.uint8)
    one[ty // 2, tx // 2] = 1
    return dict(all=np.ones((ty, tx), np.uint8), checker=checker, inverse=(1 - checker).astype(np.uint8), one=one, none=np.zeros((ty, tx), np.uint8))


def target_counts(h, w, K):
    """(ty, tx): 0, 1, K - 1, K, K + 1 and 2 K + 3 dealt to the tiles in turn, the order rotated so that the single tile of a small picture
    is estimated"""
    s = am.shape(h, w)
    values = np.array([K + 1, 2 * K + 3, 0, 1, K - 1, K])
    return values[np.arange(s["ty"] * s["tx"]) % 6].reshape(s["ty"], s["tx"])


def make(name, h, w, K):
    """dict(params, steps, gains, injected)"""
    assert name in NAMES and K in BUCKETS
    rng = rng_of(name, h, w, K)
    masks = named_masks(h, w)
    injected = np.zeros((h, w), bool)
    gains = list(GAINS)
    steps = []
    if name in UNIFORM:
        steps = [("fold", img) for img in ri.noisy(rng, h, w, uniform_count(name, K))] + [("update",), ("resolve",)]
    elif name == "counts":
        # a tile with target c joins for the LAST c folds: its count differs from the session's fold count, and one picture ends with
        # tiles at 0, 1, K - 1, K, K + 1 and 2 K + 3
        total, target = 2 * K + 3, target_counts(h, w, K)
        for k, img in enumerate(ri.noisy(rng, h, w, total, firefly=0.1)):
            steps += [("mask", (target >= total - k).astype(np.uint8)), ("fold", img)]
            if k in (K, total - 2):
                steps += [("update",), ("resolve",)]
        steps += [("update",), ("resolve",)]
    elif name == "checker":
        order = ("checker", "inverse", "checker", "all", "one", "none", "inverse")
        for k, img in enumerate(ri.noisy(rng, h, w, K + 4)):
            steps += [("mask", masks[order[k % len(order)]]), ("fold", img)]
        steps += [("update",), ("resolve",)]
    elif name in ("one", "none"):
        for img in ri.noisy(rng, h, w, K + 1):
            steps += [("mask", masks[name]), ("fold", img)]
        steps += [("update",), ("resolve",)]
    elif name == "stale":
        imgs = ri.noisy(rng, h, w, 2 * K + 2)
        steps = [("fold", img) for img in imgs[:K]] + [("update",), ("tamper",), ("update",)]      # nothing moved: every record keeps the sentinel
        steps += [("mask", masks["checker"])] + [("fold", img) for img in imgs[K:K + 2]] + [("update",), ("resolve",)]      # the checker's tiles are estimated again
        steps += [("tamper",), ("mask", masks["one"]), ("fold", imgs[K + 2]), ("update",), ("update",), ("resolve",)]
    else:
        family = {"negative_subnormal": "specials"}.get(name, name)
        special = ri.make(family, h, w, K)
        count = len(special["samples"])
        base = ri.noisy(rng_of(name + " base", h, w, K), h, w, count, firefly=0.0)
        pick = np.zeros(h * w, bool)
        pick[rng.permutation(h * w)[:h * w // 4]] = True
        injected = pick.reshape(h, w)
        if name == "negative_subnormal":                           # finite values only: negative, subnormal and signed zeros
            values = (-0.0, 0.0, 1.0e-40, -1.0e-42, -1.5, -0.75, 1.0e-45)
            special = dict(samples=[np.array(values, f32)[rng.integers(0, len(values), (h, w, 4))] for _ in range(count)], gains=[1.0])
        steps = [("fold", np.where(injected[..., None], sp, b).astype(f32)) for sp, b in zip(special["samples"], base)] + [("update",), ("resolve",)]
        gains = sorted(set(gains) | set(special["gains"]))
    for step in steps:
        if len(step) > 1:
            step[1].setflags(write=False)
    return dict(name=name, params=params_of(K), steps=steps, gains=gains, injected=injected)


def tamper(session):
    """what ("tamper",) does to the mirror's session"""
    for key, value in zip(("sum", "mse", "count", "converged", "samples", "samples_snapshot"), SENTINEL):
        session.records[key] = value


def run(case, session, on_step=None):
    """drives `session` (robust_adaptive_mirror.Session or anything with its methods) through the case; on_step(index, step, result) after
    every step, result = the summary of an update or {(gain, dest): picture} of a resolve"""
    for index, step in enumerate(case["steps"]):
        result = None
        if step[0] == "mask":
            session.set_mask(step[1])
        elif step[0] == "fold":
            session.fold(step[1])
        elif step[0] == "update":
            result = session.update()
        elif step[0] == "tamper":
            session.tamper() if hasattr(session, "tamper") else tamper(session)
        else:
            result = {(gain, dest): session.resolve(gain, dest) for gain in case["gains"] for dest in (0, 1)}
        if on_step:
            on_step(index, step, result)


def invalid_params():
    """overrides of the defaults, each of which makes the parameter record invalid (RTGL_ERR_INVALID at rtgl_robust_adaptive_begin)"""
    nan, inf = float("nan"), float("inf")
    return ([dict(buckets=k) for k in (0, 1, 2, 3, 5, 7, 9, 12, 15, 17, 32, 0xFFFFFFFF)] + [dict(threshold=v) for v in (nan, inf, 0.0, -0.05)]
            + [dict(floor=v) for v in (nan, inf, 0.0, -0.01)] + [dict(gain=v) for v in (nan, inf, -inf, -1.0, -1e-30)]
            + [dict(min_samples=7), dict(min_samples=0), dict(buckets=16, min_samples=15), dict(min_samples=33, max_samples=32), dict(max_samples=0),
               dict(max_samples=16777217), dict(max_samples=0xFFFFFFFF), dict(flags=1), dict(flags=0x80000000), dict(reserved=1), dict(reserved=0x80000000)])


def listed_cases():
    """(name, (w, h), K): every case of the CPU module"""
    return [(name, size, K) for name in NAMES for size in SIZES for K in BUCKETS]
