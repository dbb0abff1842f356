"""Inputs of the robust-denoise tests (tests/test_robust_denoise_mirror.py without a GPU, tests/test_gpu_robust_denoise.py on the device).
A helper, not a test.  A case is dict(samples = the N one-sample images folded in order (the buckets are injected the way
tests/robust_inputs.py does it: write_image, then robust_accumulate), albedo, normal, position = the first-hit planes (injected as
tests/test_gpu_denoise_inputs.py does it, through tensors over rtgl_device_aov), params = the parameter sets the call is run with).
Deterministic in (buckets family, guides family, h, w, K)."""
import numpy as np

import denoise_inputs as di
import robust_error_inputs as rei
import robust_inputs as ri

f32 = np.float32
SIZES = [(1, 1), (3, 2), (64, 4), (65, 5), (70, 53), (130, 9)]       # (w, h): below a tile, a tile, one column and one row past it, many tiles
BUCKETS = ri.BUCKETS
# bucket families: those of robust_error_inputs that fill every bucket (N = K: "full", "outlier", "ties", "overflow", "nonfinite",
# "integer_u"; N = K + 1: "gain_zero", "gain_huge", "negative"; N = 2 K: "equal"; N = 2 K + 1: "specials"; N = 2 K + 3: "ragged") and
# "long" (N = 3 K + 2).  t = 0: "equal", "gain_zero"; t at its cap: "overflow", "gain_huge".  Subnormal, negative, infinite and NaN
# values: "specials", "negative", "nonfinite".
BUCKET_FAMILIES = ("full", "gain_zero", "long", "ragged", "specials", "ties", "equal", "outlier", "integer_u", "gain_huge", "overflow", "nonfinite", "negative")
SPECIAL_FAMILIES = ("specials", "ties", "equal", "overflow", "nonfinite", "negative", "gain_huge", "gain_zero")
GUIDE_FAMILIES = ("benign", "specials", "edges", "flat")
PASSES = (0, 1, 5)
HUGE = 1e30


def nan_budget(planes, albedo=None):
    """The share of the mirror's components that may be NaN (the contract leaves a NaN's sign and payload open, so the comparison cannot
    see into one; the budget keeps that from hiding a failure).  It is worked out from the inputs alone: a NaN comes out of a pixel only
    if one of ITS OWN bucket values or albedos is not finite, or so large (>= 1e30) that a sum of K of them overflows and meets an
    infinity of the other sign.  It does not travel: v0 is made finite by step 5, the luminance term gives a tap whose luminance
    difference is not a number the weight 0, so does a geometric factor that is not a number, and a pixel whose own weights are all 0
    keeps its own value.  No family holds finite luminances above 1e18, whose squares would overflow the filtered variance.  So the share
    of NaN components is at most the share of such pixels."""
    planes = np.asarray(planes, f32)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(planes) < f32(HUGE)).all(axis=(0, -1))
        if albedo is not None:
            bad |= ~(np.abs(np.asarray(albedo, f32)[..., :3]) < f32(HUGE)).all(-1)
    return float(bad.mean())


def samples_of(family, h, w, K):
    """(samples, gains)"""
    if family == "long":
        return ri.noisy(ri.rng_of("long", h, w, K), h, w, 3 * K + 2), [1.0, 4.0]
    case = rei.make(family, h, w, K)
    return case["samples"], sorted({p.get("gain", 1.0) for p in case["params"]})


def guides_of(family, h, w, seed=0):
    """(albedo, normal, position) float32 (h, w, 4)"""
    if family in ("benign", "specials"):
        _, alb, nrm, pos = di.make(family, h, w, {}, seed)
        return alb, nrm, pos
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(77 + 31 * h + w + seed)
    alb = (rng.random((h, w, 4), dtype=f32) * f32(0.9) + f32(0.1)).astype(f32)
    nrm = np.zeros((h, w, 4), f32)
    pos = np.zeros((h, w, 4), f32)
    pos[..., 3] = 4
    if family == "flat":                                           # constant guides: every neighbour is near
        nrm[..., 2] = 1
        alb[...] = f32(0.5)
        return alb, nrm, pos
    assert family == "edges"
    # two surfaces at right angles and far apart: edges exactly on the borders of the 64 x 4 tiles, and a diagonal band through them
    side = (((xx // 64) + (yy // 4)) % 2) ^ (((xx + 2 * yy) % 11) < 4)
    nrm[..., 2] = (side == 0)
    nrm[..., 0] = (side == 1)
    pos[..., 0] = xx * f32(0.01)
    pos[..., 1] = yy * f32(0.01)
    pos[..., 2] = side * f32(10)
    pos[(yy % 7 == 3) & (xx % 5 == 1), 3] = 0                      # misses: ip = 0
    return alb, nrm, pos


PARAM_SETS = [dict(),                                                                  # defaults: every term on, demodulating
              dict(demodulate=False),
              dict(sigma_normal=0.0),                                                  # each geometric term off in turn
              dict(sigma_position=0.0, demodulate=False),
              dict(sigma_lum=0.5, sigma_normal=0.1, sigma_position=0.01)]


def make(buckets, guides, h, w, K, sets=None):
    """sets: indices into PARAM_SETS (default: all); the family's gains go round them"""
    assert buckets in BUCKET_FAMILIES and guides in GUIDE_FAMILIES and K in BUCKETS
    samples, gains = samples_of(buckets, h, w, K)
    alb, nrm, pos = guides_of(guides, h, w)
    sets = range(len(PARAM_SETS)) if sets is None else sets
    params = [dict(PARAM_SETS[s], gain=gains[i % len(gains)]) for i, s in enumerate(sets)]
    return dict(samples=samples, albedo=alb, normal=nrm, position=pos, params=params)


FULL_SIZES = ((65, 5), (70, 53))


def listed_cases():
    """(buckets, guides, (w, h), K, sets): the injected cases of the GPU module.  Every bucket family at 65 x 5 and 70 x 53, a third of
    them (taking turns) at the other sizes; the guide families and the parameter sets take turns over them."""
    out = []
    for si, (w, h) in enumerate(SIZES):
        for ki, K in enumerate(BUCKETS):
            families = BUCKET_FAMILIES if (w, h) in FULL_SIZES else BUCKET_FAMILIES[(si + ki) % 3::3]
            for fi, family in enumerate(families):
                out.append((family, GUIDE_FAMILIES[(fi + si + ki) % 4], (w, h), K, ((fi + ki) % 5, (fi + ki + 2) % 5)))
    return out


def normal_buckets(h, w, K, N, mean, sigma_left, sigma_right, seed=0):
    """N = m K samples whose bucket means are i.i.d. normal about `mean` with standard deviation sigma_left in the left half of the
    picture and sigma_right in the right half: every sample of bucket j is that bucket's mean (a mean of equal values is the value)"""
    assert N % K == 0
    rng = np.random.default_rng(4242 + seed)
    sigma = np.where(np.arange(w)[None, :] < w // 2, sigma_left, sigma_right)
    means = [(mean + sigma * rng.standard_normal((h, w))).astype(f32) for _ in range(K)]
    return [rei.grey(means[k % K]) for k in range(N)]


def checker_case(h=64, w=64, K=8, rounds=4, grey=0.5, amplitude=0.02, sigma_mean=0.002, seed=0):
    """the purpose case: a flat grey with a one-pixel checker of +-amplitude under bucket noise whose mean has the standard deviation
    sigma_mean; constant guides.  Returns (samples, truth (h, w, 4), albedo, normal, position)"""
    yy, xx = np.mgrid[0:h, 0:w]
    truth = (grey + amplitude * np.where((xx + yy) % 2 == 0, 1.0, -1.0)).astype(f32)
    rng = np.random.default_rng(2025 + seed)
    sigma_sample = sigma_mean * np.sqrt(K * rounds)
    samples = [rei.grey((truth + sigma_sample * rng.standard_normal((h, w))).astype(f32)) for _ in range(K * rounds)]
    alb, nrm, pos = guides_of("flat", h, w)
    return samples, rei.grey(truth), alb, nrm, pos
