"""Input families for rtgl_denoise that no renderer produces, and the list of cases run on them.  A helper, not a test.

tests/test_denoise_inputs.py pins the numpy restatement (tests/denoise_mirror.py) on these inputs and proves that each family catches the
defects it is there for; tests/test_gpu_denoise_inputs.py puts the same arrays in front of the kernel.  Every generator is deterministic
and returns (image, albedo, normal, position) as float32 (H, W, 4), filled over the whole array: the margin outside the 8 x 8 dispatch
footprint of a ragged image, which a rendered frame leaves at zero, carries data like every other pixel."""
import numpy as np

f32 = np.float32
FLOOR = f32(2.0 ** -10)


def _bits(*words):
    return np.array(words, np.uint32).view(f32)


# what a rendered image never holds.  Two NaNs: the default quiet one and a negative one with a payload.
NANS = _bits(0x7FC00000, 0xFFC12345)
COMMON = np.concatenate([NANS, np.array([np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 3e38, -1.5, 65504.0], f32)])
ALBEDO_EXTRA = np.array([0.0, FLOOR, np.nextafter(FLOOR, f32(0)), np.nextafter(FLOOR, f32(1)), -1.0], f32)
NORMAL_EXTRA = np.array([1e20], f32)
# t: sigma_position t squared underflows to 0 (1e-30), to a subnormal whose reciprocal overflows (1e-20, 1e-18) or is finite (1.5e-18,
# at the default 0.05), or overflows (1e20 and the common 3e38)
T_EXTRA = np.array([0.0, -1.0, 1e-30, 1e-20, 1e-18, 1.5e-18, 1e20], f32)
# colours_finite: |colour| <= 65504, albedo in (0, 1] plus the two neighbours of the floor
IMAGE_FINITE = np.array([0.0, -0.0, 1e-40, -1e-40, -1.5, 65504.0], f32)
ALBEDO_FINITE = np.array([FLOOR, np.nextafter(FLOOR, f32(0)), np.nextafter(FLOOR, f32(1)), 1.0, 1e-40, 0.5], f32)
SHARE = 0.15


def benign(H, W, seed):
    """random_inputs of tests/test_denoise_mirror.py: colours in [0, 2), albedo in [0, 1) with one pixel below the divisor's floor, normals
    nearly parallel so that the term stays open, t = 4 + z with one miss (t = 0)"""
    rng = np.random.default_rng(seed)
    img = rng.random((H, W, 4), dtype=f32) * f32(2)
    alb = rng.random((H, W, 4), dtype=f32)
    alb[0, 0, :3] = 0
    nrm = np.zeros((H, W, 4), f32)
    n = rng.normal(size=(H, W, 3))
    nrm[..., :3] = (n / np.linalg.norm(n, axis=2, keepdims=True) * 0.1 + np.array([0, 0, 1.0])).astype(f32)
    pos = rng.random((H, W, 4), dtype=f32)
    pos[..., 3] = 4 + pos[..., 2]
    pos[H // 2, W // 2] = 0
    return img, alb, nrm, pos


def _sprinkle(a, channels, values, rng):
    """One component of a share of the pixels of `a` is replaced: the k-th chosen pixel takes values[k mod n] in a random one of
    `channels`.  The share is SHARE of the pixels, and never fewer pixels than there are values (as far as the array has that many), so
    that every value occurs at every size of at least 64 pixels."""
    H, W = a.shape[:2]
    count = min(H * W, max(int(np.ceil(SHARE * H * W)), len(values)))
    where = rng.permutation(H * W)[:count]
    ch = rng.integers(0, len(channels), count)
    flat = a.reshape(H * W, 4)
    flat[where, np.asarray(channels)[ch]] = values[np.arange(count) % len(values)]


def specials(H, W, seed, colours_finite=False):
    """benign with NaN, +-inf, +-0, +-1e-40, 3e38, -1.5, 65504 over 15 % of the pixels of every array; the albedo also takes 0, 2^-10, its two
    neighbours and -1, the normal 1e20, t the values of T_EXTRA.  colours_finite: image and albedo stay finite and moderate (the family for
    parameter sets with the colour term off, where one non-finite colour would spread over the image)."""
    img, alb, nrm, pos = benign(H, W, seed)
    rng = np.random.default_rng(seed + 1000)
    _sprinkle(img, (0, 1, 2, 3), IMAGE_FINITE if colours_finite else COMMON, rng)
    _sprinkle(alb, (0, 1, 2), ALBEDO_FINITE if colours_finite else np.concatenate([COMMON, ALBEDO_EXTRA]), rng)
    _sprinkle(nrm, (0, 1, 2), np.concatenate([COMMON, NORMAL_EXTRA]), rng)
    _sprinkle(pos, (0, 1, 2), np.concatenate([COMMON, NORMAL_EXTRA]), rng)
    _sprinkle(pos, (3,), np.concatenate([COMMON, T_EXTRA]), rng)
    return img, alb, nrm, pos


# subnormal_weights: the two parameter sets it is built for
SW_COLOUR_OFF = dict(sigma_color=0.0, sigma_normal=0.5, sigma_position=1.0, demodulate=False)
SW_ALL_ON = dict(sigma_color=1e19, sigma_normal=0.5, sigma_position=1.0, demodulate=True)
SW_BASE, SW_HOT = f32(1e-19), f32(1e19)


def subnormal_weights_hot(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx % 5 == 2) & (yy % 3 == 0)


def subnormal_weights(H, W):
    """Taps whose weight is a subnormal number and still matters.  Every pixel has N = (0, 0, 1), P = 0, t = 1, albedo 1 and a colour
    around 1e-19, except the hot pixels (x mod 5 = 2, y mod 3 = 0: every 64-column block has them, and with y mod 3 they fall into every wave
    of a block): N.x = nextafter(1, 0), P.x = fl(sqrt(4 - 2^-8)), colour 1e19.  With sigma_normal = 0.5 and sigma_position = 1 a tap
    between a hot pixel and a neighbour has a normal factor of (2^-23)^4 and a position factor of about (2^-10)^4, so
    w = h[j] h[i] 2^-92 2^-40 = 1.7e-41 at distance one and 4.3e-42 at distance two: subnormal, and w 1e19 is about one per cent of
    the 1.4e-20 the pixel's own tap contributes.  A kernel that flushes w to zero is off by that much.  With the colour term on at
    sigma_color = 1e19 (SW_ALL_ON) the factor of such a tap is (3/4)^4 in the first pass and ic = 1e-38 is itself subnormal."""
    yy, xx = np.mgrid[0:H, 0:W]
    hot = subnormal_weights_hot(H, W)
    img = np.ones((H, W, 4), f32)
    for k in range(3):
        img[..., k] = SW_BASE * (f32(1) + ((xx * 7 + yy * 13 + k * 5) % 16).astype(f32) / f32(16))
    img[hot, :3] = SW_HOT
    alb = np.ones((H, W, 4), f32)
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., 2] = 1
    nrm[hot, 0] = np.nextafter(f32(1), f32(0))
    pos = np.zeros((H, W, 4), f32)
    pos[..., 3] = 1
    pos[hot, 0] = np.sqrt(f32(4) - f32(2.0 ** -8), dtype=f32)
    return img, alb, nrm, pos


# ramps: the two parameter sets it is built for.  Wide open: the factors stay near 1 up to step 128 and still depend on every plane.
RAMPS_OFF = dict(sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0, demodulate=False)
RAMPS_OPEN = dict(sigma_color=1e6, sigma_normal=100.0, sigma_position=100.0, demodulate=True)


def ramps(H, W):
    """Every pixel distinct and coded by its position with small integers (exact in binary32): colour (x, y, (31 x + 17 y) mod 64), and the
    planes likewise.  A tap from the wrong column or row, from a stale LDS word or from across the image border is off by whole units."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([xx, yy, (31 * xx + 17 * yy) % 64, 1 + (xx + 2 * yy) % 5], -1).astype(f32)
    alb = np.stack([1 + xx % 3, 1 + yy % 4, 1 + (xx + yy) % 2, 1 + 0 * xx], -1).astype(f32) * f32(0.25)
    nrm = np.stack([xx % 7, yy % 5, (xx + yy) % 3, 0 * xx], -1).astype(f32)
    pos = np.stack([xx, yy, (xx ^ yy) & 7, 8 + (xx + yy) % 4], -1).astype(f32)
    return img, alb, nrm, pos


FAMILIES = ("benign", "specials", "subnormal_weights", "ramps")


def make(family, H, W, params, seed=0):
    """The arrays of a family for a parameter set: specials keeps the colours finite exactly when the set has the colour term off"""
    if family == "benign":
        return benign(H, W, seed + 31 * H + W)
    if family == "specials":
        return specials(H, W, seed + 31 * H + W, colours_finite=params.get("sigma_color", 16.0) <= 0)
    if family == "subnormal_weights":
        return subnormal_weights(H, W)
    if family == "ramps":
        return ramps(H, W)
    raise ValueError(family)


def nan_budget(family, params):
    """The share of the output's components that may be NaN in the restatement (rtgl_denoise leaves sign and payload of a NaN open, so the
    comparison cannot see into one: the budget keeps that from hiding a failure).  With the colour term on a NaN or infinite colour has
    weight 0 for every other pixel, so the NaN outputs are about the NaN inputs: at most 2 % of the components.  Where the inputs hold no
    non-finite colour there is none."""
    return 0.02 if family == "specials" and params.get("sigma_color", 16.0) > 0 else 0.0


# ------------------------------------------------------------------------------------------------------------------------ the cases
# (width, height) everywhere below

# values
VALUE_SIZES = [(70, 53), (200, 131)]
VALUE_PASSES = (0, 1, 5, 8)
SPECIALS_PARAMS = [dict(),                                                              # defaults
                   dict(sigma_color=0.5, sigma_normal=0.1, sigma_position=0.01),        # every term on, small sigmas
                   dict(sigma_normal=0.0, sigma_position=0.0),                          # each term alone
                   dict(sigma_color=0.0, sigma_position=0.0),
                   dict(sigma_color=0.0, sigma_normal=0.0),
                   dict(demodulate=False),
                   dict(sigma_color=0.0)]                                               # colour term off
VALUE_PARAMS = {"specials": SPECIALS_PARAMS, "subnormal_weights": [SW_COLOUR_OFF, SW_ALL_ON]}

# sizes: each width with at least three heights and each height with at least three widths.  A block takes 64 columns and four rows
# `step` apart and the rows come in chunks of 4 step, so for step s the edges are at heights around 4 s (3, 4, 5 for s = 1; 9 for 2; 31, 33
# for 8; 127, 129 for 32; 513 for 128) and at widths around the multiples of 64.  The first block's segment starts at -2 s for every step
# and the last block's ends beyond the width at every width; at 257, 321 and 577 the taps at +-128 and +-256 also land inside the image, in
# other blocks.  The product is thinned by cost, which is the mirror's and goes with the pixels: the tall cases are narrow and the wide ones
# low (a first list with 257 x 513, 577 x 129 and 321 x 129 took 22 s of the module's 59 s); WIDE_SIZE below is the case that is both.
# NARROW_HEIGHTS adds the remaining heights below, at and above 4 s at a width of two blocks, where they cost little.
SIZE_CASES = [(1, 1), (1, 5), (1, 513), (2, 2), (2, 33), (2, 129), (3, 3), (3, 9), (3, 127), (3, 513), (63, 4), (63, 31), (63, 127),
              (64, 1), (64, 33), (64, 129), (65, 5), (65, 127), (65, 513), (127, 2), (127, 9), (127, 129), (129, 3), (129, 5), (129, 31),
              (257, 4), (257, 33), (257, 127), (321, 3), (321, 5), (321, 9), (321, 33), (577, 1), (577, 2), (577, 4), (577, 31)]
NARROW_HEIGHTS = [(65, h) for h in (7, 8, 15, 16, 17, 32, 63, 64, 65, 128, 255, 256, 257, 511, 512)]
SIZE_PASSES = (1, 2, 3, 4, 5, 6, 7, 8)
BENIGN_OPEN = dict(sigma_color=1e6, sigma_position=1.0)        # benign's colours and positions are random: open enough for the far taps
SIZE_RUNS = [("ramps", RAMPS_OFF), ("ramps", RAMPS_OPEN), ("benign", BENIGN_OPEN)]

# wide steps with their far taps inside the image
WIDE_SIZE = (700, 530)
WIDE_PASSES = (6, 7, 8)
WIDE_RUNS = [("ramps", RAMPS_OFF), ("ramps", RAMPS_OPEN), ("specials", dict())]


def listed_cases():
    """every (family, (width, height), parameter set with passes) the GPU module runs on generated inputs"""
    out = []
    for size in VALUE_SIZES:
        for family, sets in VALUE_PARAMS.items():
            out += [(family, size, dict(ps, passes=k)) for ps in sets for k in VALUE_PASSES]
    for size in SIZE_CASES:
        out += [(family, size, dict(ps, passes=k)) for family, ps in SIZE_RUNS for k in SIZE_PASSES]
    out += [("ramps", size, dict(RAMPS_OFF, passes=k)) for size in NARROW_HEIGHTS for k in SIZE_PASSES]
    out += [(family, WIDE_SIZE, dict(ps, passes=k)) for family, ps in WIDE_RUNS for k in WIDE_PASSES]
    return out
