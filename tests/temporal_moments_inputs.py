"""The sequences rtgl_temporal_accumulate is run on with option "temporal_moments" set.  A helper, not a test.
tests/test_temporal_moments_mirror.py pins the restatement on them; tests/test_gpu_temporal_moments.py puts the same arrays in front of
the kernels.

The families, SIZES and PARAMETER_SETS are those of tests/temporal_inputs.py, unchanged, except `specials`; every item gets an albedo
plane as its fifth element: (image, normal, position, camera, albedo).

Why `specials_sq` stands in for `specials`: the luminance is squared.  A pixel holding 3e38 gives m2 = inf, and the next blend computes
inf + (x - inf) al = NaN.  With one pixel in twelve of the image holding a COLD value, a seventh of those 3e38, the NaN share of the moments
buffer passes the project's 2 % cap (NAN_CAP), which is the condition under which "a NaN for a NaN" cannot hide a failure.  specials_sq
replaces COLD's 3e38 by 1e18 (its square, 1e36, and sums of a few of them stay finite) and strews 3e38 itself like the HOT values (NaN and
the infinities, which temporal_inputs.specials puts into one pixel of 3000): into one image component of one pixel in 3000 per call."""
import numpy as np

import temporal_inputs as ti

f32 = np.float32
SIZES, PARAMETER_SETS, NAN_CAP = ti.SIZES, ti.PARAMETER_SETS, ti.NAN_CAP
MODES = (1, 2)
ALBEDO_FLOOR = 2.0 ** -10
LOW = [0.0, ALBEDO_FLOOR, -0.25, 1e-40, 2.0 ** -11, -0.0]                  # albedo components at or below the floor: the divisor is the floor


def albedo_plane(H, W, seed):
    """a smooth positive texture in [0.2, 1], different per channel, with about one pixel in twelve holding a component at or below 2^-10"""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    a = np.stack([0.6 + 0.4 * np.sin(0.11 * x + 0.7 * c) * np.cos(0.07 * y - 0.4 * c) for c in range(3)] + [np.ones((H, W))], -1).astype(f32)
    rng = np.random.default_rng(seed + 101)
    n = H * W
    flat = a.reshape(n, 4)
    for k, p in enumerate(rng.choice(n, size=(n + 11) // 12, replace=False)):
        flat[p, int(rng.integers(3))] = f32(LOW[k % len(LOW)])
    return a


HUGE = 3e38                     # finite, and its square is not: m2 = inf beside a finite m1


def specials_sq(H, W, seed=0):
    """temporal_inputs.specials with every 3e38 (COLD's, one pixel in about 84 of each array) replaced by 1e18, and 3e38 kept among the hot
    values instead: one image component in 3000 pixels per call (see the module's text)"""
    rng = np.random.default_rng(seed + 13)
    out = []
    for image, normal, position, c in ti.specials(H, W, seed):
        image, normal, position = (np.where(a == f32(HUGE), f32(1e18), a).astype(f32) for a in (image, normal, position))
        n = H * W
        flat = image.reshape(n, 4)
        for p in rng.choice(n, size=n // 3000, replace=False):
            flat[p, int(rng.integers(3))] = f32(HUGE)
        out.append((image, normal, position, c))
    return out


FAMILIES = {k: v for k, v in ti.FAMILIES.items() if k != "specials"}
FAMILIES["specials_sq"] = specials_sq


def make(family, H, W, seed=0):
    """the family's sequence with an albedo plane per item (a new one per call, like a plane that follows the camera)"""
    return [item + (albedo_plane(H, W, seed + k),) for k, item in enumerate(FAMILIES[family](H, W, seed))]


def nan_budget(family):
    return NAN_CAP if family == "specials_sq" else 0.0


def listed_cases():
    """every (family, (width, height), parameter set, mode) the GPU module runs on generated inputs"""
    return [(f, size, ps, mode) for f in sorted(FAMILIES) for size in SIZES for ps in PARAMETER_SETS for mode in MODES]
