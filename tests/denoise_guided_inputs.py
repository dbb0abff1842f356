"""The cases rtgl_denoise_guided is run on with generated inputs: the families of tests/denoise_inputs.py (imported, not changed) with
parameter sets of the guided call.  A helper, not a test.  tests/test_denoise_guided_mirror.py pins the restatement on them and checks the
NaN cap; tests/test_gpu_denoise_guided.py puts the same arrays in front of the kernels."""
import denoise_inputs as di

# (width, height) everywhere below, as in denoise_inputs

# values: every family member that holds what no renderer produces.  The luminance term cannot be switched off, so specials always
# comes with its non-finite colours.
VALUE_SIZES = di.VALUE_SIZES
VALUE_PASSES = di.VALUE_PASSES
SPECIALS_PARAMS = [dict(),                                                              # defaults
                   dict(sigma_lum=0.5, sigma_normal=0.1, sigma_position=0.01),          # every term on, small sigmas
                   dict(sigma_normal=0.0, sigma_position=0.0),                          # the luminance term alone
                   dict(sigma_position=0.0),                                            # each geometric term off in turn
                   dict(sigma_normal=0.0),
                   dict(demodulate=False),
                   dict(firefly_ratio=0.0),                                             # clamp off
                   dict(firefly_ratio=2.5, sigma_lum=8.0, demodulate=False)]
# subnormal_weights (denoise_inputs): the geometric factors make the tap weights subnormal; sigma_lum = 1e19 keeps the luminance factor
# near 1 and (sigma_lum sigma_lum) at 1e38.  The clamp is off in one set: it would scale the hot pixels (1e19 against 1e-19) down to nothing.
SW_PARAMS = [dict(sigma_lum=1e19, sigma_normal=0.5, sigma_position=1.0, demodulate=False, firefly_ratio=0.0),
             dict(sigma_lum=1e19, sigma_normal=0.5, sigma_position=1.0, demodulate=True)]
VALUE_PARAMS = {"specials": SPECIALS_PARAMS, "subnormal_weights": SW_PARAMS}

# sizes: denoise_inputs' list (widths around the multiples of 64, heights around 4 step for every step: a pass block takes 64 columns and
# four rows `step` apart) plus the edges of the prepare kernel's tile of 64 x 4 with its halo of 4: heights 4 k - 1, 4 k, 4 k + 1 and
# widths 64 k - 1, 64 k, 64 k + 1 are in the list already; the sizes below add images smaller than the halo and a second tile row and column.
SIZE_CASES = di.SIZE_CASES + [(4, 4), (5, 8), (7, 7), (66, 6), (68, 11), (71, 12), (128, 8), (130, 13), (193, 7)]
NARROW_HEIGHTS = di.NARROW_HEIGHTS
SIZE_PASSES = di.SIZE_PASSES
RAMPS_OFF = dict(sigma_lum=1e6, sigma_normal=0.0, sigma_position=0.0, demodulate=False, firefly_ratio=0.0)
RAMPS_OPEN = dict(sigma_lum=1e6, sigma_normal=100.0, sigma_position=100.0, demodulate=True)
BENIGN_OPEN = dict(sigma_lum=8.0, sigma_position=1.0)
SIZE_RUNS = [("ramps", RAMPS_OFF), ("ramps", RAMPS_OPEN), ("benign", BENIGN_OPEN)]

WIDE_SIZE = di.WIDE_SIZE
WIDE_PASSES = di.WIDE_PASSES
WIDE_RUNS = [("ramps", RAMPS_OFF), ("ramps", RAMPS_OPEN), ("specials", dict())]

# The share of the mirror's components (denoised image and variance buffer together) that may be NaN: the comparison cannot see into a
# NaN.  The luminance term gives a NaN or infinite colour weight 0 for every other pixel and the moments skip it, so the NaN outputs are
# about the NaN inputs.
NAN_CAP = 0.02


def nan_budget(family):
    return NAN_CAP if family == "specials" else 0.0


def make(family, H, W, seed=0):
    return di.make(family, H, W, {}, seed)


def value_cases():
    """(family, (width, height), parameter set) of the value cases; each runs VALUE_PASSES"""
    return [(family, size, ps) for size in VALUE_SIZES for family, sets in VALUE_PARAMS.items() for ps in sets]


def listed_cases():
    """every (family, (width, height), parameter set, pass counts) the GPU module runs on generated inputs"""
    out = [(f, size, ps, VALUE_PASSES) for f, size, ps in value_cases()]
    out += [(f, size, ps, SIZE_PASSES) for size in SIZE_CASES for f, ps in SIZE_RUNS]
    out += [("ramps", size, RAMPS_OFF, SIZE_PASSES) for size in NARROW_HEIGHTS]
    out += [(f, WIDE_SIZE, ps, WIDE_PASSES) for f, ps in WIDE_RUNS]
    return out
