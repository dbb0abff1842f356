"""The sequences rtgl_temporal_clip is run on with generated inputs.  A helper, not a test.  tests/test_temporal_clip_mirror.py pins the
restatement on them, checks the NaN cap and proves that every plausible defect shows on one of them; tests/test_gpu_temporal_clip.py puts
the same arrays in front of the kernel.

The sequences, sizes and geometry are those of tests/temporal_inputs.py (every family there is run here too, `specials` included), each
item with the albedo plane of tests/temporal_moments_inputs.py behind it so that option "temporal_moments" = 2 can be run: an item is
(image, normal, position, camera, albedo).  Five families are added for what the clip is about: radiance that changes while the geometry
does not, radiance without noise, windows that straddle an edge of the guides, and neighbours close enough to count at the smallest sizes."""
import numpy as np

import temporal_inputs as ti
from temporal_moments_inputs import albedo_plane

f32 = np.float32
# (width, height): a 7 x 7 window on a 64 x 4 tile: a window larger than the image, and a tile edge from either side
SIZES = [(1, 1), (2, 2), (7, 5), (63, 3), (64, 4), (65, 5), (127, 7), (128, 8), (129, 9), (70, 53), (200, 131)]
assert sorted(SIZES) == sorted(ti.SIZES)
# parameters of rtgl_temporal_clip (rtgl_temporal_accumulate keeps its defaults): the defaults, each sigma off, both off, a box so narrow
# that most pixels clip and one so wide that none does, the history cut to a single frame and not at all
PARAMETER_SETS = [dict(), dict(sigma_normal=0.0), dict(sigma_position=0.0), dict(sigma_normal=0.0, sigma_position=-1.0),
                  dict(sigma_scale=0.5), dict(sigma_scale=1e6), dict(clip_history=1.0), dict(clip_history=1e6)]
MODES = (0, 1, 2)               # option "temporal_moments"
NAN_CAP = ti.NAN_CAP
RELIT_AFTER = 8                 # `relight`: frames at rest before the radiance changes


def relit(image):
    """radiance x -> 2 x + 0.5 (alpha kept): what a change of lighting does to a frame whose first hits stay where they are"""
    out = image.copy()
    out[..., :3] = f32(2) * image[..., :3] + f32(0.5)
    return out


def _relit_from(seq, k0):
    return [(relit(im) if k >= k0 else im, n, p, c) for k, (im, n, p, c) in enumerate(seq)]


def relight(H, W, seed=0):
    """the camera at rest over ROOM: 8 frames, then 4 with the radiance relit"""
    return _relit_from(ti._views([ti.cam()] * (RELIT_AFTER + 4), W, H, ti.ROOM, seed), RELIT_AFTER)


def relight_truth(H, W):
    """the noise-free radiance of `relight` before and after the change, float64 (H, W, 3)"""
    x = ti.view(ti.cam(), W, H, ti.ROOM, np.random.default_rng(0), noise=0.0)[0][..., :3].astype(np.float64)
    return x, 2.0 * x + 0.5


def relight_moving(H, W, seed=0):
    """the same change in the middle of `translate`"""
    return _relit_from(ti.translate(H, W, seed), 2)


def flat(H, W, seed=0):
    """constant noise-free radiance over STEP, the camera at rest: nothing may change, not by a rounding of the neighbourhood mean"""
    seq = ti.rest(H, W, seed)
    image = np.broadcast_to(np.array([0.3, 0.7, 0.55, 1.0], f32), (H, W, 4)).copy()
    return [(image.copy(), n, p, c) for _, n, p, c in seq]


def edge(H, W, seed=0):
    """STEP at rest, two frames and two relit ones: the windows along the depth step and along the border between hit and miss take their
    box from their own side only, and the clamp acts right up to the edge"""
    return _relit_from(ti.rest(H, W, seed + 3), 2)


NARROW_FOV = 0.04               # radians: tan(fov / 2) = 0.02


def narrow(H, W, seed=0):
    """ROOM at rest through a lens of 2.3 degrees, three frames and two relit ones.  The other families' hits are 4 tan(fov / 2) t / W
    apart against a position tolerance of 0.05 t, which is 23.7 / W tolerances: below 63 columns every hit is alone in its window and has
    the box [I, I].  Here neighbours are 1.6 / W tolerances apart, so that from 2 x 2 on every window holds several taps that count and
    the small sizes test the box and not only the pixel's own sample."""
    return _relit_from(ti._views([ti.cam(fov=NARROW_FOV)] * 5, W, H, ti.ROOM, seed + 5), 3)


FAMILIES = dict(ti.FAMILIES, relight=relight, relight_moving=relight_moving, flat=flat, edge=edge, narrow=narrow)


def make(family, H, W, seed=0):
    """the family's sequence, every item with an albedo plane behind it"""
    return [item + (albedo_plane(H, W, seed + k),) for k, item in enumerate(FAMILIES[family](H, W, seed))]


def nan_budget(family):
    return NAN_CAP if family == "specials" else 0.0


def listed_cases():
    """every (family, (width, height), parameter set, mode) the GPU module runs on generated inputs"""
    return [(f, size, ps, mode) for f in sorted(FAMILIES) for size in SIZES for ps in PARAMETER_SETS for mode in MODES]
