"""The sequences rtgl_temporal_accumulate is run on with generated inputs.  A helper, not a test.  tests/test_temporal_mirror.py pins the
restatement on them, checks the NaN cap and proves that every plausible defect shows on one of them; tests/test_gpu_temporal.py puts the
same arrays in front of the kernel.

A sequence is a list of (image, normal, position, camera): float32 arrays (rows, width, 4) and a camera dict with the camera fields of
rtgl_frame_params.  Except where a family says otherwise the planes are those of a small analytic scene seen through the camera exactly as
the contract's pinhole model sees it (pixel px looks along forward + right wd x + up ht y), so that the reprojection finds what it looks
for; the radiance is a texture fixed to the world plus per-frame noise."""
import math

import numpy as np

f32 = np.float32
FOV = float(f32(math.radians(33.0)))
# (width, height): the smallest sizes, the kernel's block tile of 64 columns x 4 rows from either side, two tile rows and columns, and
# sizes that are no multiple of anything
SIZES = [(1, 1), (2, 2), (7, 5), (63, 3), (64, 4), (65, 5), (70, 53), (129, 9), (200, 131), (127, 7), (128, 8)]
PARAMETER_SETS = [dict(), dict(sigma_normal=0.0), dict(sigma_position=0.0), dict(sigma_normal=0.0, sigma_position=-1.0),
                  dict(max_history=1.0), dict(max_history=2.5), dict(max_history=1e6)]
NAN_CAP = 0.02                  # share of the mirror's components that may be NaN: the project's condition (the comparison cannot see into one)


def cam(position=(0.0, 0.0, -35.0), yaw=0.0, pitch=0.0, fov=FOV, scale=(1.0, 1.0, 1.0), skew=0.0):
    """forward, up, right of a camera turned by yaw about y and pitch about its right axis; scale: lengths of (forward, up, right); skew:
    right += skew forward (a basis that is not quite orthogonal)"""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    right = np.array([-cy, 0.0, sy])
    fwd = np.array([sy * cp, sp, cy * cp])
    up = np.array([-sy * sp, cp, -cy * sp])
    fwd, up, right = fwd * scale[0], up * scale[1], right * scale[2] + skew * fwd * scale[0]
    r = lambda v: tuple(float(f32(x)) for x in v)
    return dict(camera_position=r(position), camera_forward=r(fwd), camera_up=r(up), camera_right=r(right), camera_fov=float(f32(fov)))


def rays(camera, W, H):
    """origin and unit directions (H, W, 3), float64, of the contract's pinhole model"""
    hw = float(f32(math.tan(camera["camera_fov"] * 0.5)))
    wd, ht = 2.0 * hw, 2.0 * hw * (H / W)
    x = (np.arange(W) / W * 2.0 - 1.0)[None, :, None]
    y = (np.arange(H) / H * 2.0 - 1.0)[:, None, None]
    d = np.array(camera["camera_forward"]) + np.array(camera["camera_right"]) * wd * x + np.array(camera["camera_up"]) * ht * y
    return np.array(camera["camera_position"]), d / np.linalg.norm(d, axis=-1, keepdims=True)


# a surface: (z of a plane facing the camera side, x range it covers, |y| it reaches, the normal it reports)
STEP = [(-10.0, (-1e9, 0.5), 1e9, (0.0, 0.0, -1.0)), (0.0, (-1e9, 1e9), 5.0, (0.6, 0.0, -0.8))]            # a near half plane in front of a band of wall
WALL = [(0.0, (-1e9, 1e9), 6.0, (0.0, 0.0, -1.0))]                                                          # a band: misses above and below
ROOM = [(0.0, (-1e9, 1e9), 1e9, (0.0, 0.0, -1.0)), (-70.0, (-1e9, 1e9), 1e9, (0.0, 0.0, 1.0))]              # a wall in front and one behind


def texture(q):
    """radiance fixed to world points or directions q (..., 3): positive, smooth, different per channel"""
    return np.stack([0.6 + 0.4 * np.sin(1.3 * q[..., 0] + 0.5 * c) * np.cos(0.7 * q[..., 1] - 0.3 * c) + 0.1 * np.sin(0.2 * q[..., 2]) for c in range(3)], -1)


def view(camera, W, H, surfaces, rng, noise=0.2):
    """(image, normal, position) of the scene through the camera; alpha of the image is 1 like a rendered frame's"""
    o, d = rays(camera, W, H)
    t = np.full((H, W), np.inf)
    nrm = np.zeros((H, W, 3))
    with np.errstate(all="ignore"):
        for z, (x0, x1), ymax, n in surfaces:
            tz = (z - o[2]) / d[..., 2]
            q = o + d * tz[..., None]
            ok = (tz > 1e-3) & (tz < t) & (q[..., 0] >= x0) & (q[..., 0] < x1) & (np.abs(q[..., 1]) < ymax)
            t = np.where(ok, tz, t)
            nrm = np.where(ok[..., None], np.array(n), nrm)
    hit = np.isfinite(t)
    ts = np.where(hit, t, 0.0)
    point = np.where(hit[..., None], o + d * ts[..., None], 0.0)
    rad = np.where(hit[..., None], texture(point), texture(3.0 * d)) + noise * (rng.random((H, W, 3)) - 0.5)
    image = np.concatenate([rad, np.ones((H, W, 1))], -1).astype(f32)
    normal = np.concatenate([nrm, np.zeros((H, W, 1))], -1).astype(f32)
    position = np.concatenate([point, ts[..., None]], -1).astype(f32)
    return image, normal, position


def _views(cameras, W, H, surfaces, seed):
    rng = np.random.default_rng(seed)
    return [view(c, W, H, surfaces, rng) + (c,) for c in cameras]


def rest(H, W, seed=0):
    return _views([cam()] * 4, W, H, STEP, seed)


def translate(H, W, seed=0):
    return _views([cam((0.37 * k, 0.11 * k, -35.0)) for k in range(4)], W, H, STEP, seed)


def rotate(H, W, seed=0):
    return _views([cam(yaw=y, pitch=p) for y, p in ((0.0, 0.0), (0.04, 0.0), (0.09, 0.03), (0.09, 0.03))], W, H, WALL, seed)


def dolly(H, W, seed=0):
    """towards the edge of the near half plane: the wall behind it comes into view beside it (disocclusion)"""
    return _views([cam((1.5, 0.0, z)) for z in (-35.0, -30.0, -24.0, -19.0, -19.0)], W, H, STEP, seed)


def all_miss(H, W, seed=0):
    return _views([cam(yaw=y, pitch=p) for y, p in ((0.0, 0.0), (0.05, 0.0), (0.05, -0.04), (0.05, -0.04))], W, H, [], seed)


def behind(H, W, seed=0):
    """the camera turns round (every hit of the new view is behind the previous camera), turns half back, and then looks at points strewn
    about it that no ray cast produced, half of them behind"""
    seq = _views([cam(yaw=y) for y in (0.0, math.pi, math.pi / 2)], W, H, ROOM, seed)
    rng = np.random.default_rng(seed + 1)
    for k in range(2):
        c = cam(yaw=math.pi / 2 + 0.3 * k)
        image, normal, position = view(c, W, H, ROOM, rng)
        pts = np.array(c["camera_position"]) + rng.uniform(-30.0, 30.0, (H, W, 3))
        position = np.concatenate([pts, np.linalg.norm(pts - np.array(c["camera_position"]), axis=-1, keepdims=True)], -1).astype(f32)
        seq.append((image, normal, position, c))
    return seq


def skewed(H, W, seed=0):
    """axes of lengths 2, 1.5 and 0.5, the right axis leaning 0.02 into the forward one"""
    return _views([cam((0.3 * k, 0.0, -35.0 + k), yaw=0.02 * k, scale=(2.0, 1.5, 0.5), skew=0.02) for k in range(4)], W, H, STEP, seed)


COLD = [0.0, -0.0, 1e-40, -1e-42, 1e-30, 3e38, -2.5]                      # values that make no NaN by themselves
HOT = [float("nan"), float("inf"), -float("inf")]
T_VALUES = [1e-25, 1e25, 1e-40, -0.0, -3.0, 1e-19, 3e19]                     # (sigma_position t)^2 underflows, overflows; t <= 0 reads as a miss


def specials(H, W, seed=0):
    """the translating sequence with special values strewn in: zeros of both signs, subnormals, huge and negative radiance, hit distances
    whose squared tolerance under- or overflows or that are not positive in about one pixel of twelve; NaN and infinities in image,
    normal and position in one pixel of 3000 per call (a NaN stays in the history and spreads over the four taps of every later
    reprojection: this is what keeps the mirror's NaN share under NAN_CAP), none at all in an image of fewer than 3000 pixels"""
    seq = _views([cam((0.0, 0.0, -35.0)), cam((0.0, 0.0, -35.0)), cam((0.37, 0.11, -35.0)), cam((0.74, 0.22, -35.0)), cam((0.74, 0.22, -35.0))], W, H, STEP, seed)
    rng = np.random.default_rng(seed + 7)
    out = []
    for image, normal, position, c in seq:
        image, normal, position = image.copy(), normal.copy(), position.copy()
        n = H * W
        for arr, comps, values in ((image, 3, COLD), (normal, 3, COLD), (position, 3, COLD), (position, None, T_VALUES)):
            idx = rng.choice(n, size=(n + 11) // 12, replace=False)
            flat = arr.reshape(n, 4)
            for k, p in enumerate(idx):
                flat[p, 3 if comps is None else int(rng.integers(comps))] = f32(values[k % len(values)])
        for arr in (image, normal, position):
            flat = arr.reshape(n, 4)
            for k, p in enumerate(rng.choice(n, size=n // 3000, replace=False)):
                flat[p, int(rng.integers(4 if arr is position else 3))] = f32(HOT[k % len(HOT)])
        out.append((image, normal, position, c))
    return out


FAMILIES = dict(rest=rest, translate=translate, rotate=rotate, dolly=dolly, all_miss=all_miss, behind=behind, skewed=skewed, specials=specials)


def make(family, H, W, seed=0):
    return FAMILIES[family](H, W, seed)


def nan_budget(family):
    return NAN_CAP if family == "specials" else 0.0


def listed_cases():
    """every (family, (width, height), parameter set) the GPU module runs on generated inputs"""
    return [(f, size, ps) for f in sorted(FAMILIES) for size in SIZES for ps in PARAMETER_SETS]
