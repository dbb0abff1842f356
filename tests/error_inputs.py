"""Input families for rtgl_error_estimate (seeded, no GPU): sequences of calls.  A family is a function (h, w) -> list of steps; a step is
dict(image=(h, w, 4) float32, frames=F, params=dict(...)): the accumulation image as it stands after the frame rendered with
u_frames = F, and the parameters of the rtgl_error_estimate call made then.  The first step of every family takes the snapshot.  The CPU
tests hand the steps to the mirror's Estimator; the GPU tests render a trivial frame with that F, copy the image in front of the kernel
and make the call.  SIZES are (rows, columns); FULL is the one size with thousands of tiles."""
import numpy as np

import error_mirror as em

SIZES = [(1, 1), (5, 7), (8, 8), (16, 16), (17, 17), (24, 24), (53, 70), (272, 272), (131, 200)]
FULL = (1080, 1920)
f32 = np.float32


def _bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def _grey(L):
    """(h, w) luminances -> (h, w, 4) pixels (v, v, v, 1): lum(v, v, v) is v up to the rounding of 0.75 v"""
    out = np.ones(L.shape + (4,), np.float32)
    out[..., :3] = np.asarray(L, np.float32)[..., None]
    return out


def _fill(pixels, h, w, shift=0):
    pixels = np.asarray(pixels, np.float32).reshape(-1, 4)
    idx = (np.arange(h * w) + shift) % len(pixels)
    return np.ascontiguousarray(pixels[idx].reshape(h, w, 4))


def nested_means(h, w, moments, mu=1.0, sigma=0.3, seed=0):
    """The unbiased means of the first n frames, n in `moments` (ascending), of per-pixel Gaussian frames N(mu, sigma^2): built from the
    increments, mean_n = (m mean_m + (n - m) J) / n with J ~ N(mu, sigma^2 / (n - m)) independent of mean_m, in float64."""
    g = np.random.default_rng(seed)
    out, mean, m = [], np.zeros((h, w)), 0
    for n in moments:
        J = mu + sigma / np.sqrt(n - m) * g.standard_normal((h, w))
        mean = (m * mean + (n - m) * J) / n
        m = n
        out.append(mean.copy())
    return out


def gaussian_steps(h, w, moments, first_frames, mu=1.0, sigma=0.3, seed=0, **params):
    """The image after n real frames counted from first_frames: frames = n - 1 + first_frames, image = mean_n n / (frames + 1)."""
    steps = []
    for n, mean in zip(moments, nested_means(h, w, moments, mu, sigma, seed)):
        F = n - 1 + first_frames
        steps.append(dict(image=_grey((mean * (n / (F + 1.0))).astype(np.float32)), frames=F, params=dict(first_frames=first_frames, **params)))
    return steps


def gauss0(h, w):
    return gaussian_steps(h, w, (16, 32, 48), 0, seed=1)


def gauss1(h, w):
    return gaussian_steps(h, w, (16, 32, 48), 1, seed=2)


def constant(h, w):
    """The same picture at both moments, counted from 0 (g = 1 exactly): every difference is 0, mse 0, converged."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.ones((h, w, 4), np.float32)
    img[..., 0], img[..., 1], img[..., 2] = (xx % 7) / f32(4.0), (yy % 5) / f32(8.0), ((xx + yy) % 3) * f32(1.5)
    return [dict(image=img, frames=F, params=dict(first_frames=0)) for F in (7, 15, 100)]


def black(h, w):
    return [dict(image=np.zeros((h, w, 4), np.float32), frames=F, params=dict()) for F in (8, 16)]


def one_noisy_tile(h, w):
    """Clean everywhere but in the last tile of the footprint: with T valid tiles the picture is converged at quantile_permille = floor(1000 (T - 1) / T)
    and not at one more.  The second and third call keep the snapshot and differ in nothing but the permille."""
    fh, fw = h // 8 * 8, w // 8 * 8
    base = f32(0.5) + (np.arange(h * w, dtype=np.float32).reshape(h, w) % f32(13.0)) / f32(16.0)
    later = base.copy()
    if fh and fw:                                                   # (the last tile that holds footprint pixels)
        later[(fh - 1) // 16 * 16:, (fw - 1) // 16 * 16:] *= f32(1.5)
    T = (-(-fh // 16)) * (-(-fw // 16))                             # (tiles that hold a footprint pixel)
    q = max(1000 * (T - 1) // T, 1) if T else 500
    p = dict(first_frames=0, threshold=0.05)
    return [dict(image=_grey(base), frames=15, params=dict(p)),
            dict(image=_grey(later), frames=31, params=dict(p, quantile_permille=q, keep_snapshot=True)),
            dict(image=_grey(later), frames=31, params=dict(p, quantile_permille=min(q + 1, 1000), keep_snapshot=True)),
            dict(image=_grey(later), frames=31, params=dict(p, quantile_permille=1000))]


def threshold_edge(h, w):
    """Snapshot 0, counted from 0, m = n - m (c = 1), floor 1 and NEGATIVE luminances (den = floor exactly): q = lum.  Tile (0, 0): every
    pixel -0.5, e = 0.25, mse = 0.25 = threshold^2 exactly: converged.  Tile (0, 1): one pixel -(0.5 + 2^-17), whose e = 0.25 + 2^-17 moves
    a full tile's sum from 64 to 64 + 2^-17 and its mse one ulp above 0.25: not converged.  The rest is black."""
    L = np.zeros((h, w), np.float32)
    L[:16, :32] = f32(-0.5)
    if w > 21 and h > 3:
        L[3, 21] = -(f32(0.5) + f32(2.0 ** -17))
    p = dict(first_frames=0, threshold=0.5, floor=1.0, quantile_permille=1000)
    return [dict(image=_grey(np.zeros((h, w), np.float32)), frames=15, params=dict(p)), dict(image=_grey(L), frames=31, params=dict(p))]


def special_pixels():
    nan, inf = f32(np.nan), f32(np.inf)
    den, big = _bits(np.uint32(1)), f32(3e38)
    return [(0.5, 0.25, 0.125, 1), (nan, 0.5, 0.5, 1), (0.5, nan, 0.5, 1), (0.5, 0.5, nan, 1), (nan, nan, nan, nan),
            (inf, 0.5, 0.5, 1), (0.5, -inf, 0.5, 1), (inf, -inf, 0, 1), (inf, inf, inf, 1), (-inf, -inf, -inf, 1),
            (0.0, 0.0, 0.0, 0), (-0.0, -0.0, -0.0, 0), (0.0, -0.0, 0.0, 1), (-1, -1, -1, 1), (-0.5, 2.0, -0.5, 1), (-3, 0.5, 1, 1),
            (den, den, den, 1), (den, 0, 0, 1), (-den, den, 0, 1), (_bits(np.uint32(0x007fffff)), 0, 0, 1), (1e-30, 1e-30, 1e-30, 1),
            (big, big, big, 1), (big, 0, 0, 1), (0, big, big, 1), (-big, big, 0, 1), (1.0, 1.0, 1.0, 1), (2.0, 0.01, 30.0, 1),
            (1e-38, 2e-38, 1e-38, 1), (-1e-39, -1e-39, -1e-39, 1), (1e19, 1e19, 1e19, 1), (-1e19, -1e19, -1e19, 1)]


def specials(h, w):
    """NaN, +-inf, +-0, negatives, denormals and 3e38 at both moments, every one meeting every other (the two images are the same list
    shifted against each other by a step that is coprime to its length); the last call with a denormal floor."""
    px = special_pixels()
    return [dict(image=_fill(px, h, w, 0), frames=4, params=dict()),
            dict(image=_fill(px, h, w, 7), frames=9, params=dict()),
            dict(image=_fill(px, h, w, 12), frames=31, params=dict(threshold=10.0)),
            dict(image=_fill(px, h, w, 13), frames=63, params=dict(floor=1e-40))]


def overflow(h, w):
    """Finite e of 2.9e38 (lum -1.7e17 over the floor 0.01) in every second pixel: each counts, a tile's sum reaches +inf, and so do its
    mse, the picture's and max_tile_mse; defined, and not converged.  The lower half of the rows stays finite."""
    L = np.zeros((h, w), np.float32)
    L[:, 0::2] = f32(-1.7e17)
    L[h // 2:, :] *= f32(1e-10)
    p = dict(first_frames=0)                                        # (g = 1: the luminance reaches the division as it stands)
    return [dict(image=_grey(np.zeros((h, w), np.float32)), frames=1, params=dict(p)), dict(image=_grey(L), frames=3, params=dict(p))]


def nan_tile(h, w):
    """Tile (0, 0) all NaN (count 0: the record {0, 0, 0, 0}, not valid), ordinary noise elsewhere."""
    steps = gaussian_steps(h, w, (8, 24), 1, seed=3)
    steps[1]["image"][:16, :16, :3] = np.nan
    return steps


FAMILIES = dict(gauss0=gauss0, gauss1=gauss1, constant=constant, black=black, one_noisy_tile=one_noisy_tile, threshold_edge=threshold_edge,
                specials=specials, overflow=overflow, nan_tile=nan_tile)


def family(name, h, w):
    return FAMILIES[name](h, w)


def run(steps, estimator=None):
    """the mirror's results of a family's steps, in order"""
    est = estimator or em.Estimator()
    out = []
    for s in steps:
        est.frame(s["frames"])
        out.append(est(s["image"], **s["params"]))
    return out
