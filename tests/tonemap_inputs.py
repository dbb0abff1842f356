"""Input families for rtgl_tonemap (seeded, no GPU): (h, w, 4) float32 images that the CPU tests hand to the mirror and the GPU tests write
into a context's image.  A family lists its probe pixels first and repeats them cyclically, so a size that is too small for all of them
still begins with the first ones; the sizes the tests use are listed in SIZES, FULL is the one size with many blocks per bin."""
import numpy as np

import tonemap_mirror as tm

FAMILIES = ["bin_edges", "thresholds", "specials", "hdr", "black"]
SIZES = [(1, 1), (5, 7), (4, 64), (3, 257), (131, 200)]            # (rows, columns)
FULL = (1080, 1920)


def _bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def _fill(pixels, h, w, shift=0):
    pixels = np.asarray(pixels, np.float32).reshape(-1, 4)
    idx = (np.arange(h * w) + shift) % len(pixels)
    return np.ascontiguousarray(pixels[idx].reshape(h, w, 4))


def bin_edge_luminances():
    """The lower edge of every bin and the float one ulp below it (bin 0: the edge 2^-16 and the value below, which bin 0 also holds)."""
    edges = (np.arange(256, dtype=np.uint32) + np.uint32(tm.BIN_BIAS)) << np.uint32(20)
    return _bits(np.stack([edges, edges - np.uint32(1)], 1).ravel())


def bin_edges(h, w):
    """A luminance on every bin's lower edge and one ulp below it: (0, 2 L, 0) has the luminance L exactly."""
    L = bin_edge_luminances()
    px = np.zeros((len(L), 4), np.float32)
    px[:, 1] = L * np.float32(2.0)
    px[:, 3] = 1.0
    return _fill(px, h, w)


def threshold_values():
    """Every T[k], k = 1..255, with the float below and the float above."""
    t = tm.T_TABLE[1:].view(np.uint32)
    return _bits(np.stack([t - np.uint32(1), t, t + np.uint32(1)], 1).ravel())


def thresholds(h, w):
    """Every T[k] with its two float neighbours in each channel in turn (the other two channels 0.5): under op 0 at exposure 1 the value
    reaches the encoder as it stands."""
    v = threshold_values()
    px = np.full((3, len(v), 4), 0.5, np.float32)
    for ch in range(3):
        px[ch, :, ch] = v
    px[..., 3] = 1.0
    return _fill(px, h, w)


def specials(h, w):
    """NaN, +-inf, +-0, negatives, denormals, 3e38 and a pixel of luminance -1 (op 1 divides by 1 + L) next to ordinary pixels."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    den, big = _bits(np.uint32(1)), np.float32(3e38)
    px = [(0.5, 0.25, 0.125, 1), (nan, 0.5, 0.5, 1), (0.5, nan, 0.5, 1), (0.5, 0.5, nan, 1), (nan, nan, nan, nan),
          (inf, 0.5, 0.5, 1), (0.5, -inf, 0.5, 1), (inf, -inf, 0, 1), (inf, inf, inf, 1), (-inf, -inf, -inf, 1),
          (0.0, 0.0, 0.0, 0), (-0.0, -0.0, -0.0, 0), (0.0, -0.0, 0.0, 1), (-1, -1, -1, 1), (-0.5, 2.0, -0.5, 1), (-3, 0.5, 1, 1),
          (den, den, den, 1), (den, 0, 0, 1), (-den, den, 0, 1), (_bits(np.uint32(0x007fffff)), 0, 0, 1), (1e-30, 1e-30, 1e-30, 1),
          (big, big, big, 1), (big, 0, 0, 1), (0, big, big, 1), (-big, big, 0, 1), (1.0, 1.0, 1.0, 1), (2.0, 0.01, 30.0, 1),
          (65536.0, 65536.0, 65536.0, 1), (131072.0, 0, 0, 1), (2.0 ** -16, 2.0 ** -16, 2.0 ** -16, 1), (2.0 ** -18, 2.0 ** -17, 0, 1)]
    return _fill(np.array(px, np.float32), h, w)


def hdr(h, w, seed=0):
    """A rendered-like HDR field: a smooth gradient over four decades, per-pixel noise, fireflies, a 30 x emissive patch and black pixels."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.exp2(-6.0 + 8.0 * (xx + 1) / (w + 1) + 2.0 * (yy + 1) / (h + 1))
    img = (base[..., None] * g.lognormal(0.0, 0.6, (h, w, 3)) * np.array([1.0, 0.8, 0.6])).astype(np.float32)
    img[g.random((h, w)) < 0.01] *= np.float32(200.0)
    img[g.random((h, w)) < 0.05] = 0.0
    img[h // 3: h // 3 + max(h // 8, 1), w // 2: w // 2 + max(w // 8, 1)] = 30.0
    out = np.ones((h, w, 4), np.float32)
    out[..., :3] = img
    return out


def black(h, w):
    return np.zeros((h, w, 4), np.float32)


def family(name, h, w):
    return {"bin_edges": bin_edges, "thresholds": thresholds, "specials": specials, "hdr": hdr, "black": black}[name](h, w)


# the parameter sets every family meets: operator x auto / manual (manual at exposure 1, so that `thresholds` and `specials` reach the
# curve as they stand), and one auto set away from the defaults
def parameter_sets():
    sets = []
    for op in (0, 1, 2):
        sets.append(dict(op=op, auto=True))
        sets.append(dict(op=op, auto=False, exposure=1.0))
    sets.append(dict(op=1, auto=True, key=0.5, white=2.0, low_permille=0, high_permille=500, exposure_min=0.5, exposure_max=8.0))
    sets.append(dict(op=2, auto=False, exposure=0.37))
    return sets
