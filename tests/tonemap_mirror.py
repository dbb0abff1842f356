"""numpy restatement of rtgl_tonemap (include/rtgl_amd.h, "display transform"; kernels in raytracer.glsl_amd/csrc/rt_tonemap.hpp): the
luminance histogram, the integer solve for the exposure, the tone curve and the sRGB encoding by thresholds.  Every float operation is
binary32 with one rounding, in the order the header writes; every integer step is exact.  The device must give the same bits: display
bytes, bins, `ignored` and the exposure.

The two tables are generated here BY FORMULA; the committed constants of rt_tonemap.hpp are the contract, and tests/test_tonemap_mirror.py
holds that the two agree."""
import numpy as np

F = np.float32

# rtgl_tonemap_defaults (stated four times: header, binding, facade, here)
DEFAULTS = dict(source=0, op=1, auto=True, exposure=1.0, key=0.18, white=4.0, adapt=1.0, exposure_min=2.0 ** -16, exposure_max=2.0 ** 16,
                low_permille=100, high_permille=20)
OP_LINEAR, OP_REINHARD, OP_ACES = 0, 1, 2
BINS = 256
BIN_BIAS = 888            # (127 - 16) * 8: bin 0 begins at 2^-16, eight bins per binade


def exposure_table():
    """P[r] = float32(2^(-r/64)), r = 0..63."""
    return np.array([2.0 ** (-r / 64.0) for r in range(64)], np.float64).astype(np.float32)


def srgb_decode(v):
    """sRGB electro-optical transfer function (IEC 61966-2-1) in float64: encoded value in [0, 1] -> linear."""
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


def threshold_table():
    """T[k] = float32 of the sRGB-decoded (k - 0.5) / 255, k = 1..255; T[0] = 0 is never compared."""
    t = np.zeros(256, np.float32)
    t[1:] = srgb_decode((np.arange(1, 256, dtype=np.float64) - 0.5) / 255.0).astype(np.float32)
    return t


P_TABLE = exposure_table()
T_TABLE = threshold_table()


def lum(r, g, b):
    return (F(0.25) * r + F(0.5) * g) + F(0.25) * b


def histogram(img):
    """(bins uint32[256], ignored) of an (h, w, 4) float32 image."""
    img = np.asarray(img, np.float32)
    with np.errstate(all="ignore"):
        L = lum(img[..., 0], img[..., 1], img[..., 2]).astype(np.float32).ravel()
        counts = L > 0                                                     # NaN, +-0 and negatives do not count
    bits = np.ascontiguousarray(L).view(np.uint32).astype(np.int64) >> 20
    b = np.clip(bits - BIN_BIAS, 0, BINS - 1)
    hist = np.bincount(b[counts], minlength=BINS).astype(np.uint32)
    return hist, int(L.size - int(counts.sum()))


def solve(hist, prev=None, **params):
    """The exposure (float32) from a histogram.  prev: the exposure the previous call stored since the last reset, or None."""
    p = dict(DEFAULTS); p.update(params)
    h = [int(x) for x in hist]
    N = sum(h)
    if N == 0:
        target = F(p["exposure"])
    else:
        lo, hi = N * int(p["low_permille"]) // 1000, N * int(p["high_permille"]) // 1000
        c = K = S = 0
        for b in range(BINS):
            kept = max(0, min(c + h[b], N - hi) - max(c, lo))
            K += kept
            S += kept * (2 * b + 1)
            c += h[b]
        m = 4 * S // K                                                     # K >= 1: low + high < 1000
        q, r = m // 64, m % 64
        with np.errstate(all="ignore"):
            target = np.ldexp(F(F(p["key"]) * P_TABLE[r]), 16 - q).astype(np.float32)
    e = F(target)
    a = F(p["adapt"])
    with np.errstate(all="ignore"):
        if a < F(1.0) and prev is not None:
            e = F(F(prev) + F(F(target - F(prev)) * a))
    emin, emax = F(p["exposure_min"]), F(p["exposure_max"])
    e = emin if e < emin else e
    e = emax if e > emax else e
    return F(e)


def encode(y):
    """sRGB code of linear y: the number of thresholds T[1..255] that are <= y (NaN and negatives 0, +inf 255)."""
    y = np.asarray(y, np.float32)
    code = np.searchsorted(T_TABLE[1:], y, side="right")
    return np.where(np.isnan(y), 0, code).astype(np.uint8)


def tone_curve(img, e, op, white):
    """(h, w, 3) float32: the tone-mapped linear colour of img.rgb at exposure e."""
    img = np.asarray(img, np.float32)
    e = F(e)
    with np.errstate(all="ignore"):
        x = (img[..., :3] * e).astype(np.float32)
        if op == OP_LINEAR:
            return x
        if op == OP_REINHARD:
            w2 = F(white) * F(white)
            Lx = lum(x[..., 0], x[..., 1], x[..., 2])
            s = (F(1.0) + Lx / w2) / (F(1.0) + Lx)
            return (x * s[..., None]).astype(np.float32)
        if op == OP_ACES:
            return ((x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))).astype(np.float32)
    raise ValueError(op)


def map_encode(img, e, op, white):
    """(h, w, 4) uint8 display buffer, rows in the image's order, alpha 255."""
    y = tone_curve(img, e, op, white)
    out = np.empty(y.shape[:2] + (4,), np.uint8)
    out[..., :3] = encode(y)
    out[..., 3] = 255
    return out


def tonemap(img, prev=None, **params):
    """One rtgl_tonemap call over img: dict(display, hist, ignored, exposure).  With auto off hist and ignored are None (the histogram and
    solve launches are skipped) and the exposure is params' own, unclamped; `prev` is then neither read nor replaced."""
    p = dict(DEFAULTS); p.update(params)
    if p["auto"]:
        hist, ignored = histogram(img)
        e = solve(hist, prev, **p)
    else:
        hist, ignored, e = None, None, F(p["exposure"])
    return dict(display=map_encode(img, e, p["op"], p["white"]), hist=hist, ignored=ignored, exposure=e)


class Tonemapper:
    """The state a context keeps between calls: the exposure the latest auto call stored, dropped by reset()."""

    def __init__(self):
        self.prev = None

    def reset(self):
        self.prev = None

    def __call__(self, img, **params):
        out = tonemap(img, self.prev, **params)
        if out["hist"] is not None:
            self.prev = out["exposure"]
        return out
