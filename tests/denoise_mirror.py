"""numpy float32 restatement of rtgl_denoise (the contract is in include/rtgl_amd.h, "denoiser").  A helper, not a test.

Vectorised over pixels, loops over the passes and the 25 taps, and does exactly the operations the contract lists, in their order.  numpy's
float32 array operations round once per operation and never fuse, which is what the contract asks for; the selects are np.where so that a
NaN behaves as defined (a NaN compares false).  Every array is float32, shaped (rows, width, 4), rows bottom-up like the image."""
import math

import numpy as np

f32 = np.float32
H5 = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
ALBEDO_FLOOR = f32(2.0 ** -10)
DEFAULTS = dict(passes=5, sigma_color=16.0, sigma_normal=0.3, sigma_position=0.05, demodulate=True)


def ew(x):
    """(1 - x/4)^4 for x < 4, else 0; a NaN gives 0"""
    q = np.where(x < f32(4), f32(1) - f32(0.25) * x, f32(0)).astype(f32)
    q = q * q
    return q * q


def dot3(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def divisor(albedo):
    a = albedo[..., :3]
    return np.where(a > ALBEDO_FLOOR, a, ALBEDO_FLOOR).astype(f32)


def denoise(image, albedo=None, normal=None, position=None, passes=5, sigma_color=16.0, sigma_normal=0.3, sigma_position=0.05, demodulate=True):
    """The denoised RGBA image.  A plane the parameters do not need may be None (albedo iff demodulating, normal iff sigma_normal > 0,
    position iff sigma_position > 0); bad parameters raise ValueError as the library returns RTGL_ERR_INVALID."""
    if not (isinstance(passes, (int, np.integer)) and 0 <= passes <= 8):
        raise ValueError("passes must be 0..8")
    if not all(math.isfinite(s) for s in (sigma_color, sigma_normal, sigma_position)):
        raise ValueError("the sigmas must be finite")
    sc, sn, sp = f32(sigma_color), f32(sigma_normal), f32(sigma_position)
    use_c, use_n, use_p = bool(sc > 0), bool(sn > 0), bool(sp > 0)
    image = np.ascontiguousarray(image, f32)
    H, W = image.shape[:2]
    for need, plane, what in ((demodulate, albedo, "albedo"), (use_n, normal, "normal"), (use_p, position, "position")):
        if need and (plane is None or plane.shape != image.shape or plane.dtype != f32):
            raise ValueError(f"the {what} plane is needed as float32 of the image's shape")
    with np.errstate(all="ignore"):
        d = divisor(albedo) if demodulate else None
        c = (image[..., :3] / d) if demodulate else image[..., :3].copy()
        for L in range(passes):
            s = 1 << L
            sig = sc * f32(2.0 ** -L)
            ic = f32(1) / (sig * sig)
            inn = f32(1) / (sn * sn) if use_n else f32(0)
            if use_p:
                spt = sp * position[..., 3]
                ip = np.where(spt > 0, f32(1) / (spt * spt), f32(0)).astype(f32)
            acc = np.zeros_like(c)
            ws = np.zeros((H, W), f32)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    dy, dx = j * s, i * s
                    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                    if y1 <= y0 or x1 <= x0:
                        continue                                      # every such tap is outside the image
                    P_ = (slice(y0, y1), slice(x0, x1))               # the pixels p whose tap q = p + (dx, dy) is inside
                    Q_ = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                    cq = c[Q_]
                    w = H5[j + 2] * H5[i + 2]
                    if use_c:
                        w = w * ew(dot3(cq - c[P_]) * ic)
                    if use_n:
                        w = w * ew(dot3(normal[Q_][..., :3] - normal[P_][..., :3]) * inn)
                    if use_p:
                        w = w * ew(dot3(position[Q_][..., :3] - position[P_][..., :3]) * ip[P_])
                    w = np.broadcast_to(np.asarray(w, f32), cq.shape[:2])
                    use = w > 0
                    acc[P_] = np.where(use[..., None], acc[P_] + w[..., None] * cq, acc[P_])
                    ws[P_] = np.where(use, ws[P_] + w, ws[P_])
            ok = ws > 0
            c = np.where(ok[..., None], acc / np.where(ok, ws, f32(1))[..., None], c).astype(f32)
        out = (c * d) if demodulate else c
    return np.concatenate([out.astype(f32), image[..., 3:4]], axis=-1)
