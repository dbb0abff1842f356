"""numpy float32 restatement of rtgl_denoise_guided (the contract is in include/rtgl_amd.h, "variance-guided denoiser").  A helper, not a test.

Built like tests/denoise_mirror.py, whose ew, dot3, divisor and H5 it uses: vectorised over pixels, loops over passes and taps, exactly the
operations the contract lists, in their order; every select is an np.where so that a NaN behaves as defined.  Arrays are float32,
(rows, width, 4), rows bottom-up like the image.  denoise_guided returns (denoised image, variance buffer {mu, v0, var, s0})."""
import math

import numpy as np

from denoise_mirror import H5, divisor, dot3, ew

f32 = np.float32
B3 = [f32(0.25), f32(0.5), f32(0.25)]
VAR_FLOOR = f32(2.0 ** -20)
DEFAULTS = dict(passes=5, sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05, firefly_ratio=1.0, demodulate=True)


def lum(c):
    return (f32(0.25) * c[..., 0] + f32(0.5) * c[..., 1]) + f32(0.25) * c[..., 2]


def _shifted(H, W, dy, dx):
    """(P, Q): slices of the pixels p whose tap q = p + (dx, dy) is inside the image, and of those taps; None when there is none"""
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y1 <= y0 or x1 <= x0:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def geometric(g, P_, Q_, normal, position, geo):
    """g times the normal and the position factor between the pixels P_ and their taps Q_ (a term whose sigma is <= 0 is skipped)"""
    use_n, use_p, inn, ip = geo
    if use_n:
        g = g * ew(dot3(normal[Q_][..., :3] - normal[P_][..., :3]) * inn)
    if use_p:
        g = g * ew(dot3(position[Q_][..., :3] - position[P_][..., :3]) * ip[P_])
    return g


def firefly_clamp(c0, ratio, normal=None, position=None, geo=(False, False, f32(0), None)):
    """c1: a pixel brighter than ratio x its brightest neighbour is scaled down to that; a neighbour counts if its geometric weight is > 0"""
    H, W = c0.shape[:2]
    l0 = lum(c0)
    m = np.zeros((H, W), f32)
    have = np.zeros((H, W), bool)
    for j in range(-1, 2):
        for i in range(-1, 2):
            sl = _shifted(H, W, j, i)
            if (i == 0 and j == 0) or sl is None:
                continue
            P_, Q_ = sl
            lq = l0[Q_]
            near = geometric(np.ones(lq.shape, f32), P_, Q_, normal, position, geo) > 0
            m[P_] = np.where(near, np.where(have[P_], np.where(lq > m[P_], lq, m[P_]), lq), m[P_])
            have[P_] = have[P_] | near
    k = ratio * m
    hot = have & (l0 > k)
    s = k / np.where(hot, l0, f32(1))
    return np.where(hot[..., None], c0 * s[..., None], c0).astype(f32)


def geometry(normal, position, sn, sp):
    """(use_n, use_p, in, ip per pixel)"""
    use_n, use_p = bool(sn > 0), bool(sp > 0)
    inn = f32(1) / (sn * sn) if use_n else f32(0)
    ip = None
    if use_p:
        spt = sp * position[..., 3]
        ip = np.where(spt > 0, f32(1) / (spt * spt), f32(0)).astype(f32)
    return use_n, use_p, inn, ip


def spatial_variance(c1, normal, position, geo, radius=3):
    """(mu, v0, s0, near): the moments of lum(c1) over the (2 radius + 1)^2 window, weighted by the geometric factors, finite taps only;
    near[j + 1][i + 1]: where the neighbour p + (i, j) is inside the image with a geometric weight > 0 (the pixel itself: everywhere)"""
    H, W = c1.shape[:2]
    l1 = lum(c1)
    near = [[np.zeros((H, W), bool) for _ in range(3)] for _ in range(3)]
    near[1][1][...] = True
    s0, s1, s2 = (np.zeros((H, W), f32) for _ in range(3))
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            sl = _shifted(H, W, j, i)
            if sl is None:
                continue
            P_, Q_ = sl
            lq = l1[Q_]
            g = geometric(np.ones(lq.shape, f32), P_, Q_, normal, position, geo)
            if abs(i) <= 1 and abs(j) <= 1 and (i or j):
                near[j + 1][i + 1][P_] = g > 0
            use = (g > 0) & (lq - lq == 0)
            s0[P_] = np.where(use, s0[P_] + g, s0[P_])
            s1[P_] = np.where(use, s1[P_] + g * lq, s1[P_])
            s2[P_] = np.where(use, s2[P_] + g * (lq * lq), s2[P_])
    ok = s0 > 0
    safe = np.where(ok, s0, f32(1))
    mu = np.where(ok, s1 / safe, f32(0)).astype(f32)
    v = s2 / safe - mu * mu
    v0 = np.where(ok & (v > 0), v, f32(0)).astype(f32)
    return mu, v0, s0, near


def blurred_variance(var, near):
    H, W = var.shape
    vs, vw = np.zeros((H, W), f32), np.zeros((H, W), f32)
    for j in range(-1, 2):
        for i in range(-1, 2):
            sl = _shifted(H, W, j, i)
            if sl is None:
                continue
            P_, Q_ = sl
            w = B3[j + 1] * B3[i + 1]
            use = near[j + 1][i + 1][P_]
            vs[P_] = np.where(use, vs[P_] + w * var[Q_], vs[P_])
            vw[P_] = np.where(use, vw[P_] + w, vw[P_])
    return vs / vw


def guided_pass(c, var, step, sl2, normal, position, geo, near):
    H, W = var.shape
    il = f32(1) / (sl2 * blurred_variance(var, near) + VAR_FLOOR)
    lc = lum(c)
    acc, ws, va = np.zeros_like(c), np.zeros((H, W), f32), np.zeros((H, W), f32)
    for j in range(-2, 3):
        for i in range(-2, 3):
            sl = _shifted(H, W, j * step, i * step)
            if sl is None:
                continue
            P_, Q_ = sl
            cq = c[Q_]
            dl = lc[Q_] - lc[P_]
            w = H5[j + 2] * H5[i + 2]
            w = geometric(w * ew((dl * dl) * il[P_]), P_, Q_, normal, position, geo)
            use = w > 0
            acc[P_] = np.where(use[..., None], acc[P_] + w[..., None] * cq, acc[P_])
            ws[P_] = np.where(use, ws[P_] + w, ws[P_])
            va[P_] = np.where(use, va[P_] + (w * w) * var[Q_], va[P_])
    ok = ws > 0
    safe = np.where(ok, ws, f32(1))
    c = np.where(ok[..., None], acc / safe[..., None], c).astype(f32)
    var = np.where(ok, va / (safe * safe), var).astype(f32)
    return c, var


def denoise_guided_each(image, albedo=None, normal=None, position=None, passes_list=(5,), sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05,
                        firefly_ratio=1.0, demodulate=True):
    """{passes: (denoised RGBA image, variance buffer)} for every pass count of passes_list, sharing the work the counts have in common.
    A plane the parameters do not need may be None; bad parameters raise ValueError as the library returns RTGL_ERR_INVALID."""
    if not all(isinstance(k, (int, np.integer)) and 0 <= k <= 8 for k in passes_list):
        raise ValueError("passes must be 0..8")
    if not all(math.isfinite(s) for s in (sigma_lum, sigma_normal, sigma_position, firefly_ratio)):
        raise ValueError("the sigmas and the ratio must be finite")
    sl, sn, sp, fr = f32(sigma_lum), f32(sigma_normal), f32(sigma_position), f32(firefly_ratio)
    if not sl > 0:
        raise ValueError("sigma_lum must be > 0")
    image = np.ascontiguousarray(image, f32)
    for need, plane, what in ((demodulate, albedo, "albedo"), (sn > 0, normal, "normal"), (sp > 0, position, "position")):
        if need and (plane is None or plane.shape != image.shape or plane.dtype != f32):
            raise ValueError(f"the {what} plane is needed as float32 of the image's shape")
    out = {}
    with np.errstate(all="ignore"):
        d = divisor(albedo) if demodulate else None
        c = (image[..., :3] / d) if demodulate else image[..., :3].copy()
        geo = geometry(normal, position, sn, sp)
        if fr > 0:
            c = firefly_clamp(c, fr, normal, position, geo)
        mu, v0, s0, near = spatial_variance(c, normal, position, geo)
        var = v0
        for L in range(max(passes_list, default=0) + 1):
            if L in passes_list:
                rgb = (c * d) if demodulate else c
                out[L] = (np.concatenate([rgb.astype(f32), image[..., 3:4]], axis=-1), np.stack([mu, v0, var, s0], -1).astype(f32))
            if L < max(passes_list):
                c, var = guided_pass(c, var, 1 << L, sl * sl, normal, position, geo, near)
    return out


def denoise_guided(image, albedo=None, normal=None, position=None, passes=5, **params):
    """(denoised RGBA image, variance buffer {mu, v0, var, s0}) for one pass count"""
    return denoise_guided_each(image, albedo, normal, position, passes_list=(passes,), **params)[passes]
