"""numpy restatement of rtgl_robust_denoise (include/rtgl_amd.h, "robust denoise"), written from the header: keys, ranks, G, t and the
resolve from robust_mirror; the divisor, ew and dot3 from denoise_mirror; the geometric weights, the near neighbours and the passes from
denoise_guided_mirror; what is new here is the per-pixel variance of the winsorized bucket luminances.  Every operation in binary32 in
the order the header writes, every select an np.where so that a NaN behaves as defined.  A helper, not a test; no GPU.
tests/test_robust_denoise_mirror.py pins it, tests/test_gpu_robust_denoise.py compares the device with it bit for bit.

Arrays are float32: planes (K, rows, width, 4), the first-hit planes (rows, width, 4), rows bottom-up like the image."""
import numpy as np

import denoise_guided_mirror as gm
import robust_mirror as rm
from denoise_mirror import divisor

f32 = np.float32
DEFAULTS = dict(passes=5, sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05, gain=1.0, demodulate=True)
DEMODULATE = 1
PLANE_ALBEDO, PLANE_NORMAL, PLANE_POSITION = 1, 2, 4


def valid_params(passes, sigma_lum, sigma_normal, sigma_position, gain, flags=DEMODULATE, reserved=(0, 0)):
    """what the library accepts; everything else is RTGL_ERR_INVALID"""
    with np.errstate(over="ignore"):
        sl, sn, sp, gain = f32(sigma_lum), f32(sigma_normal), f32(sigma_position), f32(gain)      # (the record holds binary32)
    return bool(0 <= passes <= 8 and np.isfinite(sl) and np.isfinite(sn) and np.isfinite(sp) and sl > 0 and np.isfinite(gain) and gain >= 0
                and not flags & ~DEMODULATE and not any(reserved))


def planes_needed(sigma_normal, sigma_position, demodulate):
    return (PLANE_ALBEDO if demodulate else 0) | (PLANE_NORMAL if f32(sigma_normal) > 0 else 0) | (PLANE_POSITION if f32(sigma_position) > 0 else 0)


def refused(session, N, K, tiled=False, needed=0, enabled=0, restarted=False, frames_in_planes=1):
    """RTGL_ERR_STATE: no session, a bucket without a sample, a tiled or multi-device context, a needed plane that is not enabled, or
    needed planes that hold no frame since they restarted"""
    return bool(not session or N < K or tiled or needed & ~enabled or (needed and (restarted or frames_in_planes == 0)))


def bucket_variance(planes, N, gain=1.0, d=None):
    """steps 1-5: (out (..., 4), v, v0, h) for planes (K, ..., 4) after N >= K frames; d: the divisor (..., 3) when demodulating"""
    planes = np.asarray(planes, f32)
    K = planes.shape[0]
    assert K in rm.BUCKETS and N >= K
    out, _, t = rm.resolve(planes, N, gain)
    key, rank, _ = rm.gini(planes)
    with np.errstate(all="ignore"):
        if d is None:
            x = key
        else:
            l = gm.lum(planes[..., :3] / d[None])
            x = np.where(np.isfinite(l), l, rm.INF).astype(f32)
        lo = np.zeros(t.shape, f32)
        hi = np.zeros(t.shape, f32)
        for j in range(K):
            lo = np.where(rank[j] == t, x[j], lo)
            hi = np.where(rank[j] == K - 1 - t, x[j], hi)
        w = [np.where(rank[j] < t, lo, np.where(rank[j] > K - 1 - t, hi, x[j])).astype(f32) for j in range(K)]
        M = np.zeros(t.shape, f32)
        for j in range(K):
            M = M + w[j]
        mw = M / f32(K)
        D = np.zeros(t.shape, f32)
        for j in range(K):
            dd = w[j] - mw
            D = D + dd * dd
        h = (K - 2 * t).astype(np.int32)
        v = (D / (h * (h - 1)).astype(f32)).astype(f32)
        v0 = np.where(v - v == 0, v, f32(0)).astype(f32)
    return out, v, v0, h


def near_mask(normal, position, geo, H, W):
    """step 6: near[j + 1][i + 1], where the neighbour p + (i, j) is inside the image with a geometric weight > 0"""
    near = [[np.zeros((H, W), bool) for _ in range(3)] for _ in range(3)]
    near[1][1][...] = True
    for j in range(-1, 2):
        for i in range(-1, 2):
            sl = gm._shifted(H, W, j, i)
            if sl is None or (i == 0 and j == 0):
                continue
            P_, Q_ = sl
            g = gm.geometric(np.ones(near[1][1][P_].shape, f32), P_, Q_, normal, position, geo)
            near[j + 1][i + 1][P_] = g > 0
    return near


def near_word(near):
    """the near buffer's word: bit 3 (j + 1) + (i + 1)"""
    word = np.zeros(near[1][1].shape, np.uint32)
    for j in range(3):
        for i in range(3):
            word |= near[j][i].astype(np.uint32) << np.uint32(3 * j + i)
    return word


def robust_denoise_each(planes, N, albedo=None, normal=None, position=None, passes_list=(5,), sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05,
                        gain=1.0, demodulate=True, passes=None):
    """{passes: (denoised RGBA image, variance buffer {lum(c0), v0, var, h})} for every pass count of passes_list, sharing the work the
    counts have in common (`passes` is not read: DEFAULTS may be passed whole).  A plane the parameters do not need may be None; bad
    parameters raise ValueError as the library returns RTGL_ERR_INVALID."""
    if not all(isinstance(k, (int, np.integer)) for k in passes_list) or not all(
            valid_params(k, sigma_lum, sigma_normal, sigma_position, gain) for k in passes_list):
        raise ValueError("invalid parameters")
    planes = np.ascontiguousarray(planes, f32)
    sl, sn, sp = f32(sigma_lum), f32(sigma_normal), f32(sigma_position)
    shape = planes.shape[1:]
    for need, plane, what in ((demodulate, albedo, "albedo"), (sn > 0, normal, "normal"), (sp > 0, position, "position")):
        if need and (plane is None or plane.shape != shape or plane.dtype != f32):
            raise ValueError(f"the {what} plane is needed as float32 of the image's shape")
    H, W = shape[:2]
    res = {}
    with np.errstate(all="ignore"):
        d = divisor(albedo) if demodulate else None
        out, _, v0, h = bucket_variance(planes, N, gain, d)
        c = (out[..., :3] / d).astype(f32) if demodulate else out[..., :3].copy()
        l0 = gm.lum(c)
        geo = gm.geometry(normal, position, sn, sp)
        near = near_mask(normal, position, geo, H, W)
        var = v0
        for L in range(max(passes_list, default=0) + 1):
            if L in passes_list:
                rgb = (c * d) if demodulate else c
                res[L] = (np.concatenate([rgb.astype(f32), out[..., 3:4]], axis=-1), np.stack([l0, v0, var, h.astype(f32)], -1).astype(f32))
            if L < max(passes_list):
                c, var = gm.guided_pass(c, var, 1 << L, sl * sl, normal, position, geo, near)
    return res


def robust_denoise(planes, N, albedo=None, normal=None, position=None, passes=5, **params):
    """(denoised RGBA image, variance buffer {lum(c0), v0, var after the last pass, (float)h}) for one pass count"""
    return robust_denoise_each(planes, N, albedo, normal, position, passes_list=(int(passes),), **params)[int(passes)]
