"""numpy float32 restatement of rtgl_temporal_clip (the contract is in include/rtgl_amd.h, "temporal clip"), and a second, scalar
restatement written from the same text for tests/test_temporal_clip_mirror.py.  A helper, not a test.

Built like tests/temporal_mirror.py: vectorised over pixels, a loop over the 49 taps, exactly the operations the contract lists, in their
order; every select is an np.where so that a NaN behaves as defined.  np.sqrt of a float32 is the correctly rounded square root the
contract asks for.  Arrays are float32, (rows, width, 4), rows bottom-up like the image.

`clip` is one call: (history, moments or None, image, normal, position) -> (history, moments or None), nothing modified in place.  `run`
steps a sequence the way the library is used: rtgl_temporal_accumulate, then rtgl_temporal_clip, per frame, the next accumulation
reprojecting the clipped history."""
import math

import numpy as np

import temporal_mirror as tm
import temporal_moments_mirror as mm
from denoise_mirror import dot3, ew

f32 = np.float32
DEFAULTS = dict(sigma_scale=2.0, clip_history=3.0, sigma_normal=0.3, sigma_position=0.05)
# one-defect variants of the scalar restatement (tests/test_temporal_clip_mirror.py, "teeth")
DEFECTS = ["box_not_widened", "scale_on_variance", "variance_not_clamped", "window_5x5", "kind_unchecked", "binary_weights", "n_always_cut",
           "n_never_cut", "moments_w_stale", "s2_fused", "hi_before_lo"]


def check_params(sigma_scale, clip_history, sigma_normal, sigma_position):
    if not all(math.isfinite(s) for s in (sigma_scale, clip_history, sigma_normal, sigma_position)):
        raise ValueError("sigma_scale, clip_history and the sigmas must be finite")
    if not f32(sigma_scale) > 0:
        raise ValueError("sigma_scale must be > 0")
    if not f32(clip_history) >= 1:
        raise ValueError("clip_history must be >= 1")
    return f32(sigma_scale), f32(clip_history), f32(sigma_normal), f32(sigma_position)


def _shifted(a, i, j):
    """a(p + (i, j)) for every pixel p, and whether that tap is inside the image; outside, the value is a copy of some pixel, to be ignored"""
    Hh, W = a.shape[:2]
    ys, xs = np.arange(Hh) + j, np.arange(W) + i
    inside = ((ys >= 0) & (ys < Hh))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    return a[np.clip(ys, 0, Hh - 1)][:, np.clip(xs, 0, W - 1)], inside


def window(image, normal, position, sigma_normal=0.3, sigma_position=0.05):
    """(s0, s1, s2) of every pixel: the sums over the taps of its 7 x 7 window that count.  They depend on the frame and on the two sigmas
    only, so `run` can share them between parameter sets."""
    _, _, sn, sp = check_params(1.0, 1.0, sigma_normal, sigma_position)
    use_n, use_p = bool(sn > 0), bool(sp > 0)
    image = np.ascontiguousarray(image, f32)
    Hh, W = image.shape[:2]
    if position is None or position.shape != image.shape or position.dtype != f32:
        raise ValueError("the position plane is needed as float32 of the image's shape")
    if use_n and (normal is None or normal.shape != image.shape or normal.dtype != f32):
        raise ValueError("the normal plane is needed as float32 of the image's shape")
    I = image[..., :3]
    with np.errstate(all="ignore"):
        hit = position[..., 3] > 0
        inn = f32(1) / (sn * sn) if use_n else f32(0)
        if use_p:
            spt = sp * position[..., 3]
            ip = np.where(spt > 0, f32(1) / (spt * spt), f32(0)).astype(f32)
        s0, s1, s2 = np.zeros((Hh, W), f32), np.zeros((Hh, W, 3), f32), np.zeros((Hh, W, 3), f32)
        for j in range(-3, 4):
            for i in range(-3, 4):
                Pq, inside = _shifted(position, i, j)
                c = _shifted(I, i, j)[0]
                g = np.ones((Hh, W), f32)
                if use_n:
                    g = g * ew(dot3(_shifted(normal, i, j)[0][..., :3] - normal[..., :3]) * inn)
                if use_p:
                    g = g * ew(dot3(Pq[..., :3] - position[..., :3]) * ip)
                counts = inside & ((Pq[..., 3] > 0) == hit) & (g > 0) & ((c - c) == 0).all(-1)
                s0 = np.where(counts, s0 + g, s0)
                s1 = np.where(counts[..., None], s1 + g[..., None] * c, s1)
                s2 = np.where(counts[..., None], s2 + g[..., None] * (c * c), s2)
    return s0.astype(f32), s1.astype(f32), s2.astype(f32)


def box(image, normal, position, sigma_scale=2.0, sigma_normal=0.3, sigma_position=0.05, sums=None):
    """(s0, lo, hi) of every pixel: the sum of the weights of the taps that count and the widened colour box (arbitrary where s0 is not > 0);
    sums: what `window` returned for these arrays and sigmas, if the caller has it"""
    ss = check_params(sigma_scale, 1.0, sigma_normal, sigma_position)[0]
    s0, s1, s2 = sums if sums is not None else window(image, normal, position, sigma_normal, sigma_position)
    I = np.ascontiguousarray(image, f32)[..., :3]
    with np.errstate(all="ignore"):
        safe = np.where(s0 > 0, s0, f32(1))[..., None]
        mu = s1 / safe
        v = s2 / safe - mu * mu
        v = np.where(v > 0, v, f32(0))
        e = ss * np.sqrt(v)
        lo, hi = mu - e, mu + e
        lo = np.where(I < lo, I, lo)
        hi = np.where(I > hi, I, hi)
    return s0.astype(f32), lo.astype(f32), hi.astype(f32)


def clip(history, moments, image, normal, position, sigma_scale=2.0, clip_history=3.0, sigma_normal=0.3, sigma_position=0.05, sums=None):
    """One call.  history: {rgb, n}; moments: {m1, m2, v, n} or None.  Returns the two after the call (new arrays)."""
    _, ch, _, _ = check_params(sigma_scale, clip_history, sigma_normal, sigma_position)
    s0, lo, hi = box(image, normal, position, sigma_scale, sigma_normal, sigma_position, sums)
    with np.errstate(all="ignore"):
        x, n = history[..., :3], history[..., 3]
        below = x < lo
        y = np.where(below, lo, x)
        above = y > hi
        y = np.where(above, hi, y)
        ok = s0 > 0
        clipped = ok & (below | above).any(-1)
        out = np.where(ok[..., None], y, x)
        n2 = np.where(clipped & (n > ch), ch, n)
    H2 = np.concatenate([out, n2[..., None]], -1).astype(f32)
    M2 = None
    if moments is not None:
        M2 = moments.copy()
        M2[..., 3] = n2
    return H2, M2


def run(sequence, mode=0, clip_params=None, cache=None, **temporal_params):
    """Every frame's (history after accumulate, history after clip, moments after accumulate or None, moments after clip or None) for a
    sequence of (image, normal, position, camera[, albedo]) items; mode: option "temporal_moments".  clip_params None: no clip calls (the
    histories after clip are then the ones before).  cache: a dict kept by the caller for THIS sequence, in which the window sums of its frames
    are shared between runs."""
    tp = dict(tm.DEFAULTS, **temporal_params)
    state, out = None, []
    for k, item in enumerate(sequence):
        if isinstance(item, str) and item == tm.RESET:
            state = None
            continue
        image, normal, position, camera = item[:4]
        if mode:
            state = mm.accumulate(state, image, normal, position, camera, albedo=item[4] if len(item) > 4 else None, mode=mode, **tp)
        else:
            state = tm.accumulate(state, image, normal, position, camera, **tp)
        H0, M0 = state["H"], state.get("M")
        if clip_params is not None:
            cp = dict(DEFAULTS, **clip_params)
            key = (k, max(float(f32(cp["sigma_normal"])), 0.0), max(float(f32(cp["sigma_position"])), 0.0))
            sums = None if cache is None else cache.get(key)
            if sums is None:
                sums = window(image, normal, position, cp["sigma_normal"], cp["sigma_position"])
                if cache is not None:
                    cache[key] = sums
            H1, M1 = clip(H0, M0, image, normal, position, sums=sums, **cp)
            state = dict(state, H=H1)
            if M1 is not None:
                state["M"] = M1
        else:
            H1, M1 = H0, M0
        out.append((H0, H1, M0, M1))
    return out


# ---------------------------------------------------------------------------------------------- the scalar restatement

ONE, ZERO, FOUR, QUARTER = f32(1), f32(0), f32(4), f32(0.25)


def s_ew(x):
    q = ONE - QUARTER * x if x < FOUR else ZERO
    q = q * q
    return q * q


def s_dot3(a, b):
    d = [a[k] - b[k] for k in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def scalar_clip(history, moments, image, normal, position, sigma_scale=2.0, clip_history=3.0, sigma_normal=0.3, sigma_position=0.05, defect=None,
                pixels=None):
    """one call, pixel by pixel, float32 scalars; defect: one of DEFECTS; pixels: only these (x, y) (the others are copied through)"""
    Hh, W = image.shape[:2]
    ss, ch, sn, sp_ = f32(sigma_scale), f32(clip_history), f32(sigma_normal), f32(sigma_position)
    use_n, use_p = sn > 0, sp_ > 0
    inn = ONE / (sn * sn) if use_n else ZERO
    out = history.copy()
    mom = None if moments is None else moments.copy()
    reach = 2 if defect == "window_5x5" else 3
    todo = pixels if pixels is not None else [(px, py) for py in range(Hh) for px in range(W)]
    with np.errstate(all="ignore"):
        for px, py in todo:
            I, P, Hc = image[py, px], position[py, px], history[py, px]
            hit = P[3] > 0
            if use_p:
                s = sp_ * P[3]
                ip = ONE / (s * s) if s > 0 else ZERO
            s0, s1, s2 = ZERO, [ZERO, ZERO, ZERO], [ZERO, ZERO, ZERO]
            for j in range(-reach, reach + 1):
                for i in range(-reach, reach + 1):
                    qx, qy = px + i, py + j
                    if qx < 0 or qx >= W or qy < 0 or qy >= Hh:
                        continue
                    Pq = position[qy, qx]
                    if (Pq[3] > 0) != hit and defect != "kind_unchecked":
                        continue
                    g = ONE
                    if use_n:
                        g = g * s_ew(s_dot3(normal[qy, qx], normal[py, px]) * inn)
                    if use_p:
                        g = g * s_ew(s_dot3(Pq, P) * ip)
                    if not g > 0:
                        continue
                    if defect == "binary_weights":
                        g = ONE
                    c = image[qy, qx]
                    if not (c[0] - c[0] == 0 and c[1] - c[1] == 0 and c[2] - c[2] == 0):
                        continue
                    s0 = s0 + g
                    for k in range(3):
                        s1[k] = s1[k] + g * c[k]
                        if defect == "s2_fused":
                            s2[k] = f32(np.float64(g * c[k]) * np.float64(c[k]) + np.float64(s2[k]))     # (exact in double, then one rounding)
                        else:
                            s2[k] = s2[k] + g * (c[k] * c[k])
            if not s0 > 0:
                continue
            clipped = False
            n = Hc[3]
            for k in range(3):
                mu = s1[k] / s0
                v = s2[k] / s0 - mu * mu
                if defect != "variance_not_clamped":
                    v = v if v > 0 else ZERO
                e = np.sqrt(ss * v) if defect == "scale_on_variance" else ss * np.sqrt(v)
                lo, hi = mu - e, mu + e
                if defect != "box_not_widened":
                    lo = I[k] if I[k] < lo else lo
                    hi = I[k] if I[k] > hi else hi
                x = Hc[k]
                if defect == "hi_before_lo":
                    above = x > hi
                    y = hi if above else x
                    below = y < lo
                    y = lo if below else y
                else:
                    below = x < lo
                    y = lo if below else x
                    above = y > hi
                    y = hi if above else y
                clipped = clipped or bool(below) or bool(above)
                out[py, px, k] = y
            if defect == "n_always_cut":
                clipped = True
            if defect == "n_never_cut":
                clipped = False
            if clipped and n > ch:
                n = ch
            out[py, px, 3] = n
            if mom is not None and defect != "moments_w_stale":
                mom[py, px, 3] = n
    return out, mom
