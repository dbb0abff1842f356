"""numpy float32 restatement of rtgl_temporal_accumulate with option "temporal_moments" and of rtgl_denoise_guided with option
"denoise_variance" = 1 (the contract is in include/rtgl_amd.h, "temporal luminance moments").  A helper, not a test.

Built like tests/temporal_mirror.py, whose camera record and parameter check it uses: vectorised over pixels, a loop over the taps, exactly
the operations the contract lists, in their order; every select is an np.where so that a NaN behaves as defined.  The colour history is
restated here along with the moments (they share taps, weights and blend); tests/test_temporal_moments_mirror.py holds it against
temporal_mirror.run bit for bit.

`accumulate` is one call: (state, inputs) -> state with H (history {rgb, n}) and M (moments {m1, m2, v, n}); `run` steps a sequence of
(image, normal, position, camera, albedo) items and returns every call's (H, M).  `denoise_guided_tvar` is rtgl_denoise_guided over a history
with the v0 select in front of the passes of tests/denoise_guided_mirror.py."""
import numpy as np

from denoise_guided_mirror import DEFAULTS as GUIDED_DEFAULTS
from denoise_guided_mirror import firefly_clamp, geometry, guided_pass, lum, spatial_variance
from denoise_mirror import divisor, dot3, ew
from temporal_mirror import DEFAULTS, RESET, camera_record, check_params, dot, records_equal

f32 = np.float32
MIN_HISTORY = f32(4)            # SVGF's threshold: the temporal variance is used where the history is at least this long


def option(mode):
    """an item of a sequence: rtgl_set_option("temporal_moments", mode)"""
    return ("temporal_moments", mode)


def luminance(image, albedo, mode):
    """(l, l l) of this frame: of I.rgb (mode 1) or of I.rgb / d (mode 2)"""
    x = image[..., :3]
    if mode == 2:
        if albedo is None or albedo.shape != image.shape or albedo.dtype != f32:
            raise ValueError("mode 2 needs the albedo plane as float32 of the image's shape")
        x = x / divisor(albedo)
    l = lum(x.astype(f32))
    return l, l * l


def accumulate(state, image, normal, position, camera, albedo=None, mode=1, max_history=32.0, sigma_normal=0.3, sigma_position=0.05):
    """One call with the option at `mode` (1, 2).  state: None (no history) or what the previous call returned.  Returns dict(H, M, N, P, cam)."""
    if mode not in (1, 2):
        raise ValueError("mode must be 1 or 2")
    mh, sn, sp = check_params(max_history, sigma_normal, sigma_position)
    use_n, use_p = bool(sn > 0), bool(sp > 0)
    image = np.ascontiguousarray(image, f32)
    Hh, W = image.shape[:2]
    if position is None or position.shape != image.shape or position.dtype != f32:
        raise ValueError("the position plane is needed as float32 of the image's shape")
    if use_n and (normal is None or normal.shape != image.shape or normal.dtype != f32):
        raise ValueError("the normal plane is needed as float32 of the image's shape")
    cam = camera_record(camera, W, Hh)
    I = image[..., :3]
    with np.errstate(all="ignore"):
        l, ll = luminance(image, albedo, mode)
        out, n, m1, m2 = I.copy(), np.ones((Hh, W), f32), l, ll
        if state is not None and not (use_n and state["N"] is None):
            prev, Hp, Mp, Np, Pp = state["cam"], state["H"], state["M"], state["N"], state["P"]
            Wf, Hf = f32(W), f32(Hh)
            hit = position[..., 3] > 0
            ix, iy = np.meshgrid(np.arange(W), np.arange(Hh))
            xs = (ix.astype(f32) / Wf) * f32(2) - f32(1)
            ys = (iy.astype(f32) / Hf) * f32(2) - f32(1)
            rw, uh = cam["right"] * cam["wd"], cam["up"] * cam["ht"]
            vm = np.stack([(cam["forward"][c] + rw[c] * xs) + uh[c] * ys for c in range(3)], -1)
            vh = position[..., :3] - prev["position"]
            v = np.where(hit[..., None], vh, vm).astype(f32)
            f = dot(v, prev["forward"])
            sx = ((((dot(v, prev["right"]) / f) * prev["kx"]) + f32(1)) * f32(0.5)) * Wf
            sy = ((((dot(v, prev["up"]) / f) * prev["ky"]) + f32(1)) * f32(0.5)) * Hf
            have = (f > 0) & (sx >= -1) & (sx < Wf) & (sy >= -1) & (sy < Hf)
            if records_equal(prev, cam):
                taps = [(ix, iy, np.ones((Hh, W), f32))]
            else:
                sxs, sys_ = np.where(have, sx, f32(0)), np.where(have, sy, f32(0))
                x0, y0 = np.floor(sxs), np.floor(sys_)
                fx, fy = sxs - x0, sys_ - y0
                x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
                taps = [(x0 + i, y0 + j, (fx if i else f32(1) - fx) * (fy if j else f32(1) - fy)) for j in (0, 1) for i in (0, 1)]
            inn = f32(1) / (sn * sn) if use_n else f32(0)
            if use_p:
                spt = sp * position[..., 3]
                ip = np.where(spt > 0, f32(1) / (spt * spt), f32(0)).astype(f32)
            acc = np.zeros((Hh, W, 3), f32)
            na, ws, a1, a2 = (np.zeros((Hh, W), f32) for _ in range(4))
            for qx, qy, b in taps:
                inside = have & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < Hh)
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, Hh - 1)
                Pq, Hq, Mq = Pp[qy, qx], Hp[qy, qx], Mp[qy, qx]
                w = b
                if use_n:
                    w = w * ew(dot3(Np[qy, qx][..., :3] - normal[..., :3]) * inn)
                if use_p:
                    w = w * ew(dot3(Pq[..., :3] - position[..., :3]) * ip)
                w = np.where(hit, w, b).astype(f32)
                use = inside & ((Pq[..., 3] > 0) == hit) & (w > 0)
                acc = np.where(use[..., None], acc + w[..., None] * Hq[..., :3], acc)
                na = np.where(use, na + w * Hq[..., 3], na)
                ws = np.where(use, ws + w, ws)
                a1 = np.where(use, a1 + w * Mq[..., 0], a1)
                a2 = np.where(use, a2 + w * Mq[..., 1], a2)
            ok = have & (ws > 0)
            safe = np.where(ok, ws, f32(1))
            h = acc / safe[..., None]
            nn = na / safe + f32(1)
            nn = np.where(nn > mh, mh, nn)
            al = f32(1) / nn
            blended = h + (I - h) * al[..., None]
            out = np.where(ok[..., None], blended, I).astype(f32)
            n = np.where(ok, nn, f32(1)).astype(f32)
            h1, h2 = a1 / safe, a2 / safe
            m1 = np.where(ok, h1 + (l - h1) * al, l).astype(f32)
            m2 = np.where(ok, h2 + (ll - h2) * al, ll).astype(f32)
        var = m2 - m1 * m1
        var = np.where(var > 0, var, f32(0)).astype(f32)
    return dict(H=np.concatenate([out, n[..., None]], -1).astype(f32), M=np.stack([m1, m2, var, n], -1).astype(f32),
                N=None if normal is None else normal.copy(), P=position.copy(), cam=cam, mode=mode)


def run(sequence, mode=1, **params):
    """every call's (history, moments) for a sequence of (image, normal, position, camera, albedo) items; an item RESET is
    rtgl_temporal_reset and an item option(k) sets the option: a value different from the current one drops the history"""
    ps = dict(DEFAULTS, **params)
    state, out = None, []
    for item in sequence:
        if isinstance(item, str) and item == RESET:
            state = None
            continue
        if isinstance(item[0], str):
            if item[1] != mode:
                state = None
            mode = item[1]
            continue
        image, normal, position, camera, albedo = item
        state = accumulate(state, image, normal, position, camera, albedo, mode, **ps)
        out.append((state["H"], state["M"]))
    return out


def temporal_v0(moments, v0s):
    """the select of option "denoise_variance" = 1: the variance of the history mean where the history is long enough and the moments finite"""
    M = moments
    with np.errstate(all="ignore"):
        t = (M[..., 3] >= MIN_HISTORY) & (M[..., 0] - M[..., 0] == 0) & (M[..., 1] - M[..., 1] == 0)
        return np.where(t, M[..., 2] / M[..., 3], v0s).astype(f32)


def denoise_guided_tvar_each(history, moments, albedo=None, normal=None, position=None, passes_list=(5,), sigma_lum=4.0, sigma_normal=0.3,
                             sigma_position=0.05, firefly_ratio=1.0, demodulate=True):
    """{passes: (denoised RGBA image, variance buffer {mu, v0, var, s0})}: denoise_guided_mirror.denoise_guided_each over the history with
    v0 chosen by temporal_v0.  The moments must be of mode 2 when demodulating and of mode 1 when not: the library checks, this cannot."""
    sl, sn, sp, fr = f32(sigma_lum), f32(sigma_normal), f32(sigma_position), f32(firefly_ratio)
    image = np.ascontiguousarray(history, f32)
    out = {}
    with np.errstate(all="ignore"):
        d = divisor(albedo) if demodulate else None
        c = (image[..., :3] / d) if demodulate else image[..., :3].copy()
        geo = geometry(normal, position, sn, sp)
        if fr > 0:
            c = firefly_clamp(c, fr, normal, position, geo)
        mu, v0s, s0, near = spatial_variance(c, normal, position, geo)
        v0 = temporal_v0(moments, v0s)
        var = v0
        for L in range(max(passes_list, default=0) + 1):
            if L in passes_list:
                rgb = (c * d) if demodulate else c
                out[L] = (np.concatenate([rgb.astype(f32), image[..., 3:4]], axis=-1), np.stack([mu, v0, var, s0], -1).astype(f32))
            if L < max(passes_list):
                c, var = guided_pass(c, var, 1 << L, sl * sl, normal, position, geo, near)
    return out


def denoise_guided_tvar(history, moments, albedo=None, normal=None, position=None, passes=5, **params):
    ps = dict(GUIDED_DEFAULTS, **params)
    ps.pop("passes")
    return denoise_guided_tvar_each(history, moments, albedo, normal, position, passes_list=(passes,), **ps)[passes]
