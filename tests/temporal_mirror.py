"""numpy float32 restatement of rtgl_temporal_accumulate (the contract is in include/rtgl_amd.h, "temporal accumulation").  A helper, not
a test.

Built like tests/denoise_mirror.py, whose ew and dot3 it uses: vectorised over pixels, a loop over the taps, exactly the operations the
contract lists, in their order; every select is an np.where so that a NaN behaves as defined.  Arrays are float32, (rows, width, 4), rows
bottom-up like the image.  A camera is anything with the camera fields of rtgl_frame_params as attributes or keys (camera_position,
camera_forward, camera_up, camera_right, camera_fov); camera_record builds the record the host builds, the tangent with math.tan in double.

`accumulate` is one call: (state, inputs) -> state, the state being what the library keeps between calls (the history, its copies of the
planes, the camera record); `run` steps a sequence and returns every call's history."""
import math

import numpy as np

from denoise_mirror import dot3, ew

f32 = np.float32
DEFAULTS = dict(max_history=32.0, sigma_normal=0.3, sigma_position=0.05)
RESET = "reset"                 # an item of a sequence: rtgl_temporal_reset
VECTORS = ("position", "forward", "up", "right")
SCALARS = ("hw", "asp", "wd", "ht", "ff", "rr", "uu", "kx", "ky")


def _field(camera, name):
    return camera[name] if isinstance(camera, dict) else getattr(camera, name)


def dot(a, b):
    """a: (..., 3) array or 3 scalars; b: 3 float32 scalars"""
    return (a[..., 0] * b[0] + a[..., 1] * b[1]) + a[..., 2] * b[2]


def camera_record(camera, width, height):
    rec = {k: np.array([f32(x) for x in _field(camera, "camera_" + k)], f32) for k in VECTORS}
    rec["hw"] = f32(math.tan(float(f32(_field(camera, "camera_fov"))) * 0.5))
    rec["asp"] = f32(height) / f32(width)
    rec["wd"] = f32(2) * rec["hw"]
    rec["ht"] = f32(2) * (rec["hw"] * rec["asp"])
    with np.errstate(all="ignore"):
        for k, v in (("ff", "forward"), ("rr", "right"), ("uu", "up")):
            rec[k] = f32(dot(rec[v], rec[v]))
        rec["kx"] = f32(rec["ff"] / (rec["wd"] * rec["rr"]))
        rec["ky"] = f32(rec["ff"] / (rec["ht"] * rec["uu"]))
    return rec


def records_equal(a, b):
    """every field compares equal (a NaN never does)"""
    return all(bool((a[k] == b[k]).all()) for k in VECTORS) and all(bool(a[k] == b[k]) for k in SCALARS)


def check_params(max_history, sigma_normal, sigma_position):
    if not all(math.isfinite(s) for s in (max_history, sigma_normal, sigma_position)):
        raise ValueError("max_history and the sigmas must be finite")
    if not f32(max_history) >= 1:
        raise ValueError("max_history must be >= 1")
    return f32(max_history), f32(sigma_normal), f32(sigma_position)


def accumulate(state, image, normal, position, camera, max_history=32.0, sigma_normal=0.3, sigma_position=0.05):
    """One call.  state: None (no history: the first call, or after a reset) or what the previous call returned.  normal may be None when
    the normal plane is off (then sigma_normal must be <= 0).  Returns dict(H=history {rgb, n}, N=copy of normal or None, P=copy of
    position, cam=camera record)."""
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
    out, n = I.copy(), np.ones((Hh, W), f32)
    if state is not None and not (use_n and state["N"] is None):
        prev, Hp, Np, Pp = state["cam"], state["H"], state["N"], state["P"]
        with np.errstate(all="ignore"):
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
            acc, na, ws = np.zeros((Hh, W, 3), f32), np.zeros((Hh, W), f32), np.zeros((Hh, W), f32)
            for qx, qy, b in taps:
                inside = have & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < Hh)
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, Hh - 1)
                Pq, Hq = Pp[qy, qx], Hp[qy, qx]
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
            ok = have & (ws > 0)
            safe = np.where(ok, ws, f32(1))
            h = acc / safe[..., None]
            nn = na / safe + f32(1)
            nn = np.where(nn > mh, mh, nn)
            al = f32(1) / nn
            blended = h + (I - h) * al[..., None]
            out = np.where(ok[..., None], blended, I).astype(f32)
            n = np.where(ok, nn, f32(1)).astype(f32)
    return dict(H=np.concatenate([out, n[..., None]], -1).astype(f32), N=None if normal is None else normal.copy(), P=position.copy(), cam=cam)


def run(sequence, **params):
    """every call's history for a sequence of (image, normal, position, camera) items; an item RESET is rtgl_temporal_reset"""
    ps = dict(DEFAULTS, **params)
    state, out = None, []
    for item in sequence:
        if isinstance(item, str) and item == RESET:
            state = None
            continue
        state = accumulate(state, *item, **ps)
        out.append(state["H"])
    return out
