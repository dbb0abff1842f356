"""tests/temporal_mirror.py, the numpy restatement of rtgl_temporal_accumulate that tests/test_gpu_temporal.py holds the kernel against, pinned
without a GPU: it equals a second, scalar restatement written from the contract (include/rtgl_amd.h, "temporal accumulation") in every bit
on all generated families; it has the properties the definition promises; and the scalar restatement with one plausible defect at a time
changes bits that are not NaN on a case the GPU module runs, so a kernel with that defect cannot pass there."""
import math

import numpy as np
import pytest

import temporal_inputs as ti
import temporal_mirror as tm

f32 = np.float32
ONE, ZERO, HALF, TWO, FOUR, QUARTER = f32(1), f32(0), f32(0.5), f32(2), f32(4), f32(0.25)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ---------------------------------------------------------------------------------------------- the scalar restatement

def s_ew(x):
    q = ONE - QUARTER * x if x < FOUR else ZERO
    q = q * q
    return q * q


def s_dot3(a, b):
    d = [a[k] - b[k] for k in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def s_dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def s_camera(camera, W, H):
    c = {k: [f32(x) for x in camera["camera_" + k]] for k in ("position", "forward", "up", "right")}
    c["hw"] = f32(math.tan(float(f32(camera["camera_fov"])) * 0.5))
    c["asp"] = f32(H) / f32(W)
    c["wd"] = TWO * c["hw"]
    c["ht"] = TWO * (c["hw"] * c["asp"])
    c["ff"], c["rr"], c["uu"] = s_dot(c["forward"], c["forward"]), s_dot(c["right"], c["right"]), s_dot(c["up"], c["up"])
    c["kx"] = c["ff"] / (c["wd"] * c["rr"])
    c["ky"] = c["ff"] / (c["ht"] * c["uu"])
    return c


def s_equal(a, b):
    for k in a:
        x, y = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        if not all(p == q for p, q in zip(x, y)):
            return False
    return True


DEFECTS = ["columns_outer", "no_division", "nearest_tap", "n_not_capped", "ip_from_tap", "kind_unchecked", "no_static_shortcut", "truncation",
           "alpha_off_by_one", "miss_translated"]


def scalar_call(state, image, normal, position, camera, max_history=32.0, sigma_normal=0.3, sigma_position=0.05, defect=None):
    """one call, pixel by pixel, float32 scalars; defect: one of DEFECTS"""
    H, W = image.shape[:2]
    mh, sn, sp_ = f32(max_history), f32(sigma_normal), f32(sigma_position)
    use_n, use_p = sn > 0, sp_ > 0
    cur = s_camera(camera, W, H)
    out = np.empty((H, W, 4), f32)
    history = state is not None and not (use_n and state["N"] is None)
    if history:
        prev, Hp, Np, Pp = state["cam"], state["H"], state["N"], state["P"]
        static = s_equal(prev, cur) and defect != "no_static_shortcut"
        inn = ONE / (sn * sn) if use_n else ZERO
        Wf, Hf = f32(W), f32(H)
    for py in range(H):
        for px in range(W):
            I, P = image[py, px], position[py, px]
            res, n = [I[0], I[1], I[2]], ONE
            if history:
                hit = P[3] > 0
                if hit:
                    v = [P[k] - prev["position"][k] for k in range(3)]
                else:
                    x = (f32(px) / Wf) * TWO - ONE
                    y = (f32(py) / Hf) * TWO - ONE
                    v = [(cur["forward"][k] + (cur["right"][k] * cur["wd"]) * x) + (cur["up"][k] * cur["ht"]) * y for k in range(3)]
                    if defect == "miss_translated":
                        v = [(cur["position"][k] + v[k]) - prev["position"][k] for k in range(3)]
                f = s_dot(v, prev["forward"])
                sx = ((((s_dot(v, prev["right"]) / f) * prev["kx"]) + ONE) * HALF) * Wf
                sy = ((((s_dot(v, prev["up"]) / f) * prev["ky"]) + ONE) * HALF) * Hf
                if f > 0 and sx >= -1 and sx < Wf and sy >= -1 and sy < Hf:
                    if static:
                        taps = [(px, py, ONE)]
                    else:
                        x0, y0 = (np.trunc(sx), np.trunc(sy)) if defect == "truncation" else (np.floor(sx), np.floor(sy))
                        fx, fy = sx - x0, sy - y0
                        x0, y0 = int(x0), int(y0)
                        if defect == "nearest_tap":
                            taps = [(x0 + (1 if fx >= HALF else 0), y0 + (1 if fy >= HALF else 0), ONE)]
                        else:
                            order = [(i, j) for i in (0, 1) for j in (0, 1)] if defect == "columns_outer" else [(i, j) for j in (0, 1) for i in (0, 1)]
                            taps = [(x0 + i, y0 + j, (fx if i else ONE - fx) * (fy if j else ONE - fy)) for i, j in order]
                    acc, na, ws = [ZERO, ZERO, ZERO], ZERO, ZERO
                    for qx, qy, b in taps:
                        if qx < 0 or qx >= W or qy < 0 or qy >= H:
                            continue
                        Pq = Pp[qy, qx]
                        if (Pq[3] > 0) != hit and defect != "kind_unchecked":
                            continue
                        w = b
                        if hit:
                            if use_n:
                                w = w * s_ew(s_dot3(Np[qy, qx], normal[py, px]) * inn)
                            if use_p:
                                s = sp_ * (Pq[3] if defect == "ip_from_tap" else P[3])
                                ip = ONE / (s * s) if s > 0 else ZERO
                                w = w * s_ew(s_dot3(Pq, P) * ip)
                        if w > 0:
                            Hq = Hp[qy, qx]
                            acc = [acc[k] + w * Hq[k] for k in range(3)]
                            na = na + w * Hq[3]
                            ws = ws + w
                    if ws > 0:
                        h = acc if defect == "no_division" else [acc[k] / ws for k in range(3)]
                        n = na / ws + ONE
                        if defect != "n_not_capped":
                            n = mh if n > mh else n
                        al = ONE / (n - ONE) if defect == "alpha_off_by_one" else ONE / n
                        res = [h[k] + (I[k] - h[k]) * al for k in range(3)]
            out[py, px] = (res[0], res[1], res[2], n)
    return dict(H=out, N=None if normal is None else normal.copy(), P=position.copy(), cam=cur)


def scalar_run(sequence, defect=None, **params):
    state, out = None, []
    with np.errstate(all="ignore"):
        for item in sequence:
            if isinstance(item, str):
                state = None
                continue
            state = scalar_call(state, *item, defect=defect, **dict(tm.DEFAULTS, **params))
            out.append(state["H"])
    return out


_sequences, _mirrors = {}, {}


def sequence(family, size):
    key = (family, size)
    if key not in _sequences:
        _sequences[key] = ti.make(family, size[1], size[0])
    return _sequences[key]


def mirror(family, size, ps):
    key = (family, size, tuple(sorted(ps.items())))
    if key not in _mirrors:
        _mirrors[key] = tm.run(sequence(family, size), **ps)
    return _mirrors[key]


def agrees(got, want):
    """the comparison rule of the GPU module: same bits where the mirror has a number, any NaN where it has a NaN"""
    return all(not np.where(np.isnan(w), ~np.isnan(g), bits(g) != bits(w)).any() for g, w in zip(got, want)) and len(got) == len(want)


# ---------------------------------------------------------------------------------------------- 1. the two restatements agree

SCALAR_SIZES = [(1, 1), (2, 2), (7, 5), (65, 5), (70, 53)]                # (the scalar restatement costs about 50 us per pixel and call)


@pytest.mark.parametrize("family", sorted(ti.FAMILIES))
def test_mirror_equals_the_scalar_restatement(family):
    for size in SCALAR_SIZES:
        for ps in ti.PARAMETER_SETS if size != (70, 53) else ti.PARAMETER_SETS[:1] + ti.PARAMETER_SETS[3:4] + ti.PARAMETER_SETS[5:6]:
            assert (family, size, ps) in ti.listed_cases()
            want, got = mirror(family, size, ps), scalar_run(sequence(family, size), **ps)
            assert agrees(got, want), f"{family} {size} {ps}"
            assert all((np.isnan(g) == np.isnan(w)).all() for g, w in zip(got, want)), f"{family} {size} {ps}: the NaNs are not in the same places"


def test_bad_parameters_raise():
    img, nrm, pos, c = sequence("rest", (7, 5))[0]
    for ps in (dict(max_history=0.5), dict(max_history=float("nan")), dict(sigma_normal=float("inf")), dict(sigma_position=-float("inf"))):
        with pytest.raises(ValueError):
            tm.run([(img, nrm, pos, c)], **ps)
    with pytest.raises(ValueError):
        tm.run([(img, None, pos, c)])
    assert len(tm.run([(img, None, pos, c)], sigma_normal=0.0)) == 1


# ---------------------------------------------------------------------------------------------- 2. the NaN cap

@pytest.mark.parametrize("family", sorted(ti.FAMILIES))
def test_nan_share_of_the_mirror_is_within_the_cap(family):
    """the comparison on the device cannot see into a NaN: at most NAN_CAP of any call's components, and none outside `specials`"""
    seen = 0.0
    for size in ti.SIZES:
        for ps in ti.PARAMETER_SETS:
            for k, h in enumerate(mirror(family, size, ps)):
                share = float(np.isnan(h).mean())
                seen = max(seen, share)
                assert share <= ti.nan_budget(family), f"{family} {size} {ps} call {k}: {share:.4%}"
    if family == "specials":
        assert seen > 0, "the family is there to put NaN and infinities in front of the kernel"


# ---------------------------------------------------------------------------------------------- 3. properties

def test_camera_at_rest_accumulates_a_plain_per_pixel_mean():
    """with every test passing (the same planes every call) the history after k calls is h <- h + (x - h) / n, n = min(k, max_history),
    exactly, per pixel: no resampling"""
    rng = np.random.default_rng(3)
    img, nrm, pos, c = sequence("rest", (70, 53))[0]
    frames = [np.concatenate([rng.random((53, 70, 3)), np.ones((53, 70, 1))], -1).astype(f32) for _ in range(6)]
    for mh in (32.0, 2.5, 1.0):
        out = tm.run([(x, nrm, pos, c) for x in frames], max_history=mh)
        h = frames[0][..., :3].copy()
        for k, x in enumerate(frames):
            n = f32(min(k + 1, mh))
            if k:
                h = h + (x[..., :3] - h) * (ONE / n)
            assert same(out[k][..., :3], h) and (out[k][..., 3] == n).all(), (mh, k)


def plane_views(W, H, D, shifts, rng):
    """a fronto-parallel textured plane at distance D seen by cameras displaced sideways by `shifts` pixels' worth: every quantity is a
    dyadic rational of few bits (W and D powers of two, tan(fov / 2) = 1/2), so the contract's float32 operations are all exact and
    sx - px is exactly the integer shift"""
    fov = f32(2.0 * math.atan(0.5))
    fov = next(float(c) for c in (fov, np.nextafter(fov, f32(0)), np.nextafter(fov, f32(4)), np.nextafter(np.nextafter(fov, f32(0)), f32(0)),
                                  np.nextafter(np.nextafter(fov, f32(4)), f32(4))) if f32(math.tan(float(c) * 0.5)) == HALF)
    unit = 2.0 * D / W                                          # world units per pixel on the plane (wd = 1)
    seq = []
    for s in shifts:
        # right = (-1, 0, 0): a camera displaced by s pixels along its right axis
        c = dict(camera_position=(-s * unit, 0.0, -float(D)), camera_forward=(0.0, 0.0, 1.0), camera_up=(0.0, 1.0, 0.0), camera_right=(-1.0, 0.0, 0.0), camera_fov=fov)
        x = (np.arange(W) / W * 2.0 - 1.0)[None, :] * np.ones((H, 1))
        y = (np.arange(H) / H * 2.0 - 1.0)[:, None] * np.ones((1, W))
        pos = np.stack([-s * unit - D * x, D * (H / W) * y, np.zeros((H, W)), np.full((H, W), float(D))], -1)
        assert (pos.astype(f32).astype(np.float64) == pos).all()
        nrm = np.zeros((H, W, 4), f32)
        nrm[..., 2] = -1
        col = np.round(pos[..., 0] / unit).astype(int)             # the texture: a value per world column and row, plus noise per frame
        img = np.concatenate([np.sin(0.37 * col[..., None] + np.arange(3)) * 0.5 + 0.5 + 0.1 * rng.random((H, W, 3)), np.ones((H, W, 1))], -1).astype(f32)
        seq.append((img, nrm, pos.astype(f32), c))
    return seq


def test_sideways_move_over_a_plane_shifts_the_history_by_whole_pixels():
    """bound on |history - shifted previous history blended with the frame|: 0.  Derivation: with W = 64, D = 32, tan(fov / 2) = 1/2 and a
    displacement of k pixels (k D wd / W = k / 2 world units) v, f = 32, dot(v, right), the quotient, kx = 1 and sx are dyadic rationals of
    at most 12 significant bits, so every operation of the projection is exact and sx = px + k, fx = fy = 0: the one tap with b = 1 is
    pixel (px + k, py), its position equals P(p) bit for bit and its normal too, so w = 1 and h = Hp(px + k, py) exactly.  Measured: 0."""
    W, H, D, k = 64, 16, 32, 3
    rng = np.random.default_rng(5)
    seq = plane_views(W, H, D, [0, 0, k, k, 2 * k], rng)                 # rest, move by k, rest, move by k
    out = tm.run(seq, max_history=1e6)
    assert f32(math.tan(seq[0][3]["camera_fov"] * 0.5)) == HALF
    for c in range(1, len(seq)):
        prev, cur, x = out[c - 1], out[c], seq[c][0][..., :3]
        shift = k if seq[c][3]["camera_position"] != seq[c - 1][3]["camera_position"] else 0
        src = np.arange(W) + shift
        on = src < W
        h = prev[:, src[on], :3]
        n = prev[:, src[on], 3] + ONE
        want = h + (x[:, on] - h) * (ONE / n)[..., None]
        err = float(np.abs(cur[:, on, :3].astype(np.float64) - want.astype(np.float64)).max())
        print(f"call {c}: shift {shift}, largest deviation from the shifted history {err}")
        assert same(cur[:, on, :3], want) and same(cur[:, on, 3], n), c
        assert (cur[:, ~on, 3] == 1).all() and same(cur[:, ~on, :3], x[:, ~on]), f"call {c}: the strip that entered"
    assert (out[-1][:, :W - 2 * k, 3] == 5).all() and (out[-1][:, W - k:, 3] == 1).all()


def test_pure_rotation_over_the_background_keeps_the_history():
    """all-miss pixels: the background's history follows the rotation (a direction keeps its radiance, to bilinear accuracy) and n is not
    reset inside the overlap"""
    W, H = 96, 64
    cams = [ti.cam(yaw=0.0), ti.cam(yaw=0.03), ti.cam(yaw=0.06, pitch=0.02)]
    seq = []
    for c in cams:
        o, d = ti.rays(c, W, H)
        img = np.concatenate([ti.texture(3.0 * d), np.ones((H, W, 1))], -1).astype(f32)              # no noise: the history is the background
        seq.append((img, np.zeros((H, W, 4), f32), np.zeros((H, W, 4), f32), c))
    out = tm.run(seq)
    n = out[-1][..., 3]
    inner = n[8:-8, 8:-8]
    assert (np.abs(inner - 3) < 1e-4).all(), "n restarted inside the overlap"
    assert (n == 1).any(), "nothing entered the view"
    # 12 pixels in from the edges (the view moves by 4.8 pixels a call): both reprojections had all four taps inside the image
    seen = np.zeros(n.shape, bool)
    seen[12:-12, 12:-12] = True
    err = np.abs(out[-1][..., :3] - seq[-1][0][..., :3])[seen].max()
    # every tap lies within a pixel of the direction it stands for and the weights are a convex combination, so each reprojection is off
    # by at most the texture's gradient (3 x (0.4 x 1.3 + 0.4 x 0.7 + 0.02) = 2.46 per unit of direction) over a pixel's diagonal
    # (sqrt(2) x 2 tan(16.5 deg) / 96 = 0.0087): 0.0215; the blend with the exact frame only shrinks it
    bound = 2.46 * math.sqrt(2.0) * 2.0 * math.tan(math.radians(16.5)) / 96
    first = np.abs(seq[0][0][..., :3] - seq[-1][0][..., :3])[seen].max()
    print(f"rotation: history against the rotated background {err:.2e} (bound {bound:.2e}); the first view against it {first:.2e}")
    assert err < bound, f"the history does not follow the rotation: {err}"
    assert first > bound, "a history left in place would pass as well"


def test_depth_step_drops_the_history():
    """a pixel whose previous taps all lie on the other surface gets out = I and n = 1 exactly"""
    for size in ((70, 53), (200, 131)):
        seq = sequence("dolly", size)
        out = tm.run(seq)
        dropped = 0
        for c in range(1, len(seq)):
            img, nrm, pos, camera = seq[c]
            Pp = seq[c - 1][2]
            # hits whose hit point is on the wall (z = 0) while the previous frame saw the near plane (z = -10) in every pixel of the
            # 4 x 4 about the projection: found with the mirror's own projection by asking for n == 1 there
            wall = (pos[..., 3] > 0) & (pos[..., 2] == 0)
            rec_p, rec_c = tm.camera_record(seq[c - 1][3], size[0], size[1]), tm.camera_record(camera, size[0], size[1])
            if tm.records_equal(rec_p, rec_c):
                continue
            v = pos[..., :3].astype(np.float64) - rec_p["position"]
            sx = ((v[..., 0] * rec_p["right"][0] / v[..., 2]) * rec_p["kx"] + 1) * 0.5 * size[0]
            sy = ((v[..., 1] / v[..., 2]) * rec_p["ky"] + 1) * 0.5 * size[1]
            x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
            ok = wall & (x0 >= 0) & (x0 + 1 < size[0]) & (y0 >= 0) & (y0 + 1 < size[1])
            x0, y0 = np.clip(x0, 0, size[0] - 2), np.clip(y0, 0, size[1] - 2)
            near = np.ones(ok.shape, bool)
            for j in (0, 1):
                for i in (0, 1):
                    near &= Pp[y0 + j, x0 + i, 2] == -10
            sel = ok & near
            dropped += int(sel.sum())
            assert (out[c][sel][:, 3] == 1).all() and same(out[c][sel][:, :3], img[sel][:, :3]), (size, c)
        assert dropped > 0, "the sequence has no disocclusion"


def test_points_behind_or_off_screen_have_no_history():
    img, nrm, pos, c0 = sequence("rest", (70, 53))[0]
    # the camera turns round: every hit of the new view is behind the previous camera (f <= 0)
    seq = sequence("behind", (70, 53))
    out = tm.run(seq[:2])
    assert (out[1][..., 3] == 1).all() and same(out[1][..., :3], seq[1][0][..., :3])
    # a camera displaced by far more than the view is wide: everything projects off-screen
    far = ti.cam((500.0, 0.0, -35.0))
    rng = np.random.default_rng(1)
    moved = ti.view(far, 70, 53, ti.STEP, rng)
    out = tm.run([(img, nrm, pos, c0), moved + (far,)], sigma_position=0.0, sigma_normal=0.0)
    hit = moved[2][..., 3] > 0
    assert hit.any() and (~hit).any()
    assert (out[1][hit][:, 3] == 1).all() and same(out[1][hit][:, :3], moved[0][hit][:, :3])
    both = ~hit & ~(pos[..., 3] > 0)
    both[:, [0, -1]] = False                                   # (sx within a rounding of the pixel: the edge columns may look outside)
    both[[0, -1], :] = False
    assert both.any() and (np.abs(out[1][both][:, 3] - 2) < 1e-4).all(), "the background is at infinity: a translation does not move it"


def test_reset_is_equivalent_to_a_first_call():
    seq = sequence("translate", (70, 53))
    out = tm.run(seq[:2] + [tm.RESET] + seq[2:])
    fresh = tm.run(seq[2:])
    assert same(out[2], fresh[0]) and same(out[3], fresh[1]) and (out[2][..., 3] == 1).all()
    # the normal plane switched on between calls: the history is dropped as after a reset
    a, b = seq[0], seq[1]
    out = tm.run([(a[0], None, a[2], a[3])], sigma_normal=0.0)
    state = tm.accumulate(None, a[0], None, a[2], a[3], sigma_normal=0.0)
    second = tm.accumulate(state, *b)
    assert (second["H"][..., 3] == 1).all() and same(second["H"][..., :3], b[0][..., :3])
    third = tm.accumulate(tm.accumulate(state, b[0], None, b[2], b[3], sigma_normal=0.0), *seq[2], sigma_normal=0.0)
    assert (third["H"][..., 3] > 1).any()


# ---------------------------------------------------------------------------------------------- 4. teeth

TEETH = {"columns_outer": ("translate", (70, 53), dict()),
         "no_division": ("translate", (70, 53), dict()),
         "nearest_tap": ("translate", (7, 5), dict()),
         "n_not_capped": ("rest", (7, 5), dict(max_history=2.5)),
         "ip_from_tap": ("dolly", (70, 53), dict()),
         "kind_unchecked": ("rotate", (70, 53), dict(sigma_normal=0.0, sigma_position=-1.0)),
         "no_static_shortcut": ("rest", (70, 53), dict()),
         "truncation": ("translate", (70, 53), dict()),
         "alpha_off_by_one": ("rest", (7, 5), dict()),
         "miss_translated": ("translate", (70, 53), dict())}


@pytest.mark.parametrize("defect", DEFECTS)
def test_a_defect_changes_bits_on_a_listed_case(defect):
    family, size, ps = TEETH[defect]
    assert (family, size, ps) in ti.listed_cases()
    want, got = mirror(family, size, ps), scalar_run(sequence(family, size), defect=defect, **ps)
    changed = sum(int((~np.isnan(w) & ~np.isnan(g) & (bits(g) != bits(w))).sum()) for g, w in zip(got, want))
    assert changed > 0, f"{defect}: {family} {size} {ps} does not see it"
    assert not agrees(got, want)
