"""tests/temporal_moments_mirror.py, the numpy restatement of rtgl_temporal_accumulate with option "temporal_moments" and of
rtgl_denoise_guided with option "denoise_variance" = 1 that tests/test_gpu_temporal_moments.py holds the kernels against, pinned without a
GPU: it equals a second, scalar restatement written from the contract (include/rtgl_amd.h, "temporal luminance moments") in every bit,
moments and history, and its history equals tests/temporal_mirror.py's; it has the properties the definition promises, exactly and
statistically; and a restatement with one plausible defect at a time changes bits that are not NaN on a case the GPU module runs."""
import numpy as np
import pytest

import denoise_guided_mirror as gm
import temporal_inputs as ti
import temporal_mirror as tm
import temporal_moments_inputs as mi
import temporal_moments_mirror as mm
from test_temporal_mirror import ONE, ZERO, HALF, TWO, agrees, bits, s_camera, s_dot, s_dot3, s_equal, s_ew, same

f32 = np.float32
FLOOR = f32(2.0 ** -10)
Q, H_ = f32(0.25), f32(0.5)

# ---------------------------------------------------------------------------------------------- the scalar restatement

DEFECTS = ["alpha_uncapped", "taps_bilinear_only", "not_demodulated", "v_not_clamped", "fused"]
GUIDED_DEFECTS = ["v0_not_divided", "threshold_above_4"]


def s_lum(x):
    return (Q * x[0] + H_ * x[1]) + Q * x[2]


def scalar_call(state, image, normal, position, camera, albedo, mode, max_history=32.0, sigma_normal=0.3, sigma_position=0.05, defect=None):
    """one call, pixel by pixel, float32 scalars: the contract of "temporal accumulation" with the moments' lines added; defect: one of DEFECTS"""
    H, W = image.shape[:2]
    mh, sn, sp_ = f32(max_history), f32(sigma_normal), f32(sigma_position)
    use_n, use_p = sn > 0, sp_ > 0
    cur = s_camera(camera, W, H)
    out, mom = np.empty((H, W, 4), f32), np.empty((H, W, 4), f32)
    history = state is not None and not (use_n and state["N"] is None)
    if history:
        prev, Hp, Mp, Np, Pp = state["cam"], state["H"], state["M"], state["N"], state["P"]
        static = s_equal(prev, cur)
        inn = ONE / (sn * sn) if use_n else ZERO
        Wf, Hf = f32(W), f32(H)
    for py in range(H):
        for px in range(W):
            I, P = image[py, px], position[py, px]
            x = [I[0], I[1], I[2]]
            if mode == 2 and defect != "not_demodulated":
                A = albedo[py, px]
                x = [x[k] / (A[k] if A[k] > FLOOR else FLOOR) for k in range(3)]
            l = s_lum(x)
            ll = l * l
            res, n, m1, m2 = [I[0], I[1], I[2]], ONE, l, ll
            if history:
                hit = P[3] > 0
                if hit:
                    v = [P[k] - prev["position"][k] for k in range(3)]
                else:
                    xs = (f32(px) / Wf) * TWO - ONE
                    ys = (f32(py) / Hf) * TWO - ONE
                    v = [(cur["forward"][k] + (cur["right"][k] * cur["wd"]) * xs) + (cur["up"][k] * cur["ht"]) * ys for k in range(3)]
                f = s_dot(v, prev["forward"])
                sx = ((((s_dot(v, prev["right"]) / f) * prev["kx"]) + ONE) * HALF) * Wf
                sy = ((((s_dot(v, prev["up"]) / f) * prev["ky"]) + ONE) * HALF) * Hf
                if f > 0 and sx >= -1 and sx < Wf and sy >= -1 and sy < Hf:
                    if static:
                        taps = [(px, py, ONE)]
                    else:
                        x0, y0 = np.floor(sx), np.floor(sy)
                        fx, fy = sx - x0, sy - y0
                        x0, y0 = int(x0), int(y0)
                        taps = [(x0 + i, y0 + j, (fx if i else ONE - fx) * (fy if j else ONE - fy)) for j in (0, 1) for i in (0, 1)]
                    acc, na, ws, a1, a2, bs = [ZERO, ZERO, ZERO], ZERO, ZERO, ZERO, ZERO, ZERO
                    for qx, qy, b in taps:
                        if qx < 0 or qx >= W or qy < 0 or qy >= H:
                            continue
                        Pq = Pp[qy, qx]
                        if (Pq[3] > 0) != hit:
                            continue
                        w = b
                        if hit:
                            if use_n:
                                w = w * s_ew(s_dot3(Np[qy, qx], normal[py, px]) * inn)
                            if use_p:
                                s = sp_ * P[3]
                                ip = ONE / (s * s) if s > 0 else ZERO
                                w = w * s_ew(s_dot3(Pq, P) * ip)
                        if w > 0:
                            Hq, Mq = Hp[qy, qx], Mp[qy, qx]
                            acc = [acc[k] + w * Hq[k] for k in range(3)]
                            na = na + w * Hq[3]
                            ws = ws + w
                            wm = b if defect == "taps_bilinear_only" else w
                            a1 = a1 + wm * Mq[0]
                            a2 = a2 + wm * Mq[1]
                            bs = bs + b
                    if ws > 0:
                        h = [acc[k] / ws for k in range(3)]
                        raw = na / ws + ONE
                        n = mh if raw > mh else raw
                        al = ONE / n
                        res = [h[k] + (I[k] - h[k]) * al for k in range(3)]
                        wm = bs if defect == "taps_bilinear_only" else ws
                        h1, h2 = a1 / wm, a2 / wm
                        am = ONE / raw if defect == "alpha_uncapped" else al
                        m1 = h1 + (l - h1) * am
                        m2 = h2 + (ll - h2) * am
            if defect == "fused":
                var = f32(np.float64(m2) - np.float64(m1) * np.float64(m1))          # (the product is exact in double: one rounding, then binary32)
            else:
                var = m2 - m1 * m1
            if defect != "v_not_clamped":
                var = var if var > 0 else ZERO
            out[py, px] = (res[0], res[1], res[2], n)
            mom[py, px] = (m1, m2, var, n)
    return dict(H=out, M=mom, N=None if normal is None else normal.copy(), P=position.copy(), cam=cur)


def scalar_run(sequence, mode, defect=None, **params):
    state, out = None, []
    with np.errstate(all="ignore"):
        for image, normal, position, camera, albedo in sequence:
            state = scalar_call(state, image, normal, position, camera, albedo, mode, defect=defect, **dict(tm.DEFAULTS, **params))
            out.append((state["H"], state["M"]))
    return out


def scalar_v0(M, v0s, defect=None):
    """the select of "denoise_variance" = 1, pixel by pixel"""
    out = np.empty(v0s.shape, f32)
    with np.errstate(all="ignore"):
        for idx in np.ndindex(v0s.shape):
            m = M[idx]
            long_enough = m[3] > 4 if defect == "threshold_above_4" else m[3] >= 4
            t = long_enough and m[0] - m[0] == 0 and m[1] - m[1] == 0
            out[idx] = (m[2] if defect == "v0_not_divided" else m[2] / m[3]) if t else v0s[idx]
    return out


_sequences, _mirrors = {}, {}


def sequence(family, size):
    key = (family, size)
    if key not in _sequences:
        _sequences[key] = mi.make(family, size[1], size[0])
    return _sequences[key]


def mirror(family, size, ps, mode):
    key = (family, size, tuple(sorted(ps.items())), mode)
    if key not in _mirrors:
        _mirrors[key] = mm.run(sequence(family, size), mode, **ps)
    return _mirrors[key]


def flat(results):
    """[(H, M), ...] -> [H, M, H, M, ...] for `agrees`"""
    return [a for pair in results for a in pair]


# ---------------------------------------------------------------------------------------------- 1. the restatements agree

# The whole product the GPU module runs: every family x SIZES x PARAMETER_SETS x modes 1 and 2.  The scalar restatement takes about seven
# minutes over all of it, most at 200 x 131: one case per family, size and mode, so that the cases can be spread over processes.
@pytest.mark.parametrize("mode", mi.MODES)
@pytest.mark.parametrize("size", mi.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", sorted(mi.FAMILIES))
def test_mirror_equals_the_scalar_restatement(family, size, mode):
    for ps in mi.PARAMETER_SETS:
        assert (family, size, ps, mode) in mi.listed_cases()
        want, got = flat(mirror(family, size, ps, mode)), flat(scalar_run(sequence(family, size), mode, **ps))
        assert agrees(got, want), f"{family} {size} {ps} mode {mode}"
        assert all((np.isnan(g) == np.isnan(w)).all() for g, w in zip(got, want)), f"{family} {size} {ps}: the NaNs are not in the same places"


@pytest.mark.parametrize("family", sorted(mi.FAMILIES))
def test_history_component_equals_the_temporal_mirror(family):
    """the history with the option on is the history with it off, bit for bit (a NaN for a NaN), and n rides along in the moments' w"""
    for size in mi.SIZES:
        for ps in mi.PARAMETER_SETS:
            plain = tm.run([item[:4] for item in sequence(family, size)], **ps)
            for mode in mi.MODES:
                got = mirror(family, size, ps, mode)
                assert len(got) == len(plain)
                for k, (h, m) in enumerate(got):
                    assert agrees([h], [plain[k]]) and (np.isnan(h) == np.isnan(plain[k])).all(), f"{family} {size} {ps} mode {mode} call {k}"
                    assert agrees([m[..., 3]], [h[..., 3]])
                    assert not np.isnan(m[..., 2]).any() and (m[..., 2] >= 0).all(), "v is never a NaN and never negative"


def test_inputs_reuse_the_temporal_families():
    assert mi.SIZES is ti.SIZES and mi.PARAMETER_SETS is ti.PARAMETER_SETS and mi.NAN_CAP == ti.NAN_CAP == 0.02
    assert sorted(mi.FAMILIES) == sorted((set(ti.FAMILIES) - {"specials"}) | {"specials_sq"})
    assert 3e38 in ti.COLD, "specials_sq must leave temporal_inputs as it found it"
    for family in ("translate", "behind"):
        for a, b in zip(mi.make(family, 5, 7), ti.make(family, 5, 7)):
            assert all(same(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    a, b = mi.make("specials_sq", 131, 200), ti.make("specials", 131, 200)
    huge = 0
    for x, y in zip(a, b):
        for k in range(3):                                      # image, normal, position: COLD's 3e38 became 1e18 and nothing else changed ...
            changed = bits(x[k]) != bits(y[k])
            was = y[k] == f32(3e38)
            assert was.any() and (x[k][was & changed] == f32(1e18)).all()
            if k:
                assert (changed == was).all()
            else:                                               # ... but for the image's own hot 3e38 values, one pixel in 3000
                hot = x[0] == f32(3e38)
                assert int(hot.sum()) == 200 * 131 // 3000 and ((changed & ~was) <= hot).all() and (was & ~hot <= changed).all()
                huge += int(hot.sum())
    assert huge == len(a) * (200 * 131 // 3000)
    alb = mi.albedo_plane(131, 200, 0)
    low = (alb[..., :3] <= FLOOR).any(-1).mean()
    assert 0.06 < low < 0.09, low
    assert (alb[..., :3][alb[..., :3] > FLOOR] >= 0.19).all()


# ---------------------------------------------------------------------------------------------- 2. the NaN caps

def test_nan_share_is_within_the_cap():
    """moments and history of every call, and both outputs of the guided call over the last history (every parameter set, both modes,
    clamp on and off, passes 0 / 1 / 5): at most NAN_CAP of the components on specials_sq, none anywhere else"""
    worst = dict(moments=0.0, history=0.0, guided=0.0)
    for family in sorted(mi.FAMILIES):
        for size in mi.SIZES:
            for ps in mi.PARAMETER_SETS:
                for mode in mi.MODES:
                    res = mirror(family, size, ps, mode)
                    for k, (h, m) in enumerate(res):
                        for name, a in (("history", h), ("moments", m)):
                            share = float(np.isnan(a).mean())
                            assert share <= mi.nan_budget(family), f"{name}: {family} {size} {ps} mode {mode} call {k}: {share:.4%}"
                            if family == "specials_sq":
                                worst[name] = max(worst[name], share)
                    if family == "specials_sq":
                        for ratio in (1.0, 0.0):
                            for outs in guided_mirror(family, size, ps, mode, ratio).values():
                                for a in outs:
                                    share = float(np.isnan(a).mean())
                                    assert share <= mi.NAN_CAP, f"guided: {size} {ps} mode {mode} ratio {ratio}: {share:.4%}"
                                    worst["guided"] = max(worst["guided"], share)
    print("largest NaN share on specials_sq:", {k: f"{v:.3%}" for k, v in worst.items()})
    assert worst["moments"] > 0 and worst["guided"] > 0, "the family is there to put NaN and infinities in front of the kernels"


# ---------------------------------------------------------------------------------------------- 3. exact properties

def test_constant_radiance_has_zero_variance_exactly():
    """camera at rest, the same radiance every frame: every operation is exact: h1 = (1 l) / 1 = l, m1 = l + 0 al = l, and m2 and m1 m1 are
    both the rounded l l, so v == 0 in every bit whatever the history length"""
    seq = sequence("rest", (70, 53))
    for c in (0.5, 0.3, 1e-3, 7.25):
        img = np.full((53, 70, 4), c, f32)
        const = [(img,) + seq[0][1:] for _ in range(9)]
        for mode in mi.MODES:
            with np.errstate(all="ignore"):
                l, ll = mm.luminance(img, seq[0][4], mode)
            if mode == 1:
                assert (np.abs(l - f32(c)) <= np.spacing(f32(c))).all()
            for mh in (32.0, 4.0):
                res = mm.run(const, mode, max_history=mh)
                assert (res[-1][1][..., 3] == min(9.0, mh)).all()
                for h, m in res:
                    assert same(m[..., 0], l) and same(m[..., 1], ll) and (bits(m[..., 2]) == 0).all(), (c, mode, mh)


def test_no_history_means_this_frames_moments():
    """wherever n == 1 (first call, after a reset, a disocclusion in dolly): m1 = l, m2 = l l, v = 0 exactly"""
    seen = 0
    for family, size in (("dolly", (70, 53)), ("dolly", (200, 131)), ("translate", (70, 53)), ("behind", (70, 53))):
        seq = sequence(family, size)
        for mode in mi.MODES:
            res = mm.run(seq[:2] + [tm.RESET] + seq[2:], mode)
            for k, (h, m) in enumerate(res):
                with np.errstate(all="ignore"):
                    l, ll = mm.luminance(seq[k][0], seq[k][4], mode)
                one = h[..., 3] == 1
                if k in (0, 2):
                    assert one.all()
                elif family == "dolly":
                    seen += int(one.sum())
                assert same(m[one][:, 0], l[one]) and same(m[one][:, 1], ll[one]) and (m[one][:, 2] == 0).all() and (m[one][:, 3] == 1).all()
    assert seen > 0, "the dolly sequences have no disocclusion"


def test_a_change_of_the_option_drops_the_history():
    seq = sequence("translate", (70, 53))
    for a, b in ((1, 2), (2, 1)):
        res = mm.run(seq[:2] + [mm.option(b)] + seq[2:], a)
        fresh = mm.run(seq[2:], b)
        assert (res[1][0][..., 3] > 1).any()
        assert same(res[2][0], fresh[0][0]) and same(res[2][1], fresh[0][1]) and same(res[3][1], fresh[1][1]) and (res[2][0][..., 3] == 1).all()
        # the same value again changes nothing
        again = mm.run(seq[:2] + [mm.option(a)] + seq[2:], a)
        plain = mm.run(seq, a)
        assert all(same(x[0], y[0]) and same(x[1], y[1]) for x, y in zip(again, plain))


def test_mode_2_needs_the_albedo():
    img, nrm, pos, c, alb = sequence("rest", (7, 5))[0]
    with pytest.raises(ValueError):
        mm.run([(img, nrm, pos, c, None)], 2)
    with pytest.raises(ValueError):
        mm.accumulate(None, img, nrm, pos, c, alb, mode=0)
    assert len(mm.run([(img, nrm, pos, c, None)], 1)) == 1


# ---------------------------------------------------------------------------------------------- 4. the statistical check

def test_variance_of_iid_noise_is_the_biased_sample_variance():
    """Camera at rest, 8 frames of i.i.d. grey noise, mean 0.5, variance sigma^2 = 0.04, 128 x 128, max_history >= 8: the history is a plain
    mean of n = 8 samples and v = m2 - m1^2 its biased sample variance, whose expectation is sigma^2 (n - 1) / n = sigma^2 7/8.
    Bound: the mean of v within 5 % of that.  Derivation: the relative standard error of a sample variance of 8 normal samples is
    sqrt(2 / 7); over 16,384 independent pixels, sqrt(2 / 7) / 128 = 0.4 %: 5 % is twelve standard errors."""
    W = Hh = 128
    sigma2 = 0.04
    rng = np.random.default_rng(11)
    c = ti.cam()
    _, nrm, pos = ti.view(c, W, Hh, ti.ROOM, np.random.default_rng(0))
    alb = np.ones((Hh, W, 4), f32)
    seq = []
    for _ in range(8):
        g = rng.normal(0.5, np.sqrt(sigma2), (Hh, W, 1))
        seq.append((np.concatenate([g, g, g, np.ones((Hh, W, 1))], -1).astype(f32), nrm, pos, c, alb))
    for mode in mi.MODES:
        h, m = mm.run(seq, mode, max_history=8.0)[-1]
        assert (m[..., 3] == 8).all()
        ratio = float(m[..., 2].astype(np.float64).mean()) / sigma2
        print(f"mode {mode}: mean v = {ratio:.4f} sigma^2 (expected 7/8 = 0.875)")
        assert abs(ratio - 7.0 / 8.0) <= 0.05 * 7.0 / 8.0, ratio


# ---------------------------------------------------------------------------------------------- 5. denoise_guided_tvar

_guided = {}


def guided_inputs(family, size, ps, mode):
    h, m = mirror(family, size, ps, mode)[-1]
    image, normal, position, camera, albedo = sequence(family, size)[-1]
    return h, m, albedo, normal, position


def guided_mirror(family, size, ps, mode, ratio):
    key = (family, size, tuple(sorted(ps.items())), mode, ratio)
    if key not in _guided:
        h, m, albedo, normal, position = guided_inputs(family, size, ps, mode)
        _guided[key] = mm.denoise_guided_tvar_each(h, m, albedo, normal, position, passes_list=(0, 1, 5), firefly_ratio=ratio, demodulate=mode == 2)
    return _guided[key]


@pytest.mark.parametrize("mode", mi.MODES)
def test_short_histories_fall_back_to_the_spatial_estimate(mode):
    """with every n < 4 the call equals denoise_guided bit for bit"""
    for family, size in (("translate", (70, 53)), ("specials_sq", (70, 53)), ("dolly", (65, 5))):
        for ps in (dict(max_history=2.5), dict(max_history=1.0)):
            h, m, albedo, normal, position = guided_inputs(family, size, ps, mode)
            assert (m[..., 3] < 4).all()
            for ratio in (1.0, 0.0):
                want = gm.denoise_guided_each(h, albedo, normal, position, passes_list=(0, 1, 5), firefly_ratio=ratio, demodulate=mode == 2)
                got = mm.denoise_guided_tvar_each(h, m, albedo, normal, position, passes_list=(0, 1, 5), firefly_ratio=ratio, demodulate=mode == 2)
                for L in (0, 1, 5):
                    assert agrees(got[L], want[L]), (family, size, ps, ratio, L)
    # three calls at rest: n = 3 everywhere
    seq = sequence("rest", (70, 53))
    h, m = mm.run(seq[:3], mode)[-1]
    assert (m[..., 3] == 3).all()
    assert agrees(mm.denoise_guided_tvar(h, m, seq[2][4], seq[2][1], seq[2][2], demodulate=mode == 2),
                  gm.denoise_guided(h, seq[2][4], seq[2][1], seq[2][2], demodulate=mode == 2))


@pytest.mark.parametrize("mode", mi.MODES)
def test_long_histories_use_the_variance_of_the_history_mean(mode):
    """with n >= 4 and finite moments v0 == M.z / M.w bit for bit; elsewhere v0 is the spatial estimate; mu and s0 are always the spatial ones"""
    used = 0
    for family, size in (("rest", (70, 53)), ("translate", (70, 53)), ("dolly", (200, 131)), ("specials_sq", (70, 53))):
        h, m, albedo, normal, position = guided_inputs(family, size, dict(), mode)
        _, var = mm.denoise_guided_tvar(h, m, albedo, normal, position, passes=0, demodulate=mode == 2)
        _, spatial = gm.denoise_guided(h, albedo, normal, position, passes=0, demodulate=mode == 2)
        with np.errstate(all="ignore"):
            t = (m[..., 3] >= 4) & np.isfinite(m[..., 0]) & np.isfinite(m[..., 1])
            assert same(var[t][:, 1], (m[..., 2] / m[..., 3])[t])
        assert same(var[t][:, 2], var[t][:, 1]), "passes = 0: var is v0"
        assert agrees([var[~t][:, 1]], [spatial[~t][:, 1]])
        assert agrees([var[..., 0], var[..., 3]], [spatial[..., 0], spatial[..., 3]])
        assert same(var[..., 1], scalar_v0(m, spatial[..., 1]))
        used += int(t.sum())
        if family == "rest":
            assert t.all()
        if family == "dolly":
            assert t.any() and not t.all()
    assert used > 0


# ---------------------------------------------------------------------------------------------- 6. teeth

TEETH = {"alpha_uncapped": ("rest", (7, 5), dict(max_history=2.5), 1),
         "taps_bilinear_only": ("translate", (70, 53), dict(), 1),
         "not_demodulated": ("rest", (7, 5), dict(), 2),
         "v_not_clamped": ("rest", (70, 53), dict(), 1),
         "fused": ("rest", (70, 53), dict(), 1)}
GUIDED_TEETH = {"v0_not_divided": ("rest", (7, 5), dict(), 1),
                "threshold_above_4": ("rest", (7, 5), dict(), 2)}


@pytest.mark.parametrize("defect", DEFECTS)
def test_a_defect_changes_bits_on_a_listed_case(defect):
    family, size, ps, mode = TEETH[defect]
    assert (family, size, ps, mode) in mi.listed_cases()
    want, got = flat(mirror(family, size, ps, mode)), flat(scalar_run(sequence(family, size), mode, defect=defect, **ps))
    changed = sum(int((~np.isnan(w) & ~np.isnan(g) & (bits(g) != bits(w))).sum()) for g, w in zip(got, want))
    assert changed > 0, f"{defect}: {family} {size} {ps} mode {mode} does not see it"
    assert not agrees(got, want)
    # ... and in the moments only: the history does not depend on them
    assert agrees(got[0::2], want[0::2])


@pytest.mark.parametrize("defect", GUIDED_DEFECTS)
def test_a_defect_of_the_select_changes_bits_on_a_listed_case(defect):
    """the guided call of the GPU module over the last history of a listed case: image and variance buffer"""
    family, size, ps, mode = GUIDED_TEETH[defect]
    assert (family, size, ps, mode) in mi.listed_cases()
    h, m, albedo, normal, position = guided_inputs(family, size, ps, mode)
    want = guided_mirror(family, size, ps, mode, 1.0)

    bad_select = lambda M, v0s: scalar_v0(M, v0s, defect)
    good, mm.temporal_v0 = mm.temporal_v0, bad_select
    try:
        got = mm.denoise_guided_tvar_each(h, m, albedo, normal, position, passes_list=(0, 1, 5), firefly_ratio=1.0, demodulate=mode == 2)
    finally:
        mm.temporal_v0 = good
    for L in (0, 1, 5):
        changed = sum(int((~np.isnan(w) & ~np.isnan(g) & (bits(g) != bits(w))).sum()) for g, w in zip(got[L], want[L]))
        assert changed > 0, f"{defect}: passes {L} does not see it"
    assert (bits(got[5][0][..., :3]) != bits(want[5][0][..., :3])).any(), "the filtered image does not see it"
