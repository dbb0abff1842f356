"""The reference of tests/test_gpu_denoise_inputs.py, pinned without a GPU on the inputs of tests/denoise_inputs.py.

1. The numpy restatement (tests/denoise_mirror.py) and the scalar one of tests/test_denoise_mirror.py agree in every bit, NaN payloads
   included, on NaN, infinities, subnormals, albedos around the floor and subnormal tap weights.
2. Teeth.  `restate` below is a third, switchable restatement: without a defect it is the mirror, bit for bit; with one of DEFECTS it is
   wrong in one of the ways the kernel could plausibly be wrong.  Every defect changes output bits, at components where the mirror's
   output is not a NaN, on at least one case the GPU module runs: so a kernel with that defect fails there.
3. The mirror's NaN outputs stay within the budget that the GPU comparison allows itself (denoise_inputs.nan_budget)."""
import time

import numpy as np
import pytest

import denoise_inputs as di
import denoise_mirror as dm
from test_denoise_mirror import scalar_denoise

f32 = np.float32
TINY = np.finfo(f32).tiny


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def full(params):
    return dict(dm.DEFAULTS, **params)


def mirror(arrays, params):
    return dm.denoise(*arrays, **full(params))


def scalar(arrays, params):
    kw = full(params)
    return scalar_denoise(*arrays, kw["passes"], kw["sigma_color"], kw["sigma_normal"], kw["sigma_position"], kw["demodulate"])


# ---------------------------------------------------------------------------------------------- 1. mirror = scalar restatement

# (height, width, passes): sizes at which the scalar restatement takes a second or two
SCALAR_RUNS = [(12, 23, 5), (9, 70, 3), (2, 33, 8), (5, 17, 2), (1, 1, 1), (1, 5, 1), (3, 7, 0)]
SCALAR_SETS = [("specials", ps) for ps in di.SPECIALS_PARAMS] + [("subnormal_weights", ps) for ps in di.VALUE_PARAMS["subnormal_weights"]]


@pytest.mark.filterwarnings("ignore::RuntimeWarning")         # (the scalar restatement's overflows and invalid operations are the point)
@pytest.mark.parametrize("family,params", SCALAR_SETS, ids=[f"{f}-{k}" for k, (f, _) in enumerate(SCALAR_SETS)])
def test_the_mirror_and_the_scalar_restatement_agree_in_every_bit(family, params):
    """every parameter set of the value cases; both restatements run on the same numpy, so NaN signs and payloads agree as well"""
    for H, W, passes in SCALAR_RUNS:
        ps = dict(params, passes=passes)
        arrays = di.make(family, H, W, ps)
        got, want = mirror(arrays, ps), scalar(arrays, ps)
        differ = bits(got) != bits(want)
        assert not differ.any(), f"{family} {W} x {H} {ps}: {int(differ.sum())} components differ, first at {list(zip(*np.nonzero(differ)))[:4]}"


def test_the_families_hold_what_they_promise():
    for H, W in ((8, 8), (53, 70)):
        img, alb, nrm, pos = di.specials(H, W, 3)
        for a, values in ((img, di.COMMON), (alb, np.concatenate([di.COMMON, di.ALBEDO_EXTRA])), (nrm, np.concatenate([di.COMMON, di.NORMAL_EXTRA])),
                          (pos[..., :3], np.concatenate([di.COMMON, di.NORMAL_EXTRA])), (pos[..., 3], np.concatenate([di.COMMON, di.T_EXTRA]))):
            for v in values:
                assert (bits(a) == bits(v)).any(), f"{W} x {H}: value {v!r} (bits {int(bits(v)):#x}) is missing"
        img, alb, _, _ = di.specials(H, W, 3, colours_finite=True)
        assert np.isfinite(img).all() and np.isfinite(alb).all() and (np.abs(img[..., :3]) <= 65504).all()
        assert (alb[..., :3] <= 1).all() and (alb[..., :3][alb[..., :3] < di.FLOOR] >= 0).all()
        assert (di.specials(H, W, 3)[0].view(np.uint32) == di.specials(H, W, 3)[0].view(np.uint32)).all()       # deterministic
    # ramps: every pixel distinct, every value exact
    img = di.ramps(131, 200)[0]
    assert len({tuple(p) for p in img[..., :2].reshape(-1, 2)}) == 131 * 200 and (img == np.round(img)).all()
    # subnormal_weights: the tap between a hot pixel and its neighbour has a subnormal weight under both parameter sets, in every 64-column
    # block, and hot pixels fall into every wave of a block (rows y mod 4 = 0..3 at step 1)
    H, W = 53, 200
    img, alb, nrm, pos = di.subnormal_weights(H, W)
    hot = di.subnormal_weights_hot(H, W)
    for b in range(0, W, 64):
        assert {int(y) % 4 for y in np.nonzero(hot[:, b:b + 64].any(axis=1))[0]} == {0, 1, 2, 3}
    y, x = 3, 67
    assert hot[y, x] and not hot[y, x + 1]
    dn = dm.dot3(nrm[y, x, :3] - nrm[y, x + 1, :3]) * (f32(1) / (f32(0.5) * f32(0.5)))
    dp = dm.dot3(pos[y, x, :3] - pos[y, x + 1, :3]) * f32(1)
    w = f32(3 / 8) * f32(1 / 4) * dm.ew(dn) * dm.ew(dp)
    assert 0 < w < TINY, w
    ic = f32(1) / (f32(1e19) * f32(1e19))
    w_on = w * dm.ew(dm.dot3(img[y, x, :3] - img[y, x + 1, :3]) * ic)
    assert 0 < ic < TINY and 0 < w_on < TINY, (ic, w_on)
    assert float(w) * 1e19 > 1e-3 * 1.4e-20            # ... and it matters: a thousandth of the pixel's own contribution, 10^4 roundings


# ---------------------------------------------------------------------------------------------- 2. teeth

DEFECTS = {
    "ftz_all": "every subnormal input and result is flushed to zero",
    "ftz_w": "only the tap weight w is flushed to zero when it is subnormal",
    "fma": "acc + w c(q) as one fused operation",
    "reciprocal": "acc * (1 / ws) for acc / ws",
    "clamp": "a tap outside the image is clamped to the border instead of skipped",
    "wrap": "a tap outside in x is taken from linear index q anyway (the neighbouring row)",
    "order": "columns outer and rows inner",
    "w_ge": "w >= 0 for w > 0",
    "divisor_max": "the divisor as max(A, 2^-10) with a NaN propagating",
    "ip_tap": "ip from the tap's t instead of the pixel's",
    "sigma_const": "sigma_color not halved per pass",
    "far_taps": "the far taps (i or j = +-2) of a step >= 64 dropped",
}


def ftz(a):
    a = np.asarray(a, f32)
    return np.where(np.abs(a) < TINY, np.copysign(f32(0), a), a).astype(f32)


def restate(image, albedo, normal, position, defect=None, passes=5, sigma_color=16.0, sigma_normal=0.3, sigma_position=0.05, demodulate=True):
    """the contract of rtgl_denoise (include/rtgl_amd.h) by gathers, with at most one of DEFECTS"""
    assert defect is None or defect in DEFECTS
    z = ftz if defect == "ftz_all" else (lambda a: np.asarray(a, f32))
    one, four, quarter, zero = f32(1), f32(4), f32(0.25), f32(0)
    sc, sn, sp = f32(sigma_color), f32(sigma_normal), f32(sigma_position)
    use_c, use_n, use_p = bool(sc > 0), bool(sn > 0), bool(sp > 0)
    H, W = image.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]

    def ew(x):
        q = np.where(x < four, z(one - z(quarter * x)), zero).astype(f32)
        q = z(q * q)
        return z(q * q)

    def dot3(v):
        return z(z(z(v[..., 0] * v[..., 0]) + z(v[..., 1] * v[..., 1])) + z(v[..., 2] * v[..., 2]))

    with np.errstate(all="ignore"):
        c = z(image[..., :3])
        if demodulate:
            a = z(albedo[..., :3])
            d = np.maximum(a, di.FLOOR) if defect == "divisor_max" else np.where(a > di.FLOOR, a, di.FLOOR).astype(f32)
            c = z(c / d)
        N = z(normal[..., :3]) if use_n else None
        P, t = (z(position[..., :3]), z(position[..., 3])) if use_p else (None, None)
        order = [(j, i) for j in range(-2, 3) for i in range(-2, 3)]
        if defect == "order":
            order = [(j, i) for i in range(-2, 3) for j in range(-2, 3)]
        for L in range(passes):
            s = 1 << L
            sig = sc if defect == "sigma_const" else z(sc * f32(2.0 ** -L))
            ic = z(one / z(sig * sig))
            inn = z(one / z(sn * sn)) if use_n else zero
            if use_p:
                spt = z(sp * t)
                ip = np.where(spt > 0, z(one / z(spt * spt)), zero).astype(f32)
            acc, ws = np.zeros_like(c), np.zeros((H, W), f32)
            for j, i in order:
                if defect == "far_taps" and s >= 64 and (abs(i) == 2 or abs(j) == 2):
                    continue
                qy, qx = yy + j * s, xx + i * s
                if defect == "clamp":
                    inside = np.ones((H, W), bool)
                elif defect == "wrap":
                    flat = qy * W + qx
                    inside = (qy >= 0) & (qy < H) & (flat >= 0) & (flat < H * W)
                    qy, qx = np.divmod(np.clip(flat, 0, H * W - 1), W)
                else:
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                cq = c[qy, qx]
                w = np.full((H, W), dm.H5[j + 2] * dm.H5[i + 2], f32)
                if use_c:
                    w = z(w * ew(z(dot3(z(cq - c)) * ic)))
                if use_n:
                    w = z(w * ew(z(dot3(z(N[qy, qx] - N)) * inn)))
                if use_p:
                    w = z(w * ew(z(dot3(z(P[qy, qx] - P)) * (ip[qy, qx] if defect == "ip_tap" else ip))))
                if defect == "ftz_w":
                    w = ftz(w)
                use = inside & ((w >= 0) if defect == "w_ge" else (w > 0))
                if defect == "fma":
                    new = (acc.astype(np.float64) + w[..., None].astype(np.float64) * cq.astype(np.float64)).astype(f32)
                else:
                    new = z(acc + z(w[..., None] * cq))
                acc = np.where(use[..., None], new, acc)
                ws = np.where(use, z(ws + w), ws)
            ok = ws > 0
            safe = np.where(ok, ws, one)
            res = z(acc * z(one / safe)[..., None]) if defect == "reciprocal" else z(acc / safe[..., None])
            c = np.where(ok[..., None], res, c).astype(f32)
        out = z(c * d) if demodulate else c
    return np.concatenate([out.astype(f32), image[..., 3:4]], axis=-1)


def test_without_a_defect_the_switchable_restatement_is_the_mirror():
    for family, (W, H), ps in [("specials", (70, 53), dict(passes=5)), ("specials", (70, 53), dict(sigma_color=0.0, passes=8)),
                               ("specials", (33, 2), dict(demodulate=False, passes=8)), ("subnormal_weights", (70, 53), dict(di.SW_ALL_ON, passes=5)),
                               ("subnormal_weights", (70, 53), dict(di.SW_COLOUR_OFF, passes=1)), ("ramps", (257, 4), dict(di.RAMPS_OPEN, passes=8)),
                               ("benign", (65, 5), dict(di.BENIGN_OPEN, passes=8)), ("ramps", (3, 9), dict(di.RAMPS_OFF, passes=4))]:
        arrays = di.make(family, H, W, ps)
        assert (bits(restate(*arrays, **full(ps))) == bits(mirror(arrays, ps))).all(), (family, W, H, ps)


# per defect: listed cases that must catch it (small ones, so that this stays a test of seconds); at least one has to
S70, S200 = (70, 53), (200, 131)
CATCHERS = {
    "ftz_all": [("specials", S70, dict(passes=1)), ("subnormal_weights", S70, dict(di.SW_ALL_ON, passes=1))],
    "ftz_w": [("subnormal_weights", S70, dict(di.SW_COLOUR_OFF, passes=1)), ("subnormal_weights", S200, dict(di.SW_ALL_ON, passes=5))],
    "fma": [("specials", S70, dict(passes=1)), ("benign", (65, 5), dict(di.BENIGN_OPEN, passes=1))],
    "reciprocal": [("specials", S70, dict(passes=1)), ("ramps", (65, 5), dict(di.RAMPS_OFF, passes=1))],
    "clamp": [("ramps", (65, 5), dict(di.RAMPS_OFF, passes=1)), ("ramps", (1, 5), dict(di.RAMPS_OFF, passes=1))],
    "wrap": [("ramps", (65, 5), dict(di.RAMPS_OFF, passes=1)), ("ramps", (3, 3), dict(di.RAMPS_OPEN, passes=1))],
    "order": [("benign", (65, 5), dict(di.BENIGN_OPEN, passes=1)), ("specials", S70, dict(passes=5))],
    "w_ge": [("specials", S70, dict(passes=1)), ("specials", S70, dict(demodulate=False, passes=5))],
    "divisor_max": [("specials", S70, dict(passes=0)), ("specials", S70, dict(passes=5))],
    "ip_tap": [("benign", (65, 5), dict(di.BENIGN_OPEN, passes=1)), ("specials", S70, dict(sigma_color=0.0, sigma_normal=0.0, passes=1))],
    "sigma_const": [("specials", S70, dict(passes=5)), ("specials", S70, dict(sigma_normal=0.0, sigma_position=0.0, passes=8))],
    "far_taps": [("ramps", (257, 4), dict(di.RAMPS_OFF, passes=7)), ("ramps", (257, 4), dict(di.RAMPS_OPEN, passes=8))],
}


def test_every_defect_has_catchers():
    assert set(CATCHERS) == set(DEFECTS)


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_defect_changes_bits_that_the_comparison_sees(defect):
    """`changed`: components where the mirror's output is not a NaN and the defective restatement's bits differ: exactly what the GPU
    module's comparison rule counts"""
    listed = di.listed_cases()
    caught = 0
    for family, (W, H), ps in CATCHERS[defect]:
        assert (family, (W, H), ps) in listed, f"{family} {W} x {H} {ps} is not a case of the GPU module"
        arrays = di.make(family, H, W, ps)
        want, got = mirror(arrays, ps), restate(*arrays, defect=defect, **full(ps))
        changed = ~np.isnan(want) & (bits(want) != bits(got))
        print(f"{defect} ({DEFECTS[defect]}): {family} {W} x {H} {ps}: {int(changed.sum())} of {changed.size} components change")
        caught += bool(changed.any())
    assert caught, f"no listed case sees '{DEFECTS[defect]}'"


# ---------------------------------------------------------------------------------------------- 3. the NaN budget, mirror alone

def budget_cases():
    """the listed cases on which the budget is checked here: every case of specials and subnormal_weights.  benign and ramps hold finite,
    small numbers (no NaN can arise): they are checked at passes = 8 only, which contains every shorter count's arithmetic; the GPU module
    asserts the budget again on every mirror output it compares against."""
    return [(f, size, ps) for f, size, ps in di.listed_cases() if f in ("specials", "subnormal_weights") or ps["passes"] == 8]


def test_nan_outputs_of_the_mirror_stay_within_the_budget():
    t0 = time.time()
    worst = {}
    for family, (W, H), ps in budget_cases():
        out = mirror(di.make(family, H, W, ps), ps)
        share, cap = float(np.isnan(out).mean()), di.nan_budget(family, ps)
        if share > 0:
            print(f"NaN share {share:.4%} (cap {cap:.0%}): {family} {W} x {H} {ps}")
        worst[cap] = max(worst.get(cap, 0.0), share)
        assert share <= cap, f"{family} {W} x {H} {ps}: {share:.4%} of the components are NaN, cap {cap:.0%}"
    print(f"largest NaN share per cap: {worst}; {len(budget_cases())} cases in {time.time() - t0:.1f} s")
    assert worst[0.02] > 0                                # (the budgeted cases do produce NaNs: the rule is exercised)


def test_zero_passes_without_demodulation_is_the_identity_on_specials():
    for W, H in di.VALUE_SIZES:
        arrays = di.specials(H, W, 5)
        out = mirror(arrays, dict(passes=0, demodulate=False))
        assert (bits(out) == bits(arrays[0])).all()
