"""The contract of rtgl_denoise_guided (include/rtgl_amd.h, "variance-guided denoiser"), pinned through its numpy restatement
(tests/denoise_guided_mirror.py) without a GPU.  tests/test_gpu_denoise_guided.py then holds the kernels to that restatement bit for bit.

1. The mirror and a scalar second restatement agree in every bit, on the value families of tests/denoise_inputs.py too.
2. Properties: the identity, a constant image, one firefly, the accuracy of the variance estimate, no influence across a normal step.
3. Teeth: a third restatement with one switchable defect at a time; each defect changes bits the GPU comparison sees on a listed case.
4. The mirror's NaN share over the value cases stays within the cap the GPU comparison allows itself."""
import numpy as np
import pytest

import denoise_guided_inputs as gi
import denoise_guided_mirror as gm
import denoise_inputs as di
from test_denoise_mirror import random_inputs, synthetic

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def full(params):
    return dict(gm.DEFAULTS, **params)


def mirror(arrays, params):
    return gm.denoise_guided(*arrays, **full(params))


# ---------------------------------------------------------------------------------------------- 1. an independent scalar restatement

def scalar_guided(image, albedo, normal, position, passes, sigma_lum, sigma_normal, sigma_position, firefly_ratio, demodulate):
    """The contract once more, pixel by pixel with float32 scalars and explicit ifs (slow: small images only)"""
    H, W = image.shape[:2]
    one, four, quarter, half, zero, floor = f32(1), f32(4), f32(0.25), f32(0.5), f32(0), f32(2.0 ** -10)
    h = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
    b3 = [quarter, half, quarter]
    sl, sn, sp, fr = f32(sigma_lum), f32(sigma_normal), f32(sigma_position), f32(firefly_ratio)
    inside = lambda x, y: 0 <= x < W and 0 <= y < H

    def ew(x):
        q = one - quarter * x if x < four else zero
        q = q * q
        return q * q

    def dot3(a, b):
        x, y, z = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        return (x * x + y * y) + z * z

    def lum(c):
        return (quarter * c[0] + half * c[1]) + quarter * c[2]

    def geometric(w, x, y, qx, qy, ip):
        if sn > 0:
            w = w * ew(dot3(normal[qy, qx], normal[y, x]) * (one / (sn * sn)))
        if sp > 0:
            w = w * ew(dot3(position[qy, qx], position[y, x]) * ip)
        return w

    with np.errstate(all="ignore"):
        d = [[[(albedo[y, x, k] if albedo[y, x, k] > floor else floor) for k in range(3)] if demodulate else None for x in range(W)] for y in range(H)]
        c0 = [[[(image[y, x, k] / d[y][x][k] if demodulate else image[y, x, k]) for k in range(3)] for x in range(W)] for y in range(H)]
        ip = [[zero] * W for _ in range(H)]
        if sp > 0:
            for y in range(H):
                for x in range(W):
                    spt = sp * position[y, x, 3]
                    ip[y][x] = one / (spt * spt) if spt > 0 else zero
        c = [[c0[y][x] for x in range(W)] for y in range(H)]
        if fr > 0:
            for y in range(H):
                for x in range(W):
                    m = None
                    for j in (-1, 0, 1):
                        for i in (-1, 0, 1):
                            if (i or j) and inside(x + i, y + j) and geometric(one, x, y, x + i, y + j, ip[y][x]) > 0:
                                lq = lum(c0[y + j][x + i])
                                if m is None or lq > m:
                                    m = lq
                    if m is None:
                        continue
                    l, k = lum(c0[y][x]), fr * m
                    if l > k:
                        s = k / l
                        c[y][x] = [c0[y][x][ch] * s for ch in range(3)]
        mu, v0, s0g = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
        for y in range(H):
            for x in range(W):
                s0, s1, s2 = zero, zero, zero
                for j in range(-3, 4):
                    for i in range(-3, 4):
                        qx, qy = x + i, y + j
                        if not inside(qx, qy):
                            continue
                        g = geometric(one, x, y, qx, qy, ip[y][x])
                        lq = lum(c[qy][qx])
                        if g > 0 and lq - lq == 0:
                            s0 = s0 + g
                            s1 = s1 + g * lq
                            s2 = s2 + g * (lq * lq)
                s0g[y, x] = s0
                if s0 > 0:
                    mu[y, x] = s1 / s0
                    v = s2 / s0 - mu[y, x] * mu[y, x]
                    v0[y, x] = v if v > 0 else zero
        var = [[v0[y, x] for x in range(W)] for y in range(H)]
        for L in range(passes):
            s = 1 << L
            nc, nv = [[None] * W for _ in range(H)], [[None] * W for _ in range(H)]
            for y in range(H):
                for x in range(W):
                    vs, vw = zero, zero
                    for j in (-1, 0, 1):
                        for i in (-1, 0, 1):
                            if inside(x + i, y + j) and (not (i or j) or geometric(one, x, y, x + i, y + j, ip[y][x]) > 0):
                                w = b3[j + 1] * b3[i + 1]
                                vs = vs + w * var[y + j][x + i]
                                vw = vw + w
                    il = one / ((sl * sl) * (vs / vw) + f32(2.0 ** -20))
                    acc, ws, va = [zero, zero, zero], zero, zero
                    for j in range(-2, 3):
                        for i in range(-2, 3):
                            qx, qy = x + i * s, y + j * s
                            if not inside(qx, qy):
                                continue
                            dl = lum(c[qy][qx]) - lum(c[y][x])
                            w = h[j + 2] * h[i + 2]
                            w = w * ew((dl * dl) * il)
                            w = geometric(w, x, y, qx, qy, ip[y][x])
                            if w > 0:
                                acc = [acc[k] + w * c[qy][qx][k] for k in range(3)]
                                ws = ws + w
                                va = va + (w * w) * var[qy][qx]
                    nc[y][x] = [acc[k] / ws for k in range(3)] if ws > 0 else c[y][x]
                    nv[y][x] = va / (ws * ws) if ws > 0 else var[y][x]
            c, var = nc, nv
        out = np.zeros((H, W, 4), f32)
        for y in range(H):
            for x in range(W):
                for k in range(3):
                    out[y, x, k] = c[y][x][k] * d[y][x][k] if demodulate else c[y][x][k]
                out[y, x, 3] = image[y, x, 3]
    return out, np.stack([mu, v0, np.array(var, f32).reshape(H, W), s0g], -1).astype(f32)


def scalar(arrays, params):
    kw = full(params)
    return scalar_guided(*arrays, kw["passes"], kw["sigma_lum"], kw["sigma_normal"], kw["sigma_position"], kw["firefly_ratio"], kw["demodulate"])


def assert_same(got, want, label):
    for name, g, w in zip(("image", "variance"), got, want):
        differ = bits(g) != bits(w)
        assert not differ.any(), f"{label}: {name}: {int(differ.sum())} components differ, first at {list(zip(*np.nonzero(differ)))[:4]}"


# (height, width, passes): sizes at which the scalar restatement takes a second or two
SCALAR_RUNS = [(9, 21, 4), (2, 33, 8), (5, 17, 2), (1, 1, 1), (1, 5, 1), (3, 7, 0), (8, 9, 1)]
SCALAR_SETS = [("specials", ps) for ps in gi.SPECIALS_PARAMS] + [("subnormal_weights", ps) for ps in gi.SW_PARAMS] + [("benign", gi.BENIGN_OPEN), ("benign", dict())]


@pytest.mark.filterwarnings("ignore::RuntimeWarning")         # (the scalar restatement's overflows and invalid operations are the point)
@pytest.mark.parametrize("family,params", SCALAR_SETS, ids=[f"{f}-{k}" for k, (f, _) in enumerate(SCALAR_SETS)])
def test_the_mirror_and_the_scalar_restatement_agree_in_every_bit(family, params):
    """image and variance buffer; both restatements run on the same numpy, so NaN signs and payloads agree as well"""
    for H, W, passes in SCALAR_RUNS:
        ps = dict(params, passes=passes)
        arrays = gi.make(family, H, W)
        assert_same(mirror(arrays, ps), scalar(arrays, ps), f"{family} {W} x {H} {ps}")


def test_pass_counts_computed_together_are_those_computed_alone():
    arrays = gi.make("specials", 23, 40)
    each = gm.denoise_guided_each(*arrays, passes_list=(0, 1, 3, 5), **{k: v for k, v in gm.DEFAULTS.items() if k != "passes"})
    for k in (0, 1, 3, 5):
        assert_same(each[k], mirror(arrays, dict(passes=k)), f"passes {k}")


# ---------------------------------------------------------------------------------------------- 2. properties

def test_zero_passes_without_clamp_and_demodulation_is_the_identity():
    for arrays in (random_inputs(20, 31, 1), di.specials(53, 70, 5)):
        out, var = gm.denoise_guided(*arrays, passes=0, firefly_ratio=0.0, demodulate=False)
        assert (bits(out) == bits(arrays[0])).all()
        out, _ = gm.denoise_guided(arrays[0], passes=0, firefly_ratio=-1.0, demodulate=False, sigma_normal=0, sigma_position=0)
        assert (bits(out) == bits(arrays[0])).all()


def test_planes_and_parameters_are_checked():
    img, alb, nrm, pos = random_inputs(8, 8, 2)
    gm.denoise_guided(img, None, None, None, demodulate=False, sigma_normal=0, sigma_position=0)
    for kw in (dict(), dict(demodulate=False), dict(demodulate=False, sigma_normal=0)):
        with pytest.raises(ValueError):
            gm.denoise_guided(img, None, None, None, **kw)
    for kw in (dict(passes=9), dict(passes=-1), dict(sigma_lum=0.0), dict(sigma_lum=-1.0), dict(sigma_lum=float("nan")), dict(sigma_normal=float("inf")),
               dict(firefly_ratio=float("nan")), dict(sigma_position=-float("inf"))):
        with pytest.raises(ValueError):
            gm.denoise_guided(img, alb, nrm, pos, **kw)


@pytest.mark.parametrize("params", [dict(), dict(demodulate=False), dict(passes=8, firefly_ratio=0.0), dict(sigma_normal=0.0, sigma_position=0.0)])
def test_a_constant_image_comes_back_bit_for_bit_with_zero_variance(params):
    """every luminance of a window is the same number l: with the geometric weights off s0 = n, s1 = n l exactly when n l is
    representable (l = 0.75 and n <= 49 are), so mu = l and v = fl(l l) - fl(l l) = 0; with them on, on flat guides g = 1 and the same
    holds.  A weighted mean of equal numbers x with weights that sum exactly: the colours below are dyadic and so are the weights
    h[j] h[i], so acc / ws = x exactly."""
    H, W = 37, 70
    img = np.empty((H, W, 4), f32)
    img[...] = np.array([0.5, 0.75, 1.0, 0.25], f32)
    alb = np.ones((H, W, 4), f32) if not params.get("demodulate", True) else np.full((H, W, 4), 0.5, f32)
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., 2] = 1
    pos = np.zeros((H, W, 4), f32)
    pos[..., 3] = 5
    out, var = gm.denoise_guided(img, alb, nrm, pos, **full(params))
    assert (bits(out) == bits(img)).all()
    assert (var[..., 1] == 0).all() and (var[..., 2] == 0).all()
    lum = gm.lum(img[..., :3] / (alb[..., :3] if params.get("demodulate", True) else f32(1)))
    assert (var[..., 0] == lum).all() and (var[..., 3] >= 16).all() and (var[..., 3] <= 49).all()


def test_one_firefly_leaves_the_clamp_at_its_brightest_neighbours_luminance():
    """One pixel at 1000 x a flat field, firefly_ratio = 1.  k = m = the field's luminance, exactly.  s = fl(k / l) carries one rounding,
    each channel of c1 = fl(c0 s) a second, and lum(c1) three more (its products by 0.25 and 0.5 are exact), all on positive numbers:
    |lum(c1) / k - 1| <= 5 u to first order, u = 2^-24; the test allows 6 u.  With the clamp off the pixel stays as it is."""
    H, W = 21, 30
    u = 2.0 ** -24
    img = np.empty((H, W, 4), f32)
    img[...] = np.array([0.5, 0.25, 0.125, 1.0], f32)
    base = gm.lum(img[0, 0, :3])
    img[10, 12, :3] *= f32(1000)
    assert gm.lum(img[10, 12, :3]) == f32(1000) * base
    with np.errstate(all="ignore"):
        c1 = gm.firefly_clamp(img[..., :3], f32(1))                 # (no geometric terms: every neighbour counts)
    rel = abs(float(gm.lum(c1[10, 12])) / float(base) - 1)
    print(f"clamped luminance / neighbours' luminance - 1 = {rel / u:.2f} u")
    assert rel <= 6 * u
    untouched = np.ones((H, W), bool)
    untouched[10, 12] = False
    assert (bits(c1[untouched]) == bits(img[..., :3][untouched])).all()
    # through the whole call, with and without the guides
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., 2] = 1
    pos = np.zeros((H, W, 4), f32)
    pos[..., 3] = 5
    for planes, kw in (((None, None, None), dict(demodulate=False, sigma_normal=0.0, sigma_position=0.0)), ((None, nrm, pos), dict(demodulate=False))):
        on, _ = gm.denoise_guided(img, *planes, passes=0, firefly_ratio=1.0, **kw)
        assert abs(float(gm.lum(on[10, 12, :3])) / float(base) - 1) <= 6 * u and (bits(on[untouched]) == bits(img[untouched])).all()
        off, var_off = gm.denoise_guided(img, *planes, passes=0, firefly_ratio=0.0, **kw)
        assert (bits(off) == bits(img)).all() and var_off[10, 12, 1] > 1000       # it stays, and the variance estimate sees it
        on5, var_on = gm.denoise_guided(img, *planes, passes=5, firefly_ratio=1.0, **kw)
        # five passes are weighted means of numbers within 6 u of the field's (50 u per pass at most: tests/test_denoise_mirror.py, the albedo
        # test's bound); the moments cancel two sums of about l l = 0.08 that carry some 50 roundings each: noise below 1e-6, against 1,578
        assert np.abs(on5[..., :3].astype(np.float64) / img[0, 0, :3] - 1).max() <= (6 + 50 * 5) * u and var_on[..., 1].max() < 1e-6


def test_the_variance_estimate_is_accurate_on_iid_noise():
    """128 x 128 pixels of mean 1 and i.i.d. noise of standard deviation 0.2 in all channels alike (so the luminance has variance 0.04)
    on a flat guide.  The 7 x 7 sample variance with the 1 / n normalisation has expectation 48/49 of the true one (less at the border,
    where the window is smaller: 16 pixels of 16,384 have n = 16); its sampling error over 16,384 overlapping windows is a fraction of a per
    cent.  Asked: the image mean of v0 within 10 % of the true variance."""
    H = W = 128
    rng = np.random.default_rng(11)
    img = np.ones((H, W, 4), f32)
    img[..., :3] += (rng.standard_normal((H, W, 1)) * 0.2).astype(f32)
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., 2] = 1
    pos = np.zeros((H, W, 4), f32)
    pos[..., 3] = 5
    _, var = gm.denoise_guided(img, None, nrm, pos, passes=0, firefly_ratio=0.0, demodulate=False)
    mean_v0, mean_mu = float(var[..., 1].astype(np.float64).mean()), float(var[..., 0].astype(np.float64).mean())
    print(f"mean v0 {mean_v0:.5f} (true 0.04, ratio {mean_v0 / 0.04:.4f}), mean mu {mean_mu:.5f}")
    assert abs(mean_v0 / 0.04 - 1) < 0.10
    assert abs(mean_mu - 1) < 0.01 and (var[3:-3, 3:-3, 3] == 49).all()
    # and the passes bring the variance down
    _, var5 = gm.denoise_guided(img, None, nrm, pos, passes=5, firefly_ratio=0.0, demodulate=False)
    assert float(var5[..., 2].mean()) < 0.05 * mean_v0


def test_regions_across_a_normal_step_do_not_influence_each_other():
    """|dN|^2 = 2 across the crease and 2 / 0.3^2 > 4, so the normal factor is exactly 0 there: in every pass, in the moments, and for
    the clamp's neighbours and the taps of the variance blur, which is why those two count a neighbour only where its geometric weight
    is > 0.  Changing one face's colours (fireflies included) leaves every bit of the other face alone, image and variance buffer."""
    img, alb, nrm, pos, _ = synthetic(60, 100)
    W = img.shape[1]
    img[::7, W // 2 - 1, :3] *= f32(500)                      # fireflies in the columns next to the crease, on both faces
    img[3::7, W // 2, :3] *= f32(500)
    for kw in (dict(), dict(firefly_ratio=0.0), dict(passes=8, sigma_lum=8.0), dict(passes=0)):
        out, var = gm.denoise_guided(img, alb, nrm, pos, **kw)
        img2 = img.copy()
        img2[:, W // 2:, :3] *= f32(3)
        img2[5::7, W // 2, :3] *= f32(1e4)
        out2, var2 = gm.denoise_guided(img2, alb, nrm, pos, **kw)
        assert (bits(out[:, :W // 2]) == bits(out2[:, :W // 2])).all() and (bits(var[:, :W // 2]) == bits(var2[:, :W // 2])).all(), kw
        assert not (bits(out[:, W // 2:]) == bits(out2[:, W // 2:])).all()
        img3 = img.copy()
        img3[:, :W // 2, :3] += f32(1)
        out3, var3 = gm.denoise_guided(img3, alb, nrm, pos, **kw)
        assert (bits(out[:, W // 2:]) == bits(out3[:, W // 2:])).all() and (bits(var[:, W // 2:]) == bits(var3[:, W // 2:])).all(), kw


# ---------------------------------------------------------------------------------------------- 3. teeth

DEFECTS = {
    "fma": "acc + w c(q) as one fused operation",
    "va_w": "va accumulated with w instead of w w",
    "vg_border": "vg without renormalisation at the border (divided by 1 instead of the weights used)",
    "clamp_centre": "the clamp's maximum includes the pixel itself",
    "moments_5x5": "the moments over 5 x 5 instead of 7 x 7",
    "sigma_halved": "sigma_lum halved from pass to pass",
    "nan_taps": "non-finite luminances counted in the moments",
}


def restate(image, albedo, normal, position, defect=None, passes=5, sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05, firefly_ratio=1.0, demodulate=True):
    """the contract of rtgl_denoise_guided by gathers over index arrays, with at most one of DEFECTS"""
    assert defect is None or defect in DEFECTS
    one, zero = f32(1), f32(0)
    sl, sn, sp, fr = f32(sigma_lum), f32(sigma_normal), f32(sigma_position), f32(firefly_ratio)
    use_n, use_p = bool(sn > 0), bool(sp > 0)
    H, W = image.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]

    def tap(dy, dx):
        qy, qx = yy + dy, xx + dx
        return (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W), np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)

    with np.errstate(all="ignore"):
        c = image[..., :3].astype(f32)
        if demodulate:
            d = np.where(albedo[..., :3] > di.FLOOR, albedo[..., :3], di.FLOOR).astype(f32)
            c = c / d
        inn = one / (sn * sn) if use_n else zero
        if use_p:
            spt = sp * position[..., 3]
            ip = np.where(spt > 0, one / (spt * spt), zero).astype(f32)

        def geometric(w, qy, qx):
            if use_n:
                w = w * gm.ew(gm.dot3(normal[qy, qx, :3] - normal[..., :3]) * inn)
            if use_p:
                w = w * gm.ew(gm.dot3(position[qy, qx, :3] - position[..., :3]) * ip)
            return w

        if fr > 0:
            l0 = gm.lum(c)
            m, have = np.zeros((H, W), f32), np.zeros((H, W), bool)
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    if i == 0 and j == 0 and defect != "clamp_centre":
                        continue
                    ins, qy, qx = tap(j, i)
                    ins = ins & (geometric(np.ones((H, W), f32), qy, qx) > 0)
                    lq = l0[qy, qx]
                    m = np.where(ins, np.where(have, np.where(lq > m, lq, m), lq), m)
                    have = have | ins
            k = fr * m
            hot = have & (l0 > k)
            c = np.where(hot[..., None], c * (k / np.where(hot, l0, one))[..., None], c).astype(f32)
        l1 = gm.lum(c)
        s0, s1, s2 = (np.zeros((H, W), f32) for _ in range(3))
        r = 2 if defect == "moments_5x5" else 3
        for j in range(-r, r + 1):
            for i in range(-r, r + 1):
                ins, qy, qx = tap(j, i)
                g = geometric(np.ones((H, W), f32), qy, qx)
                lq = l1[qy, qx]
                use = ins & (g > 0) & (True if defect == "nan_taps" else (lq - lq == 0))
                s0 = np.where(use, s0 + g, s0)
                s1 = np.where(use, s1 + g * lq, s1)
                s2 = np.where(use, s2 + g * (lq * lq), s2)
        ok = s0 > 0
        safe = np.where(ok, s0, one)
        mu = np.where(ok, s1 / safe, zero).astype(f32)
        v = s2 / safe - mu * mu
        v0 = np.where(ok & (v > 0), v, zero).astype(f32)
        var = v0
        for L in range(passes):
            s = 1 << L
            vs, vw = np.zeros((H, W), f32), np.zeros((H, W), f32)
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    ins, qy, qx = tap(j, i)
                    if i or j:
                        ins = ins & (geometric(np.ones((H, W), f32), qy, qx) > 0)
                    w = gm.B3[j + 1] * gm.B3[i + 1]
                    vs = np.where(ins, vs + w * var[qy, qx], vs)
                    vw = np.where(ins, vw + w, vw)
            vg = vs if defect == "vg_border" else vs / vw
            sig = sl * f32(2.0 ** -L) if defect == "sigma_halved" else sl
            il = one / ((sig * sig) * vg + gm.VAR_FLOOR)
            lc = gm.lum(c)
            acc, ws, va = np.zeros_like(c), np.zeros((H, W), f32), np.zeros((H, W), f32)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    ins, qy, qx = tap(j * s, i * s)
                    cq = c[qy, qx]
                    dl = lc[qy, qx] - lc
                    w = gm.H5[j + 2] * gm.H5[i + 2]
                    w = geometric(w * gm.ew((dl * dl) * il), qy, qx)
                    use = ins & (w > 0)
                    if defect == "fma":
                        new = (acc.astype(np.float64) + w[..., None].astype(np.float64) * cq.astype(np.float64)).astype(f32)
                    else:
                        new = acc + w[..., None] * cq
                    acc = np.where(use[..., None], new, acc)
                    ws = np.where(use, ws + w, ws)
                    va = np.where(use, va + (w if defect == "va_w" else (w * w)) * var[qy, qx], va)
            ok = ws > 0
            safe = np.where(ok, ws, one)
            c = np.where(ok[..., None], acc / safe[..., None], c).astype(f32)
            var = np.where(ok, va / (safe * safe), var).astype(f32)
        out = (c * d) if demodulate else c
    return np.concatenate([out.astype(f32), image[..., 3:4]], axis=-1), np.stack([mu, v0, var, s0], -1).astype(f32)


S70 = (70, 53)


def test_without_a_defect_the_switchable_restatement_is_the_mirror():
    for family, (W, H), ps in [("specials", S70, dict(passes=5)), ("specials", S70, dict(gi.SPECIALS_PARAMS[7], passes=8)),
                               ("specials", (33, 2), dict(demodulate=False, passes=8)), ("subnormal_weights", S70, dict(gi.SW_PARAMS[1], passes=5)),
                               ("subnormal_weights", S70, dict(gi.SW_PARAMS[0], passes=1)), ("ramps", (257, 4), dict(gi.RAMPS_OPEN, passes=8)),
                               ("benign", (65, 5), dict(gi.BENIGN_OPEN, passes=8)), ("ramps", (3, 9), dict(gi.RAMPS_OFF, passes=4))]:
        arrays = gi.make(family, H, W)
        assert_same(restate(*arrays, **full(ps)), mirror(arrays, ps), f"{family} {W} x {H} {ps}")


# per defect: listed cases (family, size, parameter set, passes) that must catch it; at least one has to
CATCHERS = {
    "fma": [("specials", S70, dict(), 1), ("benign", (65, 5), gi.BENIGN_OPEN, 1)],
    "va_w": [("benign", (65, 5), gi.BENIGN_OPEN, 1), ("specials", S70, dict(), 5)],
    "vg_border": [("benign", (65, 5), gi.BENIGN_OPEN, 1), ("specials", S70, dict(), 1)],
    "clamp_centre": [("specials", S70, dict(), 0), ("benign", (65, 5), gi.BENIGN_OPEN, 1)],
    "moments_5x5": [("specials", S70, dict(), 0), ("benign", (65, 5), gi.BENIGN_OPEN, 1)],
    "sigma_halved": [("benign", (65, 5), gi.BENIGN_OPEN, 2), ("specials", S70, dict(), 5)],
    "nan_taps": [("specials", S70, dict(), 0), ("specials", S70, dict(demodulate=False), 1)],
}


def test_every_defect_has_catchers():
    assert set(CATCHERS) == set(DEFECTS)


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_defect_changes_bits_that_the_comparison_sees(defect):
    """`changed`: components of the image or the variance buffer where the mirror's value is not a NaN and the defective restatement's
    bits differ: exactly what the GPU module's comparison rule counts"""
    listed = gi.listed_cases()
    caught = 0
    for family, (W, H), ps, k in CATCHERS[defect]:
        assert any(f == family and size == (W, H) and p == ps and k in counts for f, size, p, counts in listed), f"{family} {W} x {H} {ps} passes {k} is not a case of the GPU module"
        arrays = gi.make(family, H, W)
        want, got = mirror(arrays, dict(ps, passes=k)), restate(*arrays, defect=defect, **full(dict(ps, passes=k)))
        changed = sum(int((~np.isnan(w) & (bits(w) != bits(g))).sum()) for w, g in zip(want, got))
        print(f"{defect} ({DEFECTS[defect]}): {family} {W} x {H} {ps} passes {k}: {changed} components change")
        caught += bool(changed)
    assert caught, f"no listed case sees '{DEFECTS[defect]}'"


# ---------------------------------------------------------------------------------------------- 4. the NaN cap, mirror alone

def test_nan_outputs_of_the_mirror_stay_within_the_cap_on_the_value_cases():
    """per case and pass count, image and variance buffer together: at most 2 % of the components (0 where the inputs are finite)"""
    worst = {}
    for family, (W, H), ps in gi.value_cases():
        arrays = gi.make(family, H, W)
        each = gm.denoise_guided_each(*arrays, passes_list=gi.VALUE_PASSES, **{k: v for k, v in full(ps).items() if k != "passes"})
        for k, (img, var) in each.items():
            share = float((np.isnan(img).sum() + np.isnan(var).sum()) / (img.size + var.size))
            cap = gi.nan_budget(family)
            worst[cap] = max(worst.get(cap, 0.0), share)
            assert share <= cap, f"{family} {W} x {H} {ps} passes {k}: {share:.4%} of the components are NaN, cap {cap:.0%}"
    print(f"largest NaN share per cap: {worst}")
    assert worst[gi.NAN_CAP] > 0                          # (the capped cases do produce NaNs: the rule is exercised)
