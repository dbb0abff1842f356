"""The contract of rtgl_denoise (include/rtgl_amd.h, "denoiser"), pinned on synthetic inputs through its numpy restatement
(tests/denoise_mirror.py), without a GPU.  tests/test_gpu_denoise.py then holds the kernel to that restatement bit for bit."""
import numpy as np
import pytest

import denoise_mirror as dm

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def synthetic(H=270, W=480, seed=0):
    """Two faces with different normals (the crease at W / 2), a checkerboard albedo, multiplicative exponential noise of relative sigma 1"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(f32)
    left = xx < W // 2
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., 2] = np.where(left, 1, 0)
    nrm[..., 0] = np.where(left, 0, 1)
    pos = np.zeros((H, W, 4), f32)
    pos[..., 0] = xx * 0.01
    pos[..., 1] = yy * 0.01
    pos[..., 2] = np.where(left, 0, (xx - W // 2) * 0.01)
    pos[..., 3] = 5 + pos[..., 2]
    alb = np.ones((H, W, 4), f32)
    alb[..., 0] = np.where((xx // 16 + yy // 16) % 2 == 0, 0.8, 0.2)
    alb[..., 1] = 0.5
    alb[..., 2] = 0.3
    illum = np.where(left, 1.0, 0.4)[..., None] * np.ones(3)
    truth = (illum * alb[..., :3]).astype(f32)
    noisy = truth * rng.exponential(1.0, (H, W, 1)).astype(f32)
    img = np.concatenate([noisy, np.ones((H, W, 1), f32)], -1).astype(f32)
    return img, alb, nrm, pos, truth


def rmse(a, truth):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - truth.astype(np.float64)) ** 2)))


# ---------------------------------------------------------------------------------------------- an independent scalar restatement

def scalar_denoise(image, albedo, normal, position, passes, sigma_color, sigma_normal, sigma_position, demodulate):
    """The contract once more, pixel by pixel with float32 scalars and explicit ifs (slow: small images only)"""
    H, W = image.shape[:2]
    one, four, quarter, zero, floor = f32(1), f32(4), f32(0.25), f32(0), f32(2.0 ** -10)
    h = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
    sc, sn, sp = f32(sigma_color), f32(sigma_normal), f32(sigma_position)

    def ew(x):
        q = one - quarter * x if x < four else zero
        q = q * q
        return q * q

    def dot3(a, b):
        x, y, z = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        return (x * x + y * y) + z * z

    d = [[[(albedo[y, x, k] if albedo[y, x, k] > floor else floor) for k in range(3)] if demodulate else None for x in range(W)] for y in range(H)]
    c = [[[(image[y, x, k] / d[y][x][k] if demodulate else image[y, x, k]) for k in range(3)] for x in range(W)] for y in range(H)]
    with np.errstate(all="ignore"):
        for L in range(passes):
            s = 1 << L
            sig = sc * f32(2.0 ** -L)
            ic = one / (sig * sig)
            inn = one / (sn * sn) if sn > 0 else zero
            nxt = [[None] * W for _ in range(H)]
            for y in range(H):
                for x in range(W):
                    ip = zero
                    if sp > 0:
                        spt = sp * position[y, x, 3]
                        ip = one / (spt * spt) if spt > 0 else zero
                    acc, ws = [zero, zero, zero], zero
                    for j in range(-2, 3):
                        for i in range(-2, 3):
                            qx, qy = x + i * s, y + j * s
                            if qx < 0 or qx >= W or qy < 0 or qy >= H:
                                continue
                            w = h[j + 2] * h[i + 2]
                            if sc > 0:
                                w = w * ew(dot3(c[qy][qx], c[y][x]) * ic)
                            if sn > 0:
                                w = w * ew(dot3(normal[qy, qx], normal[y, x]) * inn)
                            if sp > 0:
                                w = w * ew(dot3(position[qy, qx], position[y, x]) * ip)
                            if w > 0:
                                acc = [acc[k] + w * c[qy][qx][k] for k in range(3)]
                                ws = ws + w
                    nxt[y][x] = [acc[k] / ws for k in range(3)] if ws > 0 else c[y][x]
            c = nxt
    out = np.zeros((H, W, 4), f32)
    for y in range(H):
        for x in range(W):
            for k in range(3):
                out[y, x, k] = c[y][x][k] * d[y][x][k] if demodulate else c[y][x][k]
            out[y, x, 3] = image[y, x, 3]
    return out


def random_inputs(H, W, seed):
    rng = np.random.default_rng(seed)
    img = rng.random((H, W, 4), dtype=f32) * f32(2)
    alb = rng.random((H, W, 4), dtype=f32)
    alb[0, 0, :3] = 0                                   # below the floor of the divisor
    nrm = np.zeros((H, W, 4), f32)
    n = rng.normal(size=(H, W, 3))
    nrm[..., :3] = (n / np.linalg.norm(n, axis=2, keepdims=True) * 0.1 + np.array([0, 0, 1.0])).astype(f32)      # nearly parallel: the term stays open
    pos = rng.random((H, W, 4), dtype=f32)
    pos[..., 3] = 4 + pos[..., 2]
    pos[H // 2, W // 2] = 0                             # a miss: t = 0
    return img, alb, nrm, pos


VARIANTS = [dict(), dict(demodulate=False, sigma_color=0.7), dict(sigma_normal=0.0, sigma_position=-1.0), dict(sigma_color=0.0)]
# (the scalar restatement is slow: the large image runs the defaults only)
SIZES = [(H, W, passes, v) for (H, W, passes) in [(3, 3, 5), (1, 1, 3), (5, 17, 4)] for v in range(len(VARIANTS))] + [(53, 70, 5, 0)]


@pytest.mark.parametrize("H,W,passes,variant", SIZES)
def test_taps_outside_the_image_are_skipped_and_every_size_works(H, W, passes, variant):
    """the vectorised restatement against the scalar one: 3 x 3 (every pass has taps outside), 70 x 53 (ragged), with terms off"""
    params = VARIANTS[variant]
    img, alb, nrm, pos = random_inputs(H, W, 7 + H)
    kw = dict(dm.DEFAULTS, passes=passes, **params)
    got = dm.denoise(img, alb, nrm, pos, **kw)
    want = scalar_denoise(img, alb, nrm, pos, kw["passes"], kw["sigma_color"], kw["sigma_normal"], kw["sigma_position"], kw["demodulate"])
    assert np.isfinite(got).all()
    assert (bits(got) == bits(want)).all()


def test_zero_passes_without_demodulation_is_the_identity():
    img, alb, nrm, pos = random_inputs(20, 31, 1)
    img[3, 4, 1] = np.nan
    img[5, 6, 2] = np.inf
    out = dm.denoise(img, passes=0, demodulate=False, sigma_normal=0, sigma_position=0)
    assert (bits(out) == bits(img)).all()
    assert (bits(dm.denoise(img, alb, nrm, pos, passes=0, demodulate=False)) == bits(img)).all()


def test_planes_are_needed_exactly_when_the_parameters_say_so():
    img, alb, nrm, pos = random_inputs(8, 8, 2)
    dm.denoise(img, None, None, None, demodulate=False, sigma_normal=0, sigma_position=0)
    for kw in (dict(), dict(demodulate=False), dict(demodulate=False, sigma_normal=0)):
        with pytest.raises(ValueError):
            dm.denoise(img, None, None, None, **kw)
    for kw in (dict(passes=9), dict(passes=-1), dict(sigma_color=float("nan")), dict(sigma_normal=float("inf"))):
        with pytest.raises(ValueError):
            dm.denoise(img, alb, nrm, pos, **kw)


def test_regions_across_a_normal_step_do_not_influence_each_other():
    """|dN|^2 = 2 across the crease and 2 / 0.3^2 > 4, so the normal factor is exactly 0: changing one face's colours leaves the
    other face's output bits alone"""
    img, alb, nrm, pos, _ = synthetic(90, 160)
    W = img.shape[1]
    out = dm.denoise(img, alb, nrm, pos)
    img2 = img.copy()
    img2[:, W // 2:, :3] *= f32(3)
    out2 = dm.denoise(img2, alb, nrm, pos)
    assert (bits(out[:, :W // 2]) == bits(out2[:, :W // 2])).all()
    assert not (bits(out[:, W // 2:]) == bits(out2[:, W // 2:])).all()
    img3 = img.copy()
    img3[:, :W // 2, :3] += f32(1)
    out3 = dm.denoise(img3, alb, nrm, pos)
    assert (bits(out[:, W // 2:]) == bits(out3[:, W // 2:])).all()


@pytest.mark.parametrize("demodulate", [True, False])
def test_one_nan_pixel_stays_one_nan_pixel(demodulate):
    img, alb, nrm, pos, _ = synthetic(90, 160)
    img[40, 50, 0] = np.nan
    out = dm.denoise(img, alb, nrm, pos, demodulate=demodulate)
    nan = np.isnan(out)
    assert nan.sum() == 1 and nan[40, 50, 0]
    assert np.isfinite(out[~nan]).all()


def test_error_falls_with_every_pass_and_demodulation_keeps_the_texture():
    img, alb, nrm, pos, truth = synthetic()
    errs = [rmse(img, truth)] + [rmse(dm.denoise(img, alb, nrm, pos, passes=k), truth) for k in range(1, 6)]
    print("RMSE unfiltered, 1..5 passes:", [round(e, 5) for e in errs])
    assert all(b < a for a, b in zip(errs, errs[1:])), errs
    flat = rmse(dm.denoise(img, alb, nrm, pos, demodulate=False), truth)
    print("RMSE 5 passes without demodulation:", round(flat, 5))
    assert errs[-1] < flat < errs[0]                    # without demodulation the checkerboard is blurred


def test_a_pure_albedo_texture_under_constant_light_comes_back():
    """I = fl(E A) with E constant per channel.  u = 2^-24.  c0 = fl(I / d) = E (1 + e1)(1 + e2), |e| <= u.  A pass replaces c by
    fl(acc / ws): acc is a sum of at most 25 rounded products with positive terms (relative error <= 25 u to first order: one product, 24
    additions), ws a sum of at most 25 positive terms (<= 24 u), one division (u): a weighted mean of values that all lie within the
    current relative spread around E, moved by at most 50 u.  The result fl(c d) adds u.  So |out / (E A) - 1| <= (3 + 50 passes) u to first
    order; the test allows (3 + 50 passes) u (1 + 2^-10) for the second-order terms.  A filter that blurred the checkerboard (albedo 0.8
    against 0.2) would be off by tens of per cent."""
    img, alb, nrm, pos, _ = synthetic(90, 160)
    E = np.array([0.7, 1.3, 2.1], f32)
    lit = img.copy()
    lit[..., :3] = alb[..., :3] * E
    exact = alb[..., :3].astype(np.float64) * E.astype(np.float64)
    for passes in (0, 1, 5):
        out = dm.denoise(lit, alb, nrm, pos, passes=passes)
        rel = np.abs(out[..., :3].astype(np.float64) / exact - 1).max()
        bound = (3 + 50 * passes) * 2.0 ** -24 * (1 + 2.0 ** -10)
        print(f"passes {passes}: max relative deviation {rel / 2.0 ** -24:.2f} u, bound {bound / 2.0 ** -24:.1f} u")
        assert rel <= bound
        assert (bits(out[..., 3]) == bits(lit[..., 3])).all()
