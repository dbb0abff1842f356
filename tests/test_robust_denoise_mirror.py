"""The numpy restatement of rtgl_robust_denoise (tests/robust_denoise_mirror.py), without a GPU.

1. Identities of the header: without demodulation v is the v of robust_error_mirror.pixel_error, bit for bit; passes = 0 without
   demodulation is robust_mirror's resolve, bit for bit.
2. A scalar restatement, written pixel by pixel from the header, equals the vectorised mirror on listed cases of the GPU module.
3. Teeth.  The scalar restatement takes at most one of DEFECTS, each a way the kernel could plausibly be wrong; every defect changes
   result bits on named cases that the GPU module runs (CATCHERS).
4. Conditions: the mean of v0 follows sigma^2 / K of normal buckets; on a fine checker under little noise the call keeps what
   rtgl_robust_resolve followed by rtgl_denoise_guided blurs (DESIGN.md 5.15 records the ratio).
5. Every refusal of refused()."""
import numpy as np
import pytest

import denoise_guided_mirror as gm
import robust_denoise_inputs as rdi
import robust_denoise_mirror as rdm
import robust_error_inputs as rei
import robust_error_mirror as rem
import robust_mirror as rm
from denoise_mirror import divisor, dot3, ew

f32 = np.float32
INF = f32(np.inf)


def words(a):
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same(a, b):
    return a.shape == b.shape and bool((words(a) == words(b)).all())


def session_planes(samples, K):
    sess = rm.Session(samples[0].shape[0], samples[0].shape[1], K)
    for s in samples:
        sess.accumulate(s)
    return sess.planes, sess.N


# ---------------------------------------------------------------------------------------------- 1. identities

SPECIAL_SIZES = [(7, 5), (17, 17), (70, 53)]


@pytest.mark.parametrize("K", rdi.BUCKETS)
@pytest.mark.parametrize("family", rdi.SPECIAL_FAMILIES + ("full", "ragged", "outlier", "integer_u"))
def test_without_demodulation_v_is_the_error_estimates_v(family, K):
    """NaN and infinite buckets, ties, all buckets equal, negative and subnormal values, t at 0 and at its cap: v of step 5 (winsorized by
    rank) against the v of the error estimate's step 7 (winsorized by value; error_mirror_v below)"""
    for w, h in SPECIAL_SIZES:
        samples, gains = rdi.samples_of(family, h, w, K)
        planes, N = session_planes(samples, K)
        for gain in gains:
            _, v, v0, hk = rdm.bucket_variance(planes, N, gain)
            want = error_mirror_v(planes, N, gain)
            assert same(v, want), f"{family} {w} x {h} K = {K} gain {gain}"
            assert same(v0, np.where(np.isfinite(want), want, f32(0)).astype(f32))
            t = rm.trim(rm.gini(planes)[2], gain, K, N)
            assert (hk == K - 2 * t).all() and (hk >= 2).all()


def error_mirror_v(planes, N, gain):
    """v of rtgl_robust_error_estimate step 7.  robust_error_mirror.pixel_error returns e = v / (den den), from which v cannot be had
    back exactly, so these are pixel_error's own lines up to v; test_the_copied_lines_are_the_error_mirrors holds them to pixel_error
    through e."""
    planes = np.asarray(planes, f32)
    K = planes.shape[0]
    key, rank, G = rm.gini(planes)
    t = rm.trim(G, gain, K, N)
    with np.errstate(all="ignore"):
        lo = np.zeros(G.shape, f32)
        hi = np.zeros(G.shape, f32)
        for j in range(K):
            lo = np.where(rank[j] == t, key[j], lo)
            hi = np.where(rank[j] == K - 1 - t, key[j], hi)
        w = []
        for j in range(K):
            wj = np.where(key[j] < lo, lo, key[j]).astype(f32)
            w.append(np.where(wj > hi, hi, wj).astype(f32))
        h = (K - 2 * t).astype(np.int32)
        M = np.zeros(G.shape, f32)
        for j in range(K):
            M = M + w[j]
        mw = M / f32(K)
        D = np.zeros(G.shape, f32)
        for j in range(K):
            d = w[j] - mw
            D = D + d * d
        v = (D / (h * (h - 1)).astype(f32)).astype(f32)
    return v


@pytest.mark.parametrize("K", rdi.BUCKETS)
def test_the_copied_lines_are_the_error_mirrors(K):
    """pixel_error's e equals error_mirror_v's v over pixel_error's den den, bit for bit"""
    for family in ("ragged", "specials", "negative", "nonfinite", "overflow"):
        samples, gains = rdi.samples_of(family, 17, 17, K)
        planes, N = session_planes(samples, K)
        for gain in gains:
            key, rank, G = rm.gini(planes)
            t = rm.trim(G, gain, K, N)
            with np.errstate(all="ignore"):
                T = np.zeros(G.shape, f32)
                for j in range(K):
                    T = np.where((t <= rank[j]) & (rank[j] <= K - 1 - t), T + key[j], T).astype(f32)
                mu = T / (K - 2 * t).astype(f32)
                den = np.where(mu > 0, mu, f32(0)).astype(f32) + f32(0.01)
                e = (error_mirror_v(planes, N, gain) / (den * den)).astype(f32)
            assert same(e, rem.pixel_error(planes, N, gain, 0.01)[0]), f"{family} K = {K} gain {gain}"


@pytest.mark.parametrize("K", rdi.BUCKETS)
def test_no_passes_without_demodulation_is_the_resolve(K):
    for family in rdi.BUCKET_FAMILIES:
        w, h = 17, 9
        samples, gains = rdi.samples_of(family, h, w, K)
        planes, N = session_planes(samples, K)
        alb, nrm, pos = rdi.guides_of("specials", h, w)
        for gain in gains:
            got, var = rdm.robust_denoise(planes, N, alb, nrm, pos, **dict(rdm.DEFAULTS, passes=0, demodulate=False, gain=gain))
            assert same(got, rm.image_plane(planes, N, gain)), f"{family} K = {K} gain {gain}"
            assert same(var[..., 1], var[..., 2])


# ---------------------------------------------------------------------------------------------- 2. the scalar restatement

DEFECTS = {
    "winsor_by_value": "w_j = min(max(x_j, lo), hi): the demodulated luminances clamped by value, not by the resolve's ranks",
    "keys_not_demodulated": "x_j = key_j although the call demodulates",
    "divide_by_K": "v = D / (K (K - 1)) instead of D / (h (h - 1))",
    "lo_hi_swapped": "lo is the x of rank K - 1 - t and hi the x of rank t",
    "alpha_of_bucket_0": "a = b_0.w instead of out.w",
    "v0_keeps_nonfinite": "v0 = v even where v is not finite",
    "near_without_position": "the near neighbours from the normal factor alone",
    "near_by_image_only": "every neighbour inside the image is near",
    "unweighted_mean": "out is the plain mean of the kept buckets, not weighted by n_j",
    "mw_over_h": "mw = M / h instead of M / K",
}


def lum3(r, g, b):
    return (f32(0.25) * r + f32(0.5) * g) + f32(0.25) * b


def scalar_prepare(planes, N, alb, nrm, pos, sigma_normal, sigma_position, gain, demodulate, defect=None):
    """steps 1-6 and the stores of a call with passes = 0, pixel by pixel: (denoised (h, w, 4), variance (h, w, 4), near word (h, w))"""
    assert defect is None or defect in DEFECTS
    K, H, W = planes.shape[:3]
    sn, sp, gain = f32(sigma_normal), f32(sigma_position), f32(gain)
    use_n, use_p = bool(sn > 0), bool(sp > 0)
    inn = f32(1) / (sn * sn) if use_n else f32(0)
    n_j = rm.bucket_samples(N, K)
    out_img, var_img, near_img = np.zeros((H, W, 4), f32), np.zeros((H, W, 4), f32), np.zeros((H, W), np.uint32)
    cap = (K - 1) // 2
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                b = [planes[j, y, x] for j in range(K)]
                l = [lum3(v[0], v[1], v[2]) for v in b]
                key = [v if np.isfinite(v) else INF for v in l]
                rank = [sum(1 for i in range(K) if i != j and (key[i] < key[j] or (key[i] == key[j] and i < j))) for j in range(K)]
                S = A = f32(0)
                for j in range(K):
                    S = S + key[j]
                    A = A + f32(2 * rank[j] - (K - 1)) * key[j]
                if not np.isfinite(S):
                    G = f32(1)
                elif not S > 0:
                    G = f32(0)
                else:
                    G = A / (f32(K) * S)
                if not G <= 1:
                    G = f32(1)
                if not G >= 0:
                    G = f32(0)
                u = (G * gain) * f32(K // 2)
                t = cap if u >= f32(cap) else int(u)
                Wsum, Csum = f32(0), np.zeros(4, f32)
                for j in range(K):
                    if t <= rank[j] <= K - 1 - t:
                        fn = f32(1) if defect == "unweighted_mean" else f32(n_j[j])
                        Wsum = Wsum + fn
                        Csum = (Csum + fn * b[j]).astype(f32)
                out = (Csum / Wsum).astype(f32)
                if demodulate:
                    d = np.array([a if a > f32(2.0 ** -10) else f32(2.0 ** -10) for a in alb[y, x, :3]], f32)
                    c0 = (out[:3] / d).astype(f32)
                else:
                    d, c0 = None, out[:3].copy()
                xs = []
                for j in range(K):
                    if demodulate and defect != "keys_not_demodulated":
                        v = lum3(b[j][0] / d[0], b[j][1] / d[1], b[j][2] / d[2])
                        xs.append(v if np.isfinite(v) else INF)
                    else:
                        xs.append(key[j])
                r_lo, r_hi = (K - 1 - t, t) if defect == "lo_hi_swapped" else (t, K - 1 - t)
                lo, hi = xs[rank.index(r_lo)], xs[rank.index(r_hi)]
                if defect == "winsor_by_value":
                    ws = [min(max(v, lo), hi) for v in xs]
                else:
                    ws = [lo if rank[j] < t else (hi if rank[j] > K - 1 - t else xs[j]) for j in range(K)]
                M = f32(0)
                for v in ws:
                    M = M + v
                hk = K - 2 * t
                mw = M / f32(hk if defect == "mw_over_h" else K)
                D = f32(0)
                for v in ws:
                    dd = v - mw
                    D = D + dd * dd
                v = D / f32(K * (K - 1) if defect == "divide_by_K" else hk * (hk - 1))
                v0 = v if (v - v == 0 or defect == "v0_keeps_nonfinite") else f32(0)
                near = 1 << 4
                if use_p:
                    spt = sp * pos[y, x, 3]
                    ip = f32(1) / (spt * spt) if spt > 0 else f32(0)
                for j in (-1, 0, 1):
                    for i in (-1, 0, 1):
                        qx, qy = x + i, y + j
                        if (i == 0 and j == 0) or not (0 <= qx < W and 0 <= qy < H):
                            continue
                        g = f32(1)
                        if defect != "near_by_image_only":
                            if use_n:
                                g = g * ew(dot3(nrm[qy, qx, :3] - nrm[y, x, :3]) * inn)
                            if use_p and defect != "near_without_position":
                                g = g * ew(dot3(pos[qy, qx, :3] - pos[y, x, :3]) * ip)
                        if g > 0:
                            near |= 1 << (3 * (j + 1) + (i + 1))
                rgb = (c0 * d).astype(f32) if demodulate else c0
                out_img[y, x, :3] = rgb
                out_img[y, x, 3] = b[0][3] if defect == "alpha_of_bucket_0" else out[3]
                var_img[y, x] = (lum3(c0[0], c0[1], c0[2]), v0, v0, f32(hk))
                near_img[y, x] = near
    return out_img, var_img, near_img


def mirror_prepare(planes, N, alb, nrm, pos, params):
    p = dict(rdm.DEFAULTS, **params)
    got = rdm.robust_denoise(planes, N, alb, nrm, pos, **dict(p, passes=0))
    with np.errstate(all="ignore"):
        geo = gm.geometry(nrm, pos, f32(p["sigma_normal"]), f32(p["sigma_position"]))
        near = rdm.near_word(rdm.near_mask(nrm, pos, geo, *planes.shape[1:3]))
    return got[0], got[1], near


def scalar_of(planes, N, alb, nrm, pos, params, defect=None):
    p = dict(rdm.DEFAULTS, **params)
    return scalar_prepare(planes, N, alb, nrm, pos, p["sigma_normal"], p["sigma_position"], p["gain"], p["demodulate"], defect)


def differing(a, b):
    return [name for name, u, v in zip(("denoised", "variance", "near"), a, b)
            if not (same(u, v) if u.dtype == np.float32 else bool((u == v).all()))]


SCALAR_CASES = [c for c in rdi.listed_cases() if c[2] in ((3, 2), (65, 5)) and c[3] in (4, 8)]


def test_the_scalar_restatement_equals_the_mirror():
    assert len(SCALAR_CASES) >= 20
    for family, guides, (w, h), K, sets in SCALAR_CASES:
        case = rdi.make(family, guides, h, w, K, sets)
        planes, N = session_planes(case["samples"], K)
        arrays = (case["albedo"], case["normal"], case["position"])
        for params in case["params"]:
            assert differing(mirror_prepare(planes, N, *arrays, params), scalar_of(planes, N, *arrays, params)) == [], f"{family} / {guides} {w} x {h} K = {K} {params}"


def test_the_nan_share_of_every_listed_case_is_within_its_budget():
    """what the GPU module's comparison cannot see into stays as small as robust_denoise_inputs.nan_budget reasons, and most cases have none"""
    clean = 0
    for family, guides, (w, h), K, sets in rdi.listed_cases():
        case = rdi.make(family, guides, h, w, K, sets)
        planes, N = session_planes(case["samples"], K)
        arrays = (case["albedo"], case["normal"], case["position"])
        for params in case["params"]:
            p = dict(rdm.DEFAULTS, **params)
            budget = rdi.nan_budget(planes, arrays[0] if p["demodulate"] else None)
            clean += budget == 0
            for k, (img, var) in rdm.robust_denoise_each(planes, N, *arrays, passes_list=rdi.PASSES, **p).items():
                for what, a in (("denoised", img), ("variance", var)):
                    assert float(np.isnan(a).mean()) <= budget, f"{family} / {guides} {w} x {h} K = {K} {params} passes {k}: {what}"
    assert clean >= len(rdi.listed_cases())                            # (of twice as many runs)


# ---------------------------------------------------------------------------------------------- 3. teeth

S65, S3 = (65, 5), (3, 2)


def case_of(family, size, K):
    hits = [c for c in rdi.listed_cases() if c[0] == family and c[2] == size and c[3] == K]
    assert len(hits) == 1, f"{family} {size} K = {K} is not a case of the GPU module"
    return hits[0]


CATCHERS = {
    "winsor_by_value": [("long", S65, 8), ("ragged", S65, 16)],
    "keys_not_demodulated": [("full", S65, 4), ("long", S65, 8), ("ragged", S65, 16)],
    "divide_by_K": [("long", S65, 8), ("ragged", S65, 4), ("gain_huge", S65, 16)],
    "lo_hi_swapped": [("long", S65, 4), ("gain_huge", S65, 4), ("full", S65, 8)],
    "alpha_of_bucket_0": [("specials", S65, 8), ("specials", S65, 4)],
    "v0_keeps_nonfinite": [("nonfinite", S65, 8), ("overflow", S65, 4)],
    "near_without_position": [("gain_zero", S65, 4), ("full", S65, 8), ("ragged", S65, 16)],      # (guides whose position factor closes where the normal's is open)
    "near_by_image_only": [("ragged", S65, 4), ("long", S65, 8), ("gain_zero", S65, 4)],
    "unweighted_mean": [("long", S65, 8), ("ragged", S65, 4), ("gain_zero", S65, 16)],
    "mw_over_h": [("long", S65, 8), ("ragged", S65, 16)],
}


def test_every_defect_has_catchers():
    assert set(CATCHERS) == set(DEFECTS)


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_defect_changes_bits_that_the_comparison_sees(defect):
    caught = 0
    for family, size, K in CATCHERS[defect]:
        family, guides, (w, h), K, sets = case_of(family, size, K)
        case = rdi.make(family, guides, h, w, K, sets)
        planes, N = session_planes(case["samples"], K)
        arrays = (case["albedo"], case["normal"], case["position"])
        changed = []
        for params in case["params"]:
            changed += differing(mirror_prepare(planes, N, *arrays, params), scalar_of(planes, N, *arrays, params, defect))
        print(f"{defect} ({DEFECTS[defect]}): {family} / {guides} {w} x {h} K = {K}: {sorted(set(changed))} change")
        caught += bool(changed)
    assert caught == len(CATCHERS[defect]), f"a listed case does not see '{DEFECTS[defect]}'"


# ---------------------------------------------------------------------------------------------- 4. conditions

def test_the_mean_of_v0_follows_the_bucket_variance():
    """buckets i.i.d. normal about a constant, sigma 0.05 in the left half and 0.5 in the right; K = 8, N = 8 K, 64 x 64, gain 0: the mean
    of v0 over a half is within 10 % of sigma^2 / K.  The relative standard deviation of s^2 with 7 degrees of freedom is
    sqrt(2 / 7) = 0.53; over 2048 pixels that is 1.2 %, so 10 % is more than eight standard errors: a condition, not a measurement."""
    K, side = 8, 64
    samples = rdi.normal_buckets(side, side, K, 8 * K, 2.0, 0.05, 0.5)
    planes, N = session_planes(samples, K)
    _, var = rdm.robust_denoise(planes, N, **dict(rdm.DEFAULTS, passes=0, demodulate=False, sigma_normal=0.0, sigma_position=0.0, gain=0.0))
    assert (var[..., 3] == K).all()
    for half, sigma in ((var[:, :side // 2, 1], 0.05), (var[:, side // 2:, 1], 0.5)):
        mean, want = float(half.astype(np.float64).mean()), sigma * sigma / K
        print(f"sigma {sigma}: mean v0 {mean:.6g}, sigma^2 / K {want:.6g}, ratio {mean / want:.4f}")
        assert abs(mean / want - 1) < 0.10


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def test_a_fine_checker_under_little_noise_is_kept():
    """a flat grey 0.5 with a one-pixel checker of +-0.02, bucket noise such that the standard deviation of the mean is 0.002, constant
    guides, K = 8, N = 32.  The bucket variance is about 4e-6: (sigma_lum sigma_lum) v + 2^-20 is about 6.5e-5, the squared step between
    neighbours 1.6e-3, so x = dl dl il is about 25 and ew = 0: the checker's two colours never mix.  rtgl_denoise_guided's 7 x 7 estimate
    sees the checker itself as variance, about 4e-4: x is about 0.25, ew about 0.77, and the checker is blurred.  (The albedo is 0.5, so
    after demodulation every variance and every squared step is four times that; the ratios stay.)  The RMSE against the noiseless
    checker must be lower for the new call; both are printed, DESIGN.md 5.15 records the ratio."""
    K = 8
    samples, truth, alb, nrm, pos = rdi.checker_case(K=K)
    planes, N = session_planes(samples, K)
    shared = dict(sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05, demodulate=True)
    new, var = rdm.robust_denoise(planes, N, alb, nrm, pos, passes=5, gain=1.0, **shared)
    resolved = rm.image_plane(planes, N, 1.0)
    old, old_var = gm.denoise_guided(resolved, alb, nrm, pos, passes=5, firefly_ratio=0.0, **shared)
    e_resolve, e_old, e_new = rmse(resolved, truth), rmse(old, truth), rmse(new, truth)
    print(f"checker: RMSE resolve {e_resolve:.6f}, resolve + denoise_guided {e_old:.6f}, robust_denoise {e_new:.6f}, ratio old / new {e_old / e_new:.2f}; "
          f"median v0 {float(np.median(var[..., 1])):.3g} against the spatial estimate {float(np.median(old_var[..., 1])):.3g}")
    assert e_new < e_old


# ---------------------------------------------------------------------------------------------- 5. refusals

def test_every_refusal():
    ok = dict(session=True, N=8, K=8, tiled=False, needed=7, enabled=7, restarted=False, frames_in_planes=1)
    assert not rdm.refused(**ok) and not rdm.refused(**dict(ok, N=9)) and not rdm.refused(**dict(ok, enabled=15))
    assert not rdm.refused(**dict(ok, needed=0, enabled=0, restarted=True, frames_in_planes=0))      # no plane needed: nothing to wait for
    for bad in (dict(session=False), dict(N=7), dict(N=0), dict(tiled=True), dict(enabled=3), dict(enabled=0), dict(needed=2, enabled=5),
                dict(restarted=True), dict(frames_in_planes=0)):
        assert rdm.refused(**dict(ok, **bad)), bad
    assert rdm.planes_needed(0.3, 0.05, True) == 7 and rdm.planes_needed(0.0, 0.05, True) == 5 and rdm.planes_needed(0.3, -1.0, False) == 2
    assert rdm.planes_needed(0.0, 0.0, False) == 0
    nan, inf = float("nan"), float("inf")
    good = dict(passes=5, sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05, gain=1.0)
    assert rdm.valid_params(**good) and rdm.valid_params(**dict(good, passes=0, sigma_normal=-1.0, sigma_position=0.0, gain=0.0, flags=0))
    for bad in (dict(passes=9), dict(sigma_lum=0.0), dict(sigma_lum=-1.0), dict(sigma_lum=nan), dict(sigma_lum=1e39), dict(sigma_normal=nan), dict(sigma_position=inf),
                dict(gain=nan), dict(gain=-1.0), dict(gain=1e39), dict(flags=2), dict(reserved=(0, 1))):
        assert not rdm.valid_params(**dict(good, **bad)), bad
        if "flags" not in bad and "reserved" not in bad:
            with pytest.raises(ValueError):
                rdm.robust_denoise(np.zeros((4, 2, 2, 4), f32), 4, passes=bad.get("passes", 0),
                                   **{k: v for k, v in dict(good, demodulate=False, **bad).items() if k != "passes"})
