"""The reference of tests/test_gpu_robust_error.py, pinned without a GPU (include/rtgl_amd.h, "robust error estimate").

1. The numpy restatement (tests/robust_error_mirror.py) and a scalar restatement written from the header, pixel by pixel and tile by tile,
   agree in every bit on the families of tests/robust_error_inputs.py, and what a family states about its result holds.
2. Teeth.  The scalar restatement takes at most one of DEFECTS, each a way the kernel could plausibly be wrong; every defect changes
   result bits on named cases that the GPU module runs.
3. The oracle table of DESIGN.md 5.13 and the stop rule, regenerated through the mirror, printed and asserted."""
import math
import os

import numpy as np
import pytest

import error_mirror as em
import robust_error_inputs as rei
import robust_error_mirror as rem
import robust_mirror as rm

f32 = np.float32

# ---------------------------------------------------------------------------------------------- 1. the scalar restatement

DEFECTS = {
    "lo_hi_swapped": "lo is the key of rank K - 1 - t and hi the key of rank t",
    "divide_by_K": "v = D / (K (K - 1)) instead of D / (h (h - 1))",
    "rank_order": "D is summed in rank order instead of bucket order",
    "mw_of_kept": "mw is the mean of the w_j of the kept buckets only",
    "floor_inside": "e = v / (mu mu + floor): the floor inside the square",
    "count_ignored": "count includes the footprint pixels that do not count",
}


def pixel(b, K, gain, floor, defect=None):
    """steps 1-9 of the header for one pixel; b: K buckets of 4 float32.  Returns (e, counts)."""
    inf = f32(np.inf)
    key = []
    for j in range(K):
        l = (f32(0.25) * b[j][0] + f32(0.5) * b[j][1]) + f32(0.25) * b[j][2]
        key.append(l if math.isfinite(l) else inf)
    kf = [float(v) for v in key]                                   # (comparisons of binary32 values are the same in binary64)
    rank = [sum(1 for i in range(K) if i != j and (kf[i] < kf[j] or (kf[i] == kf[j] and i < j))) for j in range(K)]
    S, A = f32(0), f32(0)
    for j in range(K):
        S = S + key[j]
        A = A + f32(2 * rank[j] - (K - 1)) * key[j]
    if not math.isfinite(S):
        G = f32(1)
    elif not S > 0:
        G = f32(0)
    else:
        G = A / (f32(K) * S)
    if not G <= 1:
        G = f32(1)
    if not G >= 0:
        G = f32(0)
    u = (G * f32(gain)) * f32(K // 2)
    cap = (K - 1) // 2
    t = cap if u >= f32(cap) else int(u)
    at = {rank[j]: j for j in range(K)}
    lo, hi = key[at[t]], key[at[K - 1 - t]]
    if defect == "lo_hi_swapped":
        lo, hi = hi, lo
    w = [min(max(key[j], lo), hi) for j in range(K)]
    kept = [j for j in range(K) if t <= rank[j] <= K - 1 - t]
    h = K - 2 * t
    assert len(kept) == h >= 2
    M = f32(0)
    for j in (kept if defect == "mw_of_kept" else range(K)):
        M = M + w[j]
    mw = M / f32(h if defect == "mw_of_kept" else K)
    D = f32(0)
    for j in (range(K) if defect != "rank_order" else [at[r] for r in range(K)]):
        D = D + (w[j] - mw) * (w[j] - mw)
    T = f32(0)
    for j in kept:
        T = T + key[j]
    mu = T / f32(h)
    v = D / f32(K * (K - 1) if defect == "divide_by_K" else h * (h - 1))
    if defect == "floor_inside":
        pos = mu if mu > 0 else f32(0)
        e = v / (pos * pos + f32(floor))
    else:
        den = (mu if mu > 0 else f32(0)) + f32(floor)
        e = v / (den * den)
    return e, bool(e - e == 0)


def tree256(values):
    """the balanced pairwise tree over 256 leaves, by recursion"""
    def go(lo, n):
        return values[lo] if n == 1 else go(lo, n // 2) + go(lo + n // 2, n // 2)
    return go(0, 256)


def restate(planes, N, threshold=0.05, floor=0.01, gain=1.0, quantile_permille=950, defect=None):
    """the whole estimate by scalars, laid out like the mirror's result"""
    K, h, w = planes.shape[:3]
    fh, fw = h // 8 * 8, w // 8 * 8
    ty, tx = (h + 15) // 16, (w + 15) // 16
    tiles = np.zeros((ty, tx), em.TILE_DTYPE)
    thr = f32(threshold)
    with np.errstate(all="ignore"):
        for Y in range(ty):
            for X in range(tx):
                leaves, count = [f32(0)] * 256, 0
                for i in range(256):
                    y, x = Y * 16 + i // 16, X * 16 + i % 16
                    if y < fh and x < fw:
                        e, counts = pixel([list(planes[j, y, x]) for j in range(K)], K, gain, floor, defect)
                        if counts:
                            leaves[i] = e
                        count += 1 if (counts or defect == "count_ignored") else 0
                if count:
                    s = tree256(leaves)
                    mse = s / f32(count)
                    tiles[Y, X] = (s, mse, count, 1 if mse <= thr * thr else 0)
        lanes = [f32(0)] * 256
        for i, s in enumerate(tiles["sum"].ravel()):
            lanes[i % 256] = lanes[i % 256] + s
        total, n = tree256(lanes), int(tiles["count"].sum(dtype=np.uint64))
        valid = tiles["count"] > 0
        out = dict(valid=1, frames_now=N, frames_snapshot=0, tiles_valid=int(valid.sum()), tiles_converged=int(tiles["converged"].sum()),
                   pixels_ignored=(fh * fw - n) & 0xFFFFFFFF, scale=f32(1), mse=(total / f32(n)) * f32(1) if n else f32(0),
                   max_tile_mse=max([f32(0)] + [m for m in tiles["mse"][valid]]), tiles=tiles)
    out["converged"] = int(out["tiles_valid"] > 0 and out["tiles_converged"] * 1000 >= out["tiles_valid"] * quantile_permille)
    return out


def session_planes(samples, K):
    h, w = samples[0].shape[:2]
    sess = rm.Session(h, w, K)
    for s in samples:
        sess.accumulate(s)
    return sess.planes, sess.N


@pytest.mark.parametrize("K", rei.BUCKETS)
@pytest.mark.parametrize("size", rei.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_mirror_equals_the_scalar_restatement(size, K):
    w, h = size
    for family in rei.FAMILIES:
        case = rei.make(family, h, w, K)
        planes, N = session_planes(case["samples"], K)
        for params in case["params"]:
            assert em.same_result(rem.estimate(planes, N, **params), restate(planes, N, **params)) == [], (family, size, K, params)


@pytest.mark.parametrize("K", rei.BUCKETS)
@pytest.mark.parametrize("size", rei.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_what_the_families_state_about_their_results(size, K):
    w, h = size
    fh, fw = h // 8 * 8, w // 8 * 8
    cap = rm.trim_cap(K)

    def run(family, which=0):
        case = rei.make(family, h, w, K)
        planes, N = session_planes(case["samples"], K)
        p = case["params"][which]
        return planes, N, p, rem.estimate(planes, N, **p), rem.pixel_error(planes, N, p.get("gain", 1.0), p.get("floor", 0.01))

    def zero_footprint(r):
        return r["valid"] == 1 and r["tiles_valid"] == 0 and r["converged"] == 0 and not r["tiles"].tobytes().strip(b"\0") and r["pixels_ignored"] == 0

    planes, N, p, r, (e, counts) = run("equal")                    # equal buckets: e = +0 exactly, every tile converged
    assert N == 2 * K and (e.view(np.uint32) == 0).all() and counts.all()
    if fh * fw:
        assert r["converged"] == 1 and r["tiles_converged"] == r["tiles_valid"] == ((fh + 15) // 16) * ((fw + 15) // 16) and r["mse"] == 0 and r["pixels_ignored"] == 0
        assert r["frames_now"] == N and r["frames_snapshot"] == 0 and r["scale"] == 1
    else:
        assert zero_footprint(r)
    planes, N, p, r, (e, counts) = run("outlier", 0)               # one bucket 2^20 times the others: winsorized to the rest at gain 1 ...
    assert (e.view(np.uint32) == 0).all() and counts.all() and (r["converged"] == 1 or not fh * fw)
    planes, N, p, r, (e, counts) = run("outlier", 1)               # ... and in full at gain 0: far above any threshold
    lit = rm.lum(planes[0][..., :3]) > 0
    assert (e[lit] > f32(0.05) * f32(0.05)).all() and counts.all()
    if fh * fw and lit[:fh, :fw].all():
        assert r["converged"] == 0 and r["tiles_converged"] == 0
    planes, N, p, r, (e, counts) = run("nonfinite")                # more non-finite buckets than the trim drops: the pixel is ignored
    bad = (~np.isfinite(planes[..., 0])).sum(0)
    assert not counts[bad > cap].any() and counts[bad <= cap].all()
    assert r["pixels_ignored"] == int((bad[:fh, :fw] > cap).sum())
    planes, N, p, r, (e, counts) = run("negative", 1)              # mu <= 0: den is the floor alone
    key, rank, G = rm.gini(planes)
    assert (key <= 0).all() and counts.all() and N == K + 1
    with np.errstate(all="ignore"):
        s2 = key.astype(np.float64).var(0, ddof=1) / K / 0.25      # (gain 0: the textbook s^2 / K over floor^2)
    assert np.allclose(e, s2, rtol=1e-4, atol=1e-12) and e[h // 2, w // 2] == 0
    for family, n in (("full", K), ("gain_zero", K + 1), ("ragged", 2 * K + 3)):
        planes, N, p, r, _ = run(family)
        assert N == n == r["frames_now"]
    planes, N, p, r, (e, counts) = run("edge")                     # a tile's mse exactly on threshold^2: converged; one ulp above: not
    t2 = f32(p["threshold"]) * f32(p["threshold"])
    assert (e.view(np.uint32) == t2.view(np.uint32)).all()
    planes, N, p, r2, _ = run("edge_above")
    if fh * fw:
        assert (r["tiles"]["mse"][r["tiles"]["count"] > 0].view(np.uint32) == t2.view(np.uint32)).all() and r["converged"] == 1
        full = r2["tiles"]["count"] == 256
        assert (r2["tiles"]["mse"][full].view(np.uint32) == t2.view(np.uint32) + 1).all() and not r2["tiles"]["converged"][full].any()
        assert (w, h) != (16, 16) or (full.all() and r2["converged"] == 0)
    else:
        assert zero_footprint(r) and zero_footprint(r2)


def test_validation_and_states():
    d = rem.DEFAULTS
    assert d == dict(threshold=0.05, floor=0.01, gain=1.0, quantile_permille=950) and rem.valid_params(**d)
    for bad in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=np.nan), dict(threshold=np.inf), dict(floor=0.0), dict(floor=np.nan), dict(floor=1e39),
                dict(gain=np.nan), dict(gain=-1.0), dict(gain=np.inf), dict(gain=1e39), dict(quantile_permille=0), dict(quantile_permille=1001),
                dict(flags=1), dict(reserved=(0, 0, 1))):
        assert not rem.valid_params(**{**d, **bad}), bad
    assert rem.valid_params(**{**d, "gain": 0.0}) and rem.valid_params(**{**d, "quantile_permille": 1}) and rem.valid_params(**{**d, "quantile_permille": 1000})
    for K in rei.BUCKETS:
        assert rem.refused(False, 4 * K, K) and rem.refused(True, K - 1, K) and rem.refused(True, 0, K) and not rem.refused(True, K, K)


# ---------------------------------------------------------------------------------------------- 2. teeth

S70, S17, S16, S24 = (70, 53), (17, 17), (16, 16), (24, 40)
CATCHERS = {
    "lo_hi_swapped": [("ragged", S17, 8), ("gain_huge", S24, 4), ("outlier", S16, 16)],
    "divide_by_K": [("ragged", S17, 8), ("edge", S16, 4), ("gain_huge", S70, 16)],
    "rank_order": [("ragged", S70, 8), ("full", S24, 16)],
    "mw_of_kept": [("ragged", S17, 8), ("full", S24, 16)],     # (not a full trim: with h = 2 the winsorized keys are half lo, half hi, and both means agree),
    "floor_inside": [("ragged", S17, 8), ("negative", S16, 4), ("edge", S24, 16)],
    "count_ignored": [("nonfinite", S17, 8), ("specials", S70, 4)],
}


def test_every_defect_has_catchers():
    assert set(CATCHERS) == set(DEFECTS)


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_defect_changes_bits_that_the_comparison_sees(defect):
    listed = rei.listed_cases()
    caught = 0
    for family, (w, h), K in CATCHERS[defect]:
        assert (family, (w, h), K) in listed, f"{family} {w} x {h} K = {K} is not a case of the GPU module"
        case = rei.make(family, h, w, K)
        planes, N = session_planes(case["samples"], K)
        changed = []
        for params in case["params"]:
            changed += em.same_result(rem.estimate(planes, N, **params), restate(planes, N, defect=defect, **params))
        print(f"{defect} ({DEFECTS[defect]}): {family} {w} x {h} K = {K}: {sorted(set(changed))} change")
        caught += bool(changed)
    assert caught == len(CATCHERS[defect]), f"a listed case does not see '{DEFECTS[defect]}'"


# ---------------------------------------------------------------------------------------------- 3. the oracle table and the stop rule

TABLE_N, TRUTH_FRAMES, SIZE, STOP_FRAMES, STOP_EVERY = (16, 32, 64, 128, 256), 1024, 64, 512, 8
ROWS = [("scene_c1(False)", 8, 1.0), ("scene_c1(True)", 8, 1.0), ("scene_mesh(10, 5, env_size=16)", 8, 1.0), ("scene_c1(True)", 8, 0.0), ("scene_c1(True)", 16, 1.0)]
STOPS = [("scene_c1(True)", 8, 1.0, 0.1), ("scene_c1(True)", 8, 0.0, 0.1), ("scene_c1(False)", 8, 1.0, 0.05), ("scene_c1(False)", 8, 0.0, 0.05),
         ("scene_mesh(10, 5, env_size=16)", 8, 1.0, 0.1)]


def relative_mse(image, truth, floor=0.01):
    """the mean over the picture of ((L - T) / (max(T, 0) + floor))^2 of the luminance"""
    L, T = rm.lum(image[..., :3]).astype(np.float64), rm.lum(truth[..., :3]).astype(np.float64)
    return float(np.mean(((L - T) / (np.maximum(T, 0.0) + floor)) ** 2))


@pytest.fixture(scope="module")
def table(rt, oracle):
    """tests/test_robust_mirror.py's set-up: 64 x 64, GlibcRand(0), every frame a one-sample image (frames = 0, reset_flag = 1), the truth
    the binary64 mean of 1,024 of them.  ratios[(scene, K, gain)][N] = the estimate's mse over the actual relative MSE of the resolved
    picture of the first N frames; stops[(scene, K, gain, threshold)] = (stop frame or None, actual relative RMSE there, tiles converged)
    for an estimate every 8 frames with the default floor and quantile."""
    sc = rt.scenes
    scenes = {"scene_c1(True)": (sc.scene_c1(True), sc.params_c1()), "scene_mesh(10, 5, env_size=16)": (sc.scene_mesh(10, 5, env_size=16), sc.params_c2()),
              "scene_c1(False)": (sc.scene_c1(False), sc.params_c1())}
    threads, ratios, stops = min(16, os.cpu_count() or 1), {}, {}
    for name, (scene, base) in scenes.items():
        g, total, img = sc.GlibcRand(0), np.zeros((SIZE, SIZE, 4), np.float64), np.zeros((SIZE, SIZE, 4), f32)
        sessions = {K: rm.Session(SIZE, SIZE, K) for K in sorted({K for s, K, _ in ROWS if s == name} | {K for s, K, _, _ in STOPS if s == name})}
        kept = {}                                                  # (K, N) -> the planes then
        for k in range(TRUTH_FRAMES):
            oracle.render(scene, base.replace(frames=0, reset_flag=1, random=g.rand()), img, threads=threads)
            total += img
            if k < STOP_FRAMES:
                for K, sess in sessions.items():
                    sess.accumulate(img)
                    if (k + 1) % STOP_EVERY == 0 or k + 1 in TABLE_N:
                        kept[(K, k + 1)] = sess.planes.copy()
        truth = total / TRUTH_FRAMES
        for s, K, gain in ROWS:
            if s == name:
                ratios[(s, K, gain)] = {N: float(rem.estimate(kept[(K, N)], N, gain=gain)["mse"]) / relative_mse(rm.resolve(kept[(K, N)], N, gain)[0], truth)
                                        for N in TABLE_N}
        for s, K, gain, threshold in STOPS:
            if s == name:
                stops[(s, K, gain, threshold)] = (None, None, None)
                for N in range(STOP_EVERY, STOP_FRAMES + 1, STOP_EVERY):
                    if N < K:
                        continue
                    r = rem.estimate(kept[(K, N)], N, threshold=threshold, gain=gain)
                    if r["converged"] or N == STOP_FRAMES:
                        stops[(s, K, gain, threshold)] = (N if r["converged"] else None, math.sqrt(relative_mse(rm.resolve(kept[(K, N)], N, gain)[0], truth)),
                                                          (r["tiles_converged"], r["tiles_valid"]))
                        break
    print(f"\nestimate over actual relative MSE of the resolved picture (truth: {TRUTH_FRAMES} frames)")
    for key, row in ratios.items():
        print(f"  {key[0]}, K = {key[1]}, gain {key[2]:g}: " + "; ".join(f"N = {N}: {v:.2f}" for N, v in row.items()))
    print(f"stop rule, an estimate every {STOP_EVERY} frames, 950 permille of the tiles, at most {STOP_FRAMES} frames")
    for key, (N, rmse, tiles) in stops.items():
        print(f"  {key[0]}, K = {key[1]}, gain {key[2]:g}, threshold {key[3]}: " + (f"stops after {N} frames" if N else "does not stop")
              + f", actual relative RMSE {rmse:.4f}, tiles converged {tiles[0]} of {tiles[1]}")
    return ratios, stops


def test_the_oracle_table(table):
    """the margins are over what the prototype measured; the low readings of the firefly scenes at N = 32 - 64 and the
    K = 16 row are printed, not asserted: they are limits"""
    ratios, stops = table
    for N in (32, 64, 128):                                        # the clean scene: measured 1.16 - 1.28 (the truth shares its first frames with the picture)
        assert 0.8 <= ratios[("scene_c1(False)", 8, 1.0)][N] <= 1.6, (N, ratios[("scene_c1(False)", 8, 1.0)])
    for name in ("scene_c1(True)", "scene_mesh(10, 5, env_size=16)"):      # the firefly scenes: measured 1.17 and 0.66
        assert 0.5 <= ratios[(name, 8, 1.0)][128] <= 2.0, (name, ratios[(name, 8, 1.0)])


def test_the_stop_rule(table):
    ratios, stops = table
    n1, rmse1, _ = stops[("scene_c1(True)", 8, 1.0, 0.1)]          # measured 40 frames at 0.083, the plain mean 456
    n0, rmse0, _ = stops[("scene_c1(True)", 8, 0.0, 0.1)]
    assert n1 is not None and n1 <= 64 and rmse1 <= 0.1, (n1, rmse1)
    assert n0 is None or 4 * n1 <= n0, (n1, n0)                    # (None: the plain mean needs more than 512)
    for gain in (1.0, 0.0):                                        # the clean scene: measured 128 frames at 0.017
        n, rmse, _ = stops[("scene_c1(False)", 8, gain, 0.05)]
        assert n is not None and n <= 256 and rmse < 0.05, (gain, n, rmse)
