"""The numpy restatement of rtgl_error_estimate (tests/error_mirror.py) without a GPU: against a scalar restatement written from the header
on every family x size; the estimator against the known variance of Gaussian frames and against the actual error of an oracle sequence;
and the snapshot rules over sequences of calls.  (The device is compared with the mirror in tests/test_gpu_error_estimate.py.)"""
import os

import numpy as np
import pytest

import error_inputs as ei
import error_mirror as em
import golden_cases as gc

f32 = np.float32


# ---- the scalar restatement: include/rtgl_amd.h, "error estimate", pixel by pixel ------------------------------------------------------
def tree_scalar(v):
    """the balanced tree by halving: for a power-of-two length the same additions as adjacent pairs first"""
    if len(v) == 1:
        return v[0]
    return tree_scalar(v[:len(v) // 2]) + tree_scalar(v[len(v) // 2:])


def scalar_estimate(image, snapshot, F_n, F_m, threshold, floor, quantile_permille, first_frames):
    h, w = image.shape[:2]
    fw, fh = w // 8 * 8, h // 8 * 8
    tx, ty = (w + 15) // 16, (h + 15) // 16
    n, m = F_n + 1 - first_frames, F_m + 1 - first_frames
    g_n, g_m, c = f32(float(F_n + 1) / float(n)), f32(float(F_m + 1) / float(m)), f32(float(m) / float(n - m))
    threshold, floor, zero = f32(threshold), f32(floor), f32(0.0)
    img, snap = image.tolist(), snapshot.tolist()                       # (Python floats: exact images of the binary32 values)
    tiles = np.zeros((ty, tx), em.TILE_DTYPE)
    sums, counted = [], 0
    for j in range(ty):
        for i in range(tx):
            leaves, count = [zero] * 256, 0
            for r in range(16):
                y = 16 * j + r
                if y >= fh:
                    continue
                for col in range(16):
                    x = 16 * i + col
                    if x >= fw:
                        continue
                    R, G, B = f32(img[y][x][0]), f32(img[y][x][1]), f32(img[y][x][2])
                    Ln = ((f32(0.25) * R + f32(0.5) * G) + f32(0.25) * B) * g_n
                    Lm = f32(snap[y][x]) * g_m
                    d = Ln - Lm
                    den = (Ln if Ln > 0 else zero) + floor
                    q = d / den
                    e = q * q
                    if e - e == 0:
                        leaves[16 * r + col] = e
                        count += 1
            s = tree_scalar(leaves)
            if count:
                mse = (s / f32(count)) * c
                tiles[j, i] = (s, mse, count, int(mse <= threshold * threshold))
            sums.append(tiles[j, i]["sum"])
            counted += count
    lanes = [zero] * 256
    for k, s in enumerate(sums):
        lanes[k % 256] = lanes[k % 256] + s
    total = tree_scalar(lanes)
    valid = tiles["count"] > 0
    tv, tc = int(valid.sum()), int(tiles["converged"].sum())
    return dict(valid=1, converged=int(tv > 0 and tc * 1000 >= tv * quantile_permille), frames_now=F_n, frames_snapshot=F_m, tiles_valid=tv,
                tiles_converged=tc, pixels_ignored=fw * fh - counted, scale=c, mse=(total / f32(counted)) * c if counted else zero,
                max_tile_mse=max([zero] + [t["mse"] for t in tiles.ravel() if t["count"]]), tiles=tiles)


def scalar_run(steps):
    """the header's snapshot handling over a family's steps (families never drop the snapshot in between)"""
    out, snap, F_m, first = [], None, None, None
    for s in steps:
        p = dict(em.DEFAULTS)
        p.update(s["params"])
        keep = p.pop("keep_snapshot")
        usable = snap is not None and s["frames"] > F_m and p["first_frames"] == first
        out.append(scalar_estimate(s["image"], snap, s["frames"], F_m, **p) if usable else em.empty_result(*s["image"].shape[:2]))
        if not (usable and keep):
            snap, F_m, first = em.lum(s["image"]), s["frames"], p["first_frames"]
    return out


@pytest.mark.parametrize("size", ei.SIZES, ids=[f"{w}x{h}" for h, w in ei.SIZES])
def test_the_mirror_equals_the_scalar_restatement_on_every_family(size):
    h, w = size
    with np.errstate(all="ignore"):
        for name in ei.FAMILIES:
            steps = ei.family(name, h, w)
            got, want = ei.run(steps), scalar_run(steps)
            assert got[0]["valid"] == 0 and all(r["valid"] == 1 for r in got[1:]), name
            for k, (a, b) in enumerate(zip(got, want)):
                assert em.same_result(a, b) == [], f"{name} {w} x {h}, call {k}: {em.same_result(a, b)}"
                assert not any(np.isnan(f32(a[key])) for key in em.SUMMARY_FLOAT), f"{name}: a NaN in the summary"
                assert not np.isnan(a["tiles"]["sum"]).any() and not np.isnan(a["tiles"]["mse"]).any(), f"{name}: a NaN in a tile record"


def test_the_families_hold_what_their_names_say():
    h, w = 131, 200
    r = ei.run(ei.constant(h, w))
    assert all(x["mse"] == 0 and x["max_tile_mse"] == 0 and x["converged"] == 1 and x["pixels_ignored"] == 0 for x in r[1:])
    r = ei.run(ei.black(h, w))[1]
    assert r["mse"] == 0 and r["converged"] == 1 and r["tiles_valid"] == 8 * 13                # (131 rows: the footprint ends at 128)
    r = ei.run(ei.one_noisy_tile(h, w))
    assert r[1]["tiles_converged"] == r[1]["tiles_valid"] - 1 and r[1]["converged"] == 1 and r[2]["converged"] == 0
    assert em.same_result(dict(r[1], converged=0), r[2]) == []          # (the keep flag: the same estimate, another permille)
    assert r[3]["converged"] == 0 and r[3]["frames_snapshot"] == 15
    r = ei.run(ei.threshold_edge(h, w))[1]
    t = r["tiles"]
    assert t["mse"][0, 0] == f32(0.25) and t["converged"][0, 0] == 1
    assert t["mse"][0, 1] == np.nextafter(f32(0.25), f32(1.0)) and t["converged"][0, 1] == 0
    assert t["sum"][0, 1] == f32(64.0) + f32(2.0 ** -17) and r["converged"] == 0 and r["scale"] == 1
    with np.errstate(all="ignore"):
        r = ei.run(ei.overflow(h, w))[1]
        assert np.isinf(r["mse"]) and np.isinf(r["max_tile_mse"]) and r["converged"] == 0 and r["pixels_ignored"] == 0
        assert np.isinf(r["tiles"]["sum"][0]).all() and np.isfinite(r["tiles"]["sum"][-1]).all()
        r = ei.run(ei.nan_tile(h, w))[1]
        assert r["tiles"][0, 0].tolist() == (0.0, 0.0, 0, 0) and r["pixels_ignored"] == 256 and r["tiles_valid"] == 8 * 13 - 1
        r = ei.run(ei.nan_tile(16, 16))[1]                              # nothing counts anywhere: valid, empty, not converged
        assert (r["valid"], r["tiles_valid"], r["converged"], float(r["mse"]), float(r["max_tile_mse"])) == (1, 0, 0, 0.0, 0.0)
        r = ei.run(ei.specials(h, w))
        assert all(x["pixels_ignored"] > 0 and x["tiles_valid"] > 0 for x in r[1:])
    r = ei.run(ei.gauss1(5, 7))[1]                                      # an empty footprint
    assert (r["valid"], r["tiles_valid"], r["pixels_ignored"], r["converged"]) == (1, 0, 0, 0) and r["tiles"].shape == (1, 1)


@pytest.mark.parametrize("first_frames", [0, 1])
@pytest.mark.parametrize("pair", [(16, 32), (48, 64)])
def test_gaussian_frames_of_known_sigma(pair, first_frames):
    """64 x 64, mu 1, sigma 0.3: the whole picture's mse over (sigma^2 / n) / (mu + floor)^2 within [0.9, 1.1].  4,096 degrees of freedom
    give the ratio a standard deviation of 2.2 %: the bracket is 4.5 sigma (200 seeds stayed within 0.92 .. 1.08)."""
    mu, sigma, floor = 1.0, 0.3, 0.01
    steps = ei.gaussian_steps(64, 64, pair, first_frames, mu=mu, sigma=sigma, seed=1234)
    r = ei.run(steps)[1]
    ratio = float(r["mse"]) / ((sigma ** 2 / pair[1]) / (mu + floor) ** 2)
    print(f"gaussian {pair[0]} -> {pair[1]}, first_frames {first_frames}: estimated / true = {ratio:.4f}")
    assert r["valid"] == 1 and r["pixels_ignored"] == 0 and 0.9 <= ratio <= 1.1


# ---- an oracle sequence: the estimate against the error that is actually there ----------------------------------------------------------
def oracle_images(rt, oracle, scene, base, moments, size=64):
    """the accumulation image after the frames 1 .. max(moments) of the reference's loop, copies at `moments`"""
    sc = rt.scenes
    img, out = np.zeros((size, size, 4), np.float32), {}
    for p in gc.frame_sequence(sc, base, max(moments)):
        oracle.render(scene, p, img, threads=min(16, os.cpu_count() or 1))
        if p.frames in moments:
            out[p.frames] = img.copy()
    return out


def estimated_over_actual(images, m, n, last, floor=0.01):
    """The mirror's whole-picture mse from the moments m -> n (frames counted from 1) over the actual relative MSE of moment n against
    moment `last`: both unbiased, the same denominator, in float64."""
    est = em.Estimator()
    est.frame(m)
    est(images[m], floor=floor)
    est.frame(n)
    r = est(images[n], floor=floor)
    unbiased = lambda F: em.lum(images[F]).astype(np.float64) * ((F + 1.0) / F)
    Ln, Lt = unbiased(n), unbiased(last)
    actual = np.mean(((Ln - Lt) / (np.maximum(Ln, 0.0) + floor)) ** 2)
    return float(r["mse"]) / actual, r


@pytest.fixture(scope="module")
def c1_images(rt, oracle):
    sc = rt.scenes
    return oracle_images(rt, oracle, sc.scene_c1(False), sc.params_c1(), (16, 32, 48, 64, 128, 1024))


def test_the_estimate_meets_the_actual_error_of_an_oracle_sequence(c1_images):
    """scene_c1(False), params_c1(), 64 x 64, frames 1 .. 1024: the estimate 32 -> 64 over the actual relative MSE of frame 64 against
    frame 1,024 within [0.8, 1.25] (float64 restatement: 1.015; neighbouring pairs 0.96 .. 1.15)."""
    for m, n in ((16, 32), (48, 64), (64, 128)):
        print(f"scene_c1(False) {m} -> {n}: estimated / actual = {estimated_over_actual(c1_images, m, n, 1024)[0]:.4f}")
    ratio, r = estimated_over_actual(c1_images, 32, 64, 1024)
    print(f"scene_c1(False) 32 -> 64: estimated / actual = {ratio:.4f}  (mse {float(r['mse']):.6g}, {r['tiles_converged']} / {r['tiles_valid']} tiles converged)")
    assert r["valid"] == 1 and 0.8 <= ratio <= 1.25


def test_firefly_ridden_scenes_are_printed_not_asserted(rt, oracle):
    """the lit sphere scene and the mesh scene under-estimate (Limits): radiance not yet seen cannot be estimated"""
    sc = rt.scenes
    for label, scene, base in (("scene_c1(True)", sc.scene_c1(True), sc.params_c1()), ("scene_mesh(10, 5, env_size=16)", sc.scene_mesh(10, 5, env_size=16), sc.params_c2())):
        ratio, r = estimated_over_actual(oracle_images(rt, oracle, scene, base, (32, 64, 1024)), 32, 64, 1024)
        print(f"{label} 32 -> 64: estimated / actual = {ratio:.4f}")
        assert r["valid"] == 1 and np.isfinite(ratio)


# ---- the snapshot rules ------------------------------------------------------------------------------------------------------------------
def means(n_list, seed=5):
    return dict(zip(n_list, (s["image"] for s in ei.gaussian_steps(24, 24, n_list, 1, seed=seed))))


def test_snapshot_rules_over_a_sequence():
    img = means((8, 16, 24, 32, 40))
    est = em.Estimator()
    est.frame(8)
    first = est(img[8])
    assert first["valid"] == 0 and em.same_result(first, em.empty_result(24, 24)) == [] and est.has_snapshot() and est.fm == 8
    est.frame(16)
    r = est(img[16])
    assert (r["valid"], r["frames_now"], r["frames_snapshot"]) == (1, 16, 8) and est.fm == 16       # the snapshot moved on
    # the keep flag: the snapshot of frame 16 stays, two later calls measure against it
    est.frame(24)
    k1 = est(img[24], keep_snapshot=True)
    est.frame(32)
    k2 = est(img[32], keep_snapshot=True)
    assert (k1["frames_snapshot"], k2["frames_snapshot"], est.fm) == (16, 16, 16) and k2["scale"] == f32(16.0 / 16.0)
    assert em.same_result(k2, em.estimate(img[32], em.lum(img[16]), 32, 16)) == []
    # the keep flag without a snapshot takes one
    fresh = em.Estimator()
    fresh.frame(8)
    assert fresh(img[8], keep_snapshot=True)["valid"] == 0 and fresh.has_snapshot()
    # every dropping event: the next call is a first call again
    for event in ("drop", "reset_frame"):
        est.frame(40)
        assert est(img[40])["valid"] == 1
        if event == "drop":                                             # rtgl_error_reset, rtgl_clear_image, rtgl_write_image_f32, rtgl_bind_device_image
            est.drop()
            est.frame(41)
        else:                                                           # a rendered frame with reset_flag != 0
            est.frame(41, reset_flag=1)
        assert not est.has_snapshot()
        r = est(img[40])
        assert r["valid"] == 0 and est.has_snapshot() and est.fm == 41
        est.frame(32)                                                   # (so that the loop's next call at 40 is a later moment)
        est(img[32])


def test_a_call_that_is_not_later_or_counts_differently_takes_a_new_snapshot():
    img = means((8, 16, 24))
    est = em.Estimator()
    est.frame(16)
    est(img[16])
    assert est(img[16])["valid"] == 0 and est.fm == 16                  # F_n == F_m
    est.frame(8)
    assert est(img[8])["valid"] == 0 and est.fm == 8                    # F_n < F_m: the snapshot is now frame 8's
    est.frame(16)
    assert est(img[16], first_frames=0)["valid"] == 0 and est.first == 0    # another first_frames
    est.frame(24)
    r = est(img[24], first_frames=0)
    assert r["valid"] == 1 and r["scale"] == f32(17.0 / 8.0)
    with pytest.raises(AssertionError):                                 # n < 1
        est.frame(0)
        est(img[8], first_frames=2)
