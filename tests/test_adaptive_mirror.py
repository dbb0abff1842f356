"""tests/adaptive_mirror.py against a scalar restatement written from the header (include/rtgl_amd.h, "adaptive sampling"), on every size
at which the shapes take another path and with the special values; the rules for n == m, m == 0, the cap and a tile exactly on the
threshold; a fully masked session against the oracle's ordinary accumulation, bit for bit; and the two oracle loops of DESIGN.md 5.11,
whose error figures are printed, not asserted.  No GPU."""
import os

import numpy as np
import pytest

import adaptive_mirror as am
import golden_cases as gc

f32 = np.float32
SIZES = [(1, 1), (8, 8), (16, 16), (24, 40), (70, 53), (64, 64)]          # (width, height)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the scalar restatement ---------------------------------------------------------------------------------------------------------------
def s_lum(p):
    return (f32(0.25) * f32(p[0]) + f32(0.5) * f32(p[1])) + f32(0.25) * f32(p[2])


def s_tree(v):
    v = [f32(x) for x in v]
    while len(v) > 1:
        v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
    return v[0]


def s_shape(h, w):
    return (h + 15) // 16, (w + 15) // 16, h // 8 * 8, w // 8 * 8


def s_tile_pixels(h, w, t):
    ty, tx, fh, fw = s_shape(h, w)
    x0, y0 = (t % tx) * 16, (t // tx) * 16
    return sum(1 for y in range(y0, y0 + 16) for x in range(x0, x0 + 16) if x < fw and y < fh)


def s_blocks(h, w, mask):
    ty, tx, fh, fw = s_shape(h, w)
    return [by * (fw // 8) + bx for by in range(fh // 8) for bx in range(fw // 8) if mask[(by // 2) * tx + bx // 2]]


def s_merge(image, sample, n, mask):
    h, w = image.shape[:2]
    ty, tx, fh, fw = s_shape(h, w)
    image, n = image.copy(), list(n)
    with np.errstate(all="ignore"):
        for t in range(ty * tx):
            if not mask[t]:
                continue
            k = n[t]
            for y in range((t // tx) * 16, (t // tx) * 16 + 16):
                for x in range((t % tx) * 16, (t % tx) * 16 + 16):
                    if x < fw and y < fh:
                        for ch in range(3):
                            image[y, x, ch] = (sample[y, x, ch] + image[y, x, ch] * f32(k)) / f32(k + 1)
                        image[y, x, 3] = f32(1.0)
            n[t] = k + 1
    return image, n


def s_update(image, snapshot, n, m, records, threshold, floor):
    h, w = image.shape[:2]
    ty, tx, fh, fw = s_shape(h, w)
    snapshot, m, records = snapshot.copy(), list(m), [tuple(r) for r in records]
    threshold, floor = f32(threshold), f32(floor)
    with np.errstate(all="ignore"):
        for t in range(ty * tx):
            if not n[t] > m[t]:
                continue
            leaves, count = [], 0
            for i in range(256):
                x, y = (t % tx) * 16 + (i & 15), (t // tx) * 16 + (i >> 4)
                e = f32(0.0)
                if x < fw and y < fh:
                    Ln = s_lum(image[y, x])
                    if m[t] >= 1:
                        Lm = snapshot[y, x]
                        d = Ln - Lm
                        den = (Ln if Ln > 0 else f32(0.0)) + floor
                        q = d / den
                        qq = q * q
                        if qq - qq == 0:
                            e, count = qq, count + 1
                    snapshot[y, x] = Ln
                leaves.append(e)
            if count:
                total = s_tree(leaves)
                mse = (total / f32(count)) * (f32(m[t]) / f32(n[t] - m[t]))
                records[t] = (total, mse, count, int(mse <= threshold * threshold), n[t], n[t])
            else:
                records[t] = (f32(0.0), f32(0.0), 0, 0, n[t], n[t])
            m[t] = n[t]
    return snapshot, m, records


def s_rule(h, w, records, min_samples, max_samples):
    out = []
    for t, r in enumerate(records):
        n, fin = r[4], r[2] > 0 and r[3] != 0
        out.append(int(s_tile_pixels(h, w, t) > 0 and (n < min_samples or (n < max_samples and not fin))))
    return out


def s_summary(h, w, records, mask, max_samples):
    tiles = [t for t in range(len(records)) if s_tile_pixels(h, w, t) > 0]
    fin = lambda r: r[2] > 0 and r[3] != 0
    mses = [records[t][1] for t in tiles if records[t][2] > 0]
    return dict(tiles_total=len(tiles), tiles_active=sum(mask[t] for t in tiles), tiles_converged=sum(fin(records[t]) for t in tiles),
                tiles_capped=sum((not fin(records[t])) and records[t][4] >= max_samples for t in tiles), blocks_active=len(s_blocks(h, w, mask)),
                samples_min=min((records[t][4] for t in tiles), default=0), samples_max=max((records[t][4] for t in tiles), default=0),
                converged=int(not any(mask[t] for t in tiles)), samples_total=sum(records[t][4] * s_tile_pixels(h, w, t) for t in tiles),
                max_tile_mse=max(mses) if mses else f32(0.0))


def records_as_tuples(records):
    return [(r["sum"], r["mse"], int(r["count"]), int(r["converged"]), int(r["samples"]), int(r["samples_snapshot"])) for r in records.ravel()]


def same_records(mirror, scalar):
    for a, b in zip(records_as_tuples(mirror), scalar):
        if bits(a[0]) != bits(b[0]) or bits(a[1]) != bits(b[1]) or a[2:] != tuple(b[2:]):
            return False
    return True


def special_image(rng, h, w):
    """positive radiance with NaN, +-inf, negatives, zeros and values whose squares overflow scattered over it"""
    img = rng.random((h, w, 4), np.float32) * f32(2.0)
    flat = img.reshape(-1, 4)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -1.5, 0.0, -0.0, 3.0e38, -3.0e38, 1.0e-40, 2.0e19, 1.0e30)):
        idx = rng.integers(0, len(flat), 1 + len(flat) // 97)
        flat[idx, k % 3] = v
    return img


# ---- mirror == scalar -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_mirror_equals_the_scalar_restatement(size):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    s = am.shape(h, w)
    nt = s["ty"] * s["tx"]
    assert [s_tile_pixels(h, w, t) for t in range(nt)] == list(am.tile_pixels(h, w).ravel())
    sess = am.Session(h, w, threshold=0.3, floor=0.01, min_samples=2, max_samples=6)
    assert list(sess.mask.ravel()) == [int(s_tile_pixels(h, w, t) > 0) for t in range(nt)]
    if (w, h) == (1, 1):
        assert not sess.mask.any() and len(sess.blocks()) == 0
    image, snapshot, n, m = sess.image.copy(), sess.snapshot.copy(), [0] * nt, [0] * nt
    records = [(f32(0), f32(0), 0, 0, 0, 0)] * nt
    for step in range(9):
        if step in (3, 6):                                   # an explicit mask: every other tile, then the complement
            tiles = (np.arange(nt) + step) % 2
            sess.set_mask(tiles)
            assert list(sess.mask.ravel()) == [int(tiles[t] and s_tile_pixels(h, w, t) > 0) for t in range(nt)]
        mask = list(sess.mask.ravel())
        assert list(sess.blocks()) == s_blocks(h, w, mask)
        assert list(am.tile_list(sess.mask)) == [t for t in range(nt) if mask[t]]
        xs, ys = am.slot_pixels(h, w, sess.blocks())
        on = np.zeros((h, w), int)
        np.add.at(on, (ys, xs), 1)
        assert (on == am.active_pixels(h, w, sess.mask)).all()     # every active pixel is exactly one slot of queue 0
        sample = special_image(rng, h, w) if step % 2 else rng.random((h, w, 4), np.float32)
        sess.frame(sample)
        image, n = s_merge(image, sample, n, mask)
        assert (bits(sess.image) == bits(image)).all() and list(sess.n.ravel()) == n
        if step % 2:
            got = sess.update()
            snapshot, m, records = s_update(image, snapshot, n, m, records, 0.3, 0.01)
            assert (bits(sess.snapshot) == bits(snapshot)).all() and list(sess.m.ravel()) == m
            assert same_records(sess.records, records)
            assert list(sess.mask.ravel()) == s_rule(h, w, records, 2, 6)
            assert am.same_summary(got, s_summary(h, w, records, list(sess.mask.ravel()), 6)) == []
            assert not np.isnan(sess.records["sum"]).any() and not np.isnan(sess.records["mse"]).any()


def test_a_sum_that_overflows_is_defined_and_not_converged():
    sess = am.Session(16, 16, threshold=0.05, floor=0.01, min_samples=1, max_samples=100)
    sess.frame(np.full((16, 16, 4), 1.0, np.float32))
    sess.update()
    sess.frame(np.full((16, 16, 4), 1.0, np.float32))
    sess.snapshot[:] = f32(-1.0e17)                           # q = 1e17 / 0.01 = 1e19 and q q = 1e38 are finite; 256 of them are not
    sess.image[..., :3] = f32(1.0e-30)
    got = sess.update()
    r = sess.records[0, 0]
    assert r["count"] == 256 and np.isposinf(r["sum"]) and np.isposinf(r["mse"]) and r["converged"] == 0
    assert np.isposinf(got["max_tile_mse"]) and sess.mask[0, 0] == 1


def test_untouched_tiles_keep_record_and_snapshot_and_the_first_update_only_takes_the_snapshot():
    rng = np.random.default_rng(3)
    sess = am.Session(32, 32, min_samples=1, max_samples=50)
    sess.frame(rng.random((32, 32, 4), np.float32))
    got = sess.update()                                       # m == 0 everywhere
    assert (sess.records["count"] == 0).all() and (sess.records["samples"] == 1).all() and (sess.records["samples_snapshot"] == 1).all()
    assert got["tiles_converged"] == 0 and got["tiles_active"] == 4 and (sess.m == 1).all()
    sess.set_mask([[1, 0], [0, 0]])
    sess.frame(rng.random((32, 32, 4), np.float32))
    before_s, before_r = sess.snapshot.copy(), sess.records.copy()
    sess.update()
    assert sess.records[0, 0]["count"] == 256 and sess.records[0, 0]["samples"] == 2
    assert (sess.records.ravel()[1:] == before_r.ravel()[1:]).all()                       # n == m: kept
    assert (bits(sess.snapshot[16:, :]) == bits(before_s[16:, :])).all() and (bits(sess.snapshot[:16, 16:]) == bits(before_s[:16, 16:])).all()
    sess.update()                                             # nothing moved: everything kept
    assert sess.records[0, 0]["count"] == 256


def test_the_cap_and_the_minimum():
    r = np.zeros((1, 3), am.TILE_DTYPE)
    r["samples"] = [[3, 8, 8]]
    r["count"], r["converged"] = [[256, 256, 256]], [[1, 0, 1]]
    # below the minimum a converged tile stays active; at the cap an unconverged one stops
    assert list(am.rule(16, 48, r, min_samples=4, max_samples=8).ravel()) == [1, 0, 0]
    assert list(am.rule(16, 48, r, min_samples=1, max_samples=9).ravel()) == [0, 1, 0]
    r["count"] = 0                                            # converged without a count is not valid
    assert list(am.rule(16, 48, r, min_samples=1, max_samples=9).ravel()) == [1, 1, 1]
    s = am.summary(16, 48, r, am.rule(16, 48, r, 1, 8), max_samples=8)
    assert (s["tiles_capped"], s["tiles_converged"], s["tiles_active"], s["converged"]) == (2, 0, 1, 0)


def on_threshold_session(extra):
    """8 x 8, n = 2 m, den = 1: one pixel with q = 1/8 gives mse = 2^-12 = threshold^2 for threshold 1/64 exactly; `extra` adds a second
    pixel with q^2 = 1.125 ulp of 2^-6, which lifts the sum, and the mse, by exactly one ulp"""
    sess = am.Session(8, 8, threshold=1.0 / 64, floor=0.5, min_samples=1, max_samples=100)
    sess.n[:], sess.m[:] = 2, 1
    sess.image[...] = f32(0.5)
    sess.snapshot[:] = f32(0.5)
    sess.snapshot[0, 0] = f32(0.375)
    if extra:
        sess.snapshot[3, 5] = f32(0.5) - f32(0.75 * 2.0 ** -14)
    sess.update()
    return sess.records[0, 0]


def test_a_tile_on_the_threshold_is_converged_and_one_ulp_above_is_not():
    on, above = on_threshold_session(False), on_threshold_session(True)
    assert on["count"] == 64 and bits(on["mse"]) == bits(f32(2.0 ** -12)) and on["converged"] == 1
    assert bits(above["mse"]) == bits(np.nextafter(f32(2.0 ** -12), f32(1.0))) and above["converged"] == 0


# ---- against the oracle ------------------------------------------------------------------------------------------------------------------------
def oracle_sample(oracle, scene, p, size):
    img = np.zeros((size, size, 4), np.float32)
    oracle.render(scene, p.replace(frames=0, reset_flag=1), img, threads=min(16, os.cpu_count() or 1))
    return img


def test_a_full_mask_equals_the_oracles_ordinary_accumulation(rt, oracle):
    sc = rt.scenes
    scene, base, size, K = sc.scene_c1(False), sc.params_c1(), 24, 6
    sess, img = am.Session(size, size), np.zeros((size, size, 4), np.float32)
    for k, p in enumerate(gc.frame_sequence(sc, base, K)):
        sess.frame(oracle_sample(oracle, scene, p, size))
        oracle.render(scene, p.replace(frames=k, reset_flag=0), img, threads=min(16, os.cpu_count() or 1))
        assert (bits(sess.image) == bits(img)).all(), k
    assert (sess.n == K).all()


def adaptive_loop(rt, oracle, scene, base, min_samples, max_samples, size=64, check_every=16, limit=64):
    sc = rt.scenes
    sess = am.Session(size, size, threshold=0.05, floor=0.01, min_samples=min_samples, max_samples=max_samples)
    g, frames, summary = sc.GlibcRand(0), 0, None
    for _ in range(limit):
        for _ in range(check_every):
            sess.frame(oracle_sample(oracle, scene, base.replace(random=g.rand()), size))
            frames += 1
        summary = sess.update()
        if summary["converged"]:
            break
    return sess, frames, summary


def relative_mse(image, truth, floor=0.01):
    L, T = am.lum(image).astype(np.float64), am.lum(truth).astype(np.float64)
    return float(np.mean(((L - T) / (np.maximum(T, 0.0) + floor)) ** 2))


def check_loop_ended(sess, summary, max_samples):
    assert summary["converged"] == 1 and not sess.mask.any()
    fin = am.done(sess.records)
    assert (fin | (sess.records["samples"] >= max_samples)).all()
    assert summary["tiles_converged"] + summary["tiles_capped"] == summary["tiles_total"] == 16
    assert summary["samples_min"] < summary["samples_max"]                                 # the counts differ between tiles


def test_the_oracle_loop_on_the_sphere_scene(rt, oracle):
    """scene_c1(False), params_c1(), 64 x 64, GlibcRand(0), floor 0.01, threshold 0.05, min 16, max 512, an update every 16 frames.  The
    error figures are printed for DESIGN.md 5.11, not asserted."""
    sc = rt.scenes
    scene, base = sc.scene_c1(False), sc.params_c1()
    sess, frames, summary = adaptive_loop(rt, oracle, scene, base, 16, 512)
    check_loop_ended(sess, summary, 512)
    spp = summary["samples_total"] / (64 * 64)
    print(f"scene_c1(False): stopped after {frames} frames, per-tile samples {summary['samples_min']} .. {summary['samples_max']}, "
          f"{summary['samples_total']} samples = {spp:.1f} spp, {summary['tiles_capped']} tiles at the cap")
    assert spp < 64
    truth, uniform, g = np.zeros((64, 64, 4), np.float32), {}, sc.GlibcRand(0)
    for k in range(1024):
        oracle.render(scene, base.replace(frames=k, reset_flag=0, random=g.rand()), truth, threads=min(16, os.cpu_count() or 1))
        if k + 1 in (32, 64, 128):
            uniform[k + 1] = truth.copy()
    print(f"  relative MSE against 1024 frames: adaptive {relative_mse(sess.image, truth):.3g}; uniform " +
          ", ".join(f"{k} spp {relative_mse(v, truth):.3g}" for k, v in uniform.items()))
    L, T = am.lum(sess.image).astype(np.float64), am.lum(truth).astype(np.float64)
    per_tile = (((L - T) / (np.maximum(T, 0.0) + 0.01)) ** 2).reshape(4, 16, 4, 16).mean((1, 3)) ** 0.5
    print(f"  largest actual relative RMSE of a tile: {per_tile.max():.3g}")


def test_the_oracle_loop_on_the_mesh_scene(rt, oracle):
    """scene_mesh(10, 5, env_size=16), params_c2(), min 16, max 256: ends at the cap"""
    sc = rt.scenes
    sess, frames, summary = adaptive_loop(rt, oracle, sc.scene_mesh(10, 5, env_size=16), sc.params_c2(), 16, 256)
    check_loop_ended(sess, summary, 256)
    print(f"scene_mesh(10, 5, env_size=16): stopped after {frames} frames, per-tile samples {summary['samples_min']} .. {summary['samples_max']}, "
          f"{summary['samples_total'] / 4096:.1f} spp on average, {summary['tiles_capped']} tiles at the cap")
