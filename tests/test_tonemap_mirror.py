"""The numpy restatement of rtgl_tonemap (tests/tonemap_mirror.py) against a scalar restatement written straight from the header's
contract, the committed tables against their formulas, and the properties the design rests on: the encoder is the correctly rounded sRGB
code, a picture scaled by a power of two gets the reciprocal exposure and the same bytes, and the defaults keep the 30 x light of the
project's own scene from blowing the picture out.  No GPU."""
import bisect
import os
import re
import struct

import numpy as np
import pytest

import tonemap_inputs as ti
import tonemap_mirror as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "raytracer.glsl_amd", "csrc", "rt_tonemap.hpp")
F = np.float32


def committed_table(name, n):
    with open(KERNELS) as f:
        text = f.read()
    body = re.search(r"const\s+float\s+" + name + r"\[(\d+)\]\s*=\s*\{(.*?)\};", text, re.S)
    assert body and int(body.group(1)) == n, name
    vals = [float.fromhex(v) for v in re.findall(r"(-?0x[0-9a-fA-F.]+p[-+]?\d+)f", body.group(2))]
    assert len(vals) == n, (name, len(vals))
    arr = np.array(vals, np.float64)
    assert (arr.astype(np.float32).astype(np.float64) == arr).all(), f"{name}: an entry is not a binary32 value"
    return arr.astype(np.float32)


@pytest.fixture(scope="module")
def tables():
    return committed_table("kTonemapExposure", 64), committed_table("kTonemapThreshold", 256)


def test_committed_tables_equal_their_formulas_and_are_monotonic(tables):
    P, T = tables
    assert (P.view(np.uint32) == tm.exposure_table().view(np.uint32)).all()
    assert (T.view(np.uint32) == tm.threshold_table().view(np.uint32)).all()
    assert P[0] == 1.0 and (np.diff(P.astype(np.float64)) < 0).all() and P[63] > 0.5
    assert T[0] == 0.0 and (np.diff(T[1:].astype(np.float64)) > 0).all() and T[1] > 0.0 and T[255] < 1.0


def test_decoding_a_code_and_encoding_it_returns_the_code():
    k = np.arange(256)
    lin = tm.srgb_decode(k / 255.0).astype(np.float32)
    assert (tm.encode(lin) == k).all()
    # ... and the encoder is the nearest code of the float64 sRGB encoding wherever that is not within 1e-6 of a tie
    y = np.random.default_rng(5).random(20000).astype(np.float32)
    enc = np.where(y <= 0.0031308, 12.92 * y.astype(np.float64), 1.055 * y.astype(np.float64) ** (1 / 2.4) - 0.055) * 255.0
    clear = np.abs(enc - np.floor(enc) - 0.5) > 1e-6
    assert (tm.encode(y)[clear] == np.rint(enc[clear])).all()
    assert list(tm.encode(np.array([np.nan, -1.0, -0.0, 0.0, np.inf, -np.inf, 1.0, 3e38], np.float32))) == [0, 0, 0, 0, 255, 0, 255, 255]


# ---- the scalar restatement: one pixel at a time, from the header's text, the committed tables ----------------------------------------
def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def s_lum(r, g, b):
    return F(F(F(0.25) * r) + F(F(0.5) * g)) + F(F(0.25) * b)


def s_histogram(img):
    hist, ignored = [0] * 256, 0
    for r, g, b, _ in img.reshape(-1, 4):
        L = s_lum(r, g, b)
        if L > 0:
            hist[min(max((f32_bits(L) >> 20) - 888, 0), 255)] += 1
        else:
            ignored += 1
    return hist, ignored


def s_solve(hist, prev, p, P):
    N = sum(hist)
    if N == 0:
        target = F(p["exposure"])
    else:
        lo, hi = N * p["low_permille"] // 1000, N * p["high_permille"] // 1000
        order = [b for b in range(256) for _ in range(hist[b])][lo:N - hi]      # the kept pixels' bins, as a sorted list
        K, S = len(order), sum(2 * b + 1 for b in order)
        m = 4 * S // K
        target = F(np.ldexp(F(F(p["key"]) * P[m % 64]), 16 - m // 64))
    e = target
    if prev is not None and F(p["adapt"]) < 1:
        e = F(F(prev) + F(F(target - F(prev)) * F(p["adapt"])))
    e = F(p["exposure_min"]) if e < F(p["exposure_min"]) else e
    e = F(p["exposure_max"]) if e > F(p["exposure_max"]) else e
    return F(e)


def s_pixel(c, e, p, T):
    x = [F(F(v) * e) for v in c[:3]]
    if p["op"] == 1:
        Lx = s_lum(*x)
        s = F(F(F(1) + F(Lx / F(F(p["white"]) * F(p["white"])))) / F(F(1) + Lx))
        y = [F(v * s) for v in x]
    elif p["op"] == 2:
        y = [F(F(v * F(F(F(2.51) * v) + F(0.03))) / F(F(v * F(F(F(2.43) * v) + F(0.59))) + F(0.14))) for v in x]
    else:
        y = x
    return [0 if v != v else bisect.bisect_right(T, float(v)) for v in y] + [255]


@pytest.mark.parametrize("name", ti.FAMILIES)
def test_mirror_equals_the_scalar_restatement(name, tables):
    P, T = tables
    Tl = [float(v) for v in T[1:]]
    rng = np.random.default_rng(11)
    with np.errstate(all="ignore"):
        for h, w in ti.SIZES:
            img = ti.family(name, h, w)
            small = h * w <= 1024
            for params in ti.parameter_sets():
                p = dict(tm.DEFAULTS); p.update(params)
                got = tm.tonemap(img, **params)
                if p["auto"]:
                    hist, ignored = s_histogram(img) if small else (list(got["hist"]), got["ignored"])
                    assert list(got["hist"]) == hist and got["ignored"] == ignored and sum(hist) + ignored == h * w
                    e = s_solve(hist, None, p, P)
                else:
                    assert got["hist"] is None
                    e = F(p["exposure"])
                assert f32_bits(got["exposure"]) == f32_bits(e), (name, h, w, params)
                flat, disp = img.reshape(-1, 4), got["display"].reshape(-1, 4)
                for i in (range(h * w) if small else rng.choice(h * w, 300, replace=False)):      # above 1024 pixels a sample
                    assert list(disp[i]) == s_pixel(flat[i], e, p, Tl), (name, h, w, params, int(i), flat[i])


def test_adapt_moves_a_share_of_the_way_and_reset_forgets(tables):
    P, _ = tables
    a, b = ti.hdr(5, 7), ti.hdr(5, 7) * F(16.0)
    t = tm.Tonemapper()
    prev, seq = None, []
    for k, img in enumerate([a, b, b, b, b]):
        if k == 3:
            t.reset(); prev = None
        out = t(img, adapt=0.25)
        want = s_solve(s_histogram(img)[0], prev, dict(tm.DEFAULTS, adapt=0.25), P)
        assert f32_bits(out["exposure"]) == f32_bits(want), k
        prev = want
        seq.append(float(want))
    target_b = float(tm.tonemap(b)["exposure"])
    assert seq[0] > seq[1] > seq[2] > target_b and seq[3] == target_b == seq[4]
    # a manual call neither reads nor replaces the stored exposure
    t(a, auto=False, exposure=3.0)
    assert float(t.prev) == seq[4]


def test_scaling_by_a_power_of_two_scales_the_exposure_and_keeps_the_bytes():
    g = np.random.default_rng(3)
    img = np.ones((37, 53, 4), np.float32)
    img[..., :3] = np.exp2(g.uniform(-9.0, 9.0, (37, 53, 1)) + g.uniform(-0.5, 0.5, (37, 53, 3))).astype(np.float32)
    L = tm.lum(img[..., 0], img[..., 1], img[..., 2])
    assert L.min() * 2.0 ** -3 > 2.0 ** -16 and L.max() * 2.0 ** 3 < 2.0 ** 16        # every luminance stays inside the bin range
    for op in (0, 1, 2):
        base = tm.tonemap(img, op=op)
        for j in range(-3, 4):
            scaled = img.copy()
            scaled[..., :3] *= F(2.0 ** j)
            out = tm.tonemap(scaled, op=op)
            assert float(out["exposure"]) == float(base["exposure"]) * 2.0 ** -j, (op, j)
            assert (out["display"] == base["display"]).all(), (op, j)
            assert (np.roll(base["hist"], 8 * j) == out["hist"]).all()


def test_defaults_keep_the_lit_golden_scene_from_blowing_out():
    """tests/golden/c1_light_8f.npz, final image (96 x 96, the 30 x emissive light): pixels with a channel at 255 under the plain clamp of
    rtgl_read_image_u8 and under rtgl_tonemap's defaults; DESIGN.md 5.9 records both counts and the mean code."""
    img = np.load(os.path.join(ROOT, "tests", "golden", "c1_light_8f.npz"))["expected"].astype(np.float32)
    clamp = np.rint(np.clip(np.nan_to_num(img[..., :3], nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
    out = tm.tonemap(img)
    blown_clamp = int((clamp == 255).any(-1).sum())
    blown_tone = int((out["display"][..., :3] == 255).any(-1).sum())
    mean_code = float(out["display"][..., :3].mean())
    print(f"c1_light_8f: channel at 255 in {blown_clamp} pixels with the clamp, {blown_tone} with the defaults; exposure {float(out['exposure']):.6g}, "
          f"mean code {mean_code:.2f} (clamp: {float(clamp.mean()):.2f}), ignored {out['ignored']}")
    assert blown_tone < blown_clamp
    assert 64.0 < mean_code < 192.0                                    # neither a dark nor a washed-out picture
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 5.9"):design.index("## 6.")]
    assert f"in **{blown_clamp}** pixels" in section and f"in **{blown_tone}** with the defaults" in section and f"**{mean_code:.2f}**" in section
