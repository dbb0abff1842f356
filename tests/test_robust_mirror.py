"""The reference of tests/test_gpu_robust.py, pinned without a GPU (include/rtgl_amd.h, "robust accumulation").

1. The numpy restatement (tests/robust_mirror.py) and a scalar restatement written from the header, pixel by pixel, agree in every bit on
   the families of tests/robust_inputs.py, and what a family states about its result holds.
2. Teeth.  The scalar restatement takes at most one of DEFECTS, each a way the kernel could plausibly be wrong; every defect changes output
   bits on a named case that the GPU module runs.
3. The oracle table of DESIGN.md 5.12, regenerated through the mirror and asserted."""
import math
import os

import numpy as np
import pytest

import robust_inputs as ri
import robust_mirror as rm

f32 = np.float32


def bits(a):
    """the words of `a`, every NaN as one word: the contract defines where a NaN comes out, not its sign or payload (which differ between
    processors, and here between numpy's scalar and array paths)"""
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 1. the scalar restatement

DEFECTS = {
    "no_tie_break": "rank_j counts only key_i < key_j: the tie-break by index is dropped",
    "key_not_mapped": "a non-finite luminance is used as the key as it is",
    "rank_order_sums": "W and C are summed in rank order instead of bucket order",
    "cap_off_by_one": "t is capped at K / 2 instead of (K - 1) / 2",
    "unit_weights": "every kept bucket weighs 1 instead of n_j",
    "trim_while_short": "t is not forced to 0 while N < K",
    "w_not_folded": "the fold leaves w = 1 instead of folding it like a colour",
}


def fold_pixel(b, x, k, defect=None):
    fk, fk1 = f32(k), f32(k + 1)
    out = [(f32(x[c]) + f32(b[c]) * fk) / fk1 for c in range(4)]
    if defect == "w_not_folded":
        out[3] = f32(1)
    return out


def resolve_pixel(b, K, N, gain, defect=None):
    """steps 1-9 of the header for one pixel; b: K buckets of 4 float32.  Returns (out[4], G, t)."""
    inf = f32(np.inf)
    key = []
    for j in range(K):
        l = (f32(0.25) * b[j][0] + f32(0.5) * b[j][1]) + f32(0.25) * b[j][2]
        key.append(l if (math.isfinite(l) or defect == "key_not_mapped") else inf)
    kf = [float(v) for v in key]                                   # (comparisons of binary32 values are the same in binary64)
    rank = []
    for j in range(K):
        r = 0
        for i in range(K):
            if i != j and (kf[i] < kf[j] or (kf[i] == kf[j] and i < j and defect != "no_tie_break")):
                r += 1
        rank.append(r)
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
    cap = K // 2 if defect == "cap_off_by_one" else (K - 1) // 2
    t = cap if u >= f32(cap) else int(u)
    if N < K and defect != "trim_while_short":
        t = 0
    n = [N // K + (1 if j < N % K else 0) for j in range(K)]
    order = range(K) if defect != "rank_order_sums" else sorted(range(K), key=lambda j: rank[j])
    W, C = f32(0), [f32(0)] * 4
    for j in order:
        if n[j] > 0 and t <= rank[j] <= K - 1 - t:
            fn = f32(1) if defect == "unit_weights" else f32(n[j])
            W = W + fn
            C = [C[c] + fn * b[j][c] for c in range(4)]
    return [C[c] / W for c in range(4)], G, t


def restate(samples, K, gain, defect=None):
    """a session by scalars: (planes (K, h, w, 4), output plane, image plane, t)"""
    h, w = samples[0].shape[:2]
    N = len(samples)
    planes = np.zeros((K, h, w, 4), f32)
    buffer_, image, ts = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32), np.zeros((h, w), np.int32)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                b = [[f32(0)] * 4 for _ in range(K)]
                for k, s in enumerate(samples):
                    b[k % K] = fold_pixel(b[k % K], s[y, x], k // K, defect)
                planes[:, y, x] = b
                out, G, t = resolve_pixel(b, K, N, gain, defect)
                buffer_[y, x] = out[:3] + [G]
                image[y, x] = out
                ts[y, x] = t
    return planes, buffer_, image, ts


def mirror(samples, K, gain):
    h, w = samples[0].shape[:2]
    sess = rm.Session(h, w, K)
    for s in samples:
        sess.accumulate(s)
    return sess.planes, sess.resolve(gain, rm.DEST_BUFFER), sess.resolve(gain, rm.DEST_IMAGE), rm.resolve(sess.planes, sess.N, gain)[2]


@pytest.mark.parametrize("K", ri.BUCKETS)
@pytest.mark.parametrize("size", ri.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_mirror_equals_the_scalar_restatement(size, K):
    w, h = size
    for family in ri.FAMILIES:
        case = ri.make(family, h, w, K)
        for gain in case["gains"]:
            got, want = mirror(case["samples"], K, gain), restate(case["samples"], K, gain)
            for name, a, b in zip(("planes", "buffer", "image"), got, want):
                assert (bits(a) == bits(b)).all(), (family, size, K, gain, name)
            assert (got[3] == want[3]).all(), (family, size, K, gain, "t")


@pytest.mark.parametrize("K", ri.BUCKETS)
@pytest.mark.parametrize("size", ri.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_what_the_families_state_about_their_results(size, K):
    w, h = size
    cap = rm.trim_cap(K)

    def run(family, gain=None):
        case = ri.make(family, h, w, K)
        return case, mirror(case["samples"], K, case["gains"][0] if gain is None else gain)

    case, (planes, buf, img, t) = run("equal")                     # the bucket value exactly, G = 0, nothing trimmed
    v = case["samples"][0]
    assert all((bits(p) == bits(v)).all() for p in planes)
    assert (bits(img) == bits(v)).all() and (bits(buf[..., 3]) == 0).all() and not t.any()
    case, (planes, buf, img, t) = run("outlier")                   # exactly the constant
    c = np.minimum.reduce(case["samples"])
    assert (bits(img) == bits(c)).all() and (bits(buf[..., :3]) == bits(c[..., :3])).all() and (t == cap).all()
    case, (planes, buf, img, t) = run("ties")                      # ranks come by index: a permutation whatever the ties
    _, rank, G = rm.gini(planes)
    assert (np.sort(rank, 0) == np.arange(K).reshape(K, 1, 1)).all()
    assert not np.isnan(img).any()
    if w * h > 30:
        assert (G == 0).any() and (t > 0).any()
    case, (planes, buf, img, t) = run("integer_u")                 # u = K / 4 exactly; one ulp below, one bucket fewer goes at either end
    assert (bits(buf[..., 3]) == bits(f32(0.5))).all() and (t == min(K // 4, cap)).all()
    _, (_, buf2, _, t2) = run("integer_u", case["gains"][1])
    assert (t2 == K // 4 - 1).all() and (bits(buf2[..., 3]) == bits(f32(0.5))).all()
    for family in ("short", "gain_zero"):                          # N < K, and gain 0: nothing is trimmed, the weighted mean
        for gain in ri.make(family, h, w, K)["gains"]:
            assert not run(family, gain)[1][3].any(), family
    _, (planes, buf, img, t) = run("gain_huge")                    # t at its cap wherever G > 0
    assert ((t == cap) | (buf[..., 3] == 0)).all() and (t == cap).any()
    _, (planes, buf, img, t) = run("overflow")                     # S = +inf: G = 1, t at its cap
    assert (buf[..., 3] == 1).all() and (t == cap).all() and np.isfinite(planes).all()
    case, (planes, buf, img, t) = run("nonfinite")                 # the NaN comes out where more buckets are non-finite than the trim drops
    bad = (~np.isfinite(planes[..., 0])).sum(0)
    assert (~np.isfinite(img[..., 0]))[bad > cap].all()            # (G = 1, t = cap: the ranks cap .. K - 1 - cap stay, the bad ones are the highest)
    assert np.isfinite(img[..., 0])[(bad <= cap) & (bad > 0)].all()
    assert (buf[..., 3][bad > 0] == 1).all()


def test_counts_and_validation():
    for K in ri.BUCKETS:
        for N in range(0, 3 * K + 2):
            n = rm.bucket_samples(N, K)
            assert n.sum() == N and n.max() - n.min() <= 1 and (np.diff(n) <= 0).all()
            assert rm.bucket_samples(N + 1, K)[rm.next_bucket(N, K)] == rm.next_count(N, K) + 1
    assert [rm.trim_cap(K) for K in ri.BUCKETS] == [1, 3, 7]
    assert all(rm.valid_params(K) for K in ri.BUCKETS) and not any(rm.valid_params(K) for K in (0, 1, 2, 3, 5, 12, 32))
    assert not rm.valid_params(8, flags=1) and not rm.valid_params(8, reserved=(0, 0, 0, 0, 0, 1))
    assert rm.valid_resolve_params(0.0, 0) and rm.valid_resolve_params(1e30, 1)
    for gain in (np.nan, np.inf, -np.inf, -1.0, 1e39):
        assert not rm.valid_resolve_params(gain, 0), gain
    assert not rm.valid_resolve_params(1.0, 2) and not rm.valid_resolve_params(1.0, 0, flags=2) and not rm.valid_resolve_params(1.0, 0, reserved=(1, 0, 0, 0, 0))


# ---------------------------------------------------------------------------------------------- 2. teeth

S70, S17, S7 = (70, 53), (17, 17), (7, 5)
CATCHERS = {
    "no_tie_break": [("ties", S17, 8), ("ties", S7, 4), ("integer_u", S17, 16)],
    "key_not_mapped": [("nonfinite", S17, 8), ("specials", S70, 4)],
    "rank_order_sums": [("ragged", S17, 8), ("full", S70, 16)],
    "cap_off_by_one": [("gain_huge", S17, 8), ("overflow", S7, 4)],
    "unit_weights": [("ragged", S17, 8), ("ragged", S7, 16)],
    "trim_while_short": [("short", S17, 8), ("short", S7, 16)],
    "w_not_folded": [("equal", S7, 4), ("specials", S17, 8)],
}


def test_every_defect_has_catchers():
    assert set(CATCHERS) == set(DEFECTS)


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_each_defect_changes_bits_that_the_comparison_sees(defect):
    listed = ri.listed_cases()
    caught = 0
    for family, (w, h), K in CATCHERS[defect]:
        assert (family, (w, h), K) in listed, f"{family} {w} x {h} K = {K} is not a case of the GPU module"
        case = ri.make(family, h, w, K)
        changed = 0
        for gain in case["gains"]:
            want, got = mirror(case["samples"], K, gain), restate(case["samples"], K, gain, defect)
            changed += sum(int((bits(a) != bits(b)).sum()) for a, b in zip(want[:3], got[:3]))
        print(f"{defect} ({DEFECTS[defect]}): {family} {w} x {h} K = {K}: {changed} words change")
        caught += bool(changed)
    assert caught == len(CATCHERS[defect]), f"a listed case does not see '{DEFECTS[defect]}'"


# ---------------------------------------------------------------------------------------------- 3. the oracle table

def relative_mse(image, truth, floor=0.01):
    """the mean over the picture of ((L - T) / (max(T, 0) + floor))^2 of the luminance"""
    L, T = rm.lum(image[..., :3]).astype(np.float64), rm.lum(truth[..., :3]).astype(np.float64)
    return float(np.mean(((L - T) / (np.maximum(T, 0.0) + floor)) ** 2))


TABLE_N, TABLE_K, TRUTH_FRAMES, SIZE = (32, 64, 128), 8, 1024, 64


@pytest.fixture(scope="module")
def table(rt, oracle):
    """per scene: {N: (mean's relative MSE, robust's, energy kept, share of pixels trimmed)}.  64 x 64, GlibcRand(0), every frame a
    one-sample image (frames = 0, reset_flag = 1); the truth is the binary64 mean of 1,024 of them; mean and robust picture of N frames
    are of the first N."""
    sc = rt.scenes
    scenes = {"scene_c1(True)": (sc.scene_c1(True), sc.params_c1()), "scene_mesh(10, 5, env_size=16)": (sc.scene_mesh(10, 5, env_size=16), sc.params_c2()),
              "scene_c1(False)": (sc.scene_c1(False), sc.params_c1())}
    threads, out = min(16, os.cpu_count() or 1), {}
    for name, (scene, base) in scenes.items():
        g, sess, total, rows = sc.GlibcRand(0), rm.Session(SIZE, SIZE, TABLE_K), np.zeros((SIZE, SIZE, 4), np.float64), {}
        img, at = np.zeros((SIZE, SIZE, 4), f32), {}
        for k in range(TRUTH_FRAMES):
            oracle.render(scene, base.replace(frames=0, reset_flag=1, random=g.rand()), img, threads=threads)
            total += img
            if k < max(TABLE_N):
                sess.accumulate(img)
            if k + 1 in TABLE_N:
                res, _, t = rm.resolve(sess.planes, sess.N, 1.0)
                at[k + 1] = ((total / (k + 1)).astype(f32), res, float((t > 0).mean()))
        truth = total / TRUTH_FRAMES
        for N, (mean, robust, trimmed) in at.items():
            kept = float(rm.lum(robust[..., :3]).astype(np.float64).sum() / rm.lum(mean[..., :3]).astype(np.float64).sum())
            rows[N] = (relative_mse(mean, truth), relative_mse(robust, truth), kept, trimmed)
        out[name] = rows
    print(f"\nrelative MSE of the luminance against {TRUTH_FRAMES} frames, K = {TABLE_K}, gain 1: mean -> robust")
    for name, rows in out.items():
        print(f"  {name}: " + "; ".join(f"N = {N}: {m:.5f} -> {r:.5f}" for N, (m, r, _, _) in rows.items())
              + f"; energy kept (N = 32) {rows[32][2]:.4f}; pixels trimmed (N = 32) {100 * rows[32][3]:.1f} %")
    return out


def test_the_oracle_table(table):
    for name in ("scene_c1(True)", "scene_mesh(10, 5, env_size=16)"):      # the firefly scenes: at most half the mean's error
        mean, robust, _, _ = table[name][32]
        assert robust <= 0.5 * mean, (name, mean, robust)
    mean, robust, _, _ = table["scene_c1(False)"][32]                      # the clean scene: untouched
    assert robust <= 1.1 * mean, (mean, robust)
    for name, rows in table.items():
        assert rows[32][2] >= 0.9, (name, rows[32][2])
