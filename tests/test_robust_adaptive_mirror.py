"""tests/robust_adaptive_mirror.py without a GPU (include/rtgl_amd.h, "robust adaptive sampling"): with uniform counts the session is the
plain robust session and its error estimate, bit for bit; the mirror equals a scalar per-pixel restatement written from the header; the
special-value families of tests/robust_inputs.py put a non-finite output only where they were injected, and every tile record is finite;
each seeded defect of the scalar restatement is caught by the named case tests/test_gpu_robust_adaptive.py also runs; and the mirror
refuses every parameter record the library refuses."""
import numpy as np
import pytest

import adaptive_mirror as am
import robust_adaptive_inputs as rai
import robust_adaptive_mirror as ram
import robust_error_mirror as rem
import robust_mirror as rm

f32 = np.float32
INF = f32(np.inf)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    """bit for bit, except that a NaN equals any NaN (its sign and payload are not defined)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------------------- 1. uniform counts: the robust session

@pytest.mark.parametrize("K", rai.BUCKETS)
@pytest.mark.parametrize("size", [(8, 8), (24, 40), (70, 53), (130, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_uniform_counts_reduce_to_the_robust_session(size, K):
    w, h = size
    s = am.shape(h, w)
    inside = np.zeros((h, w), bool)
    inside[:s["fh"], :s["fw"]] = True
    for name in rai.UNIFORM:
        case = rai.make(name, h, w, K)
        N = rai.uniform_count(name, K)
        sess, plain = ram.Session(h, w, **case["params"]), rm.Session(h, w, K)
        for step in case["steps"]:
            if step[0] == "fold":
                sess.fold(step[1])
                plain.accumulate(step[1])
                assert same(sess.planes[:, inside], plain.planes[:, inside]) and (bits(sess.planes[:, ~inside]) == 0).all()
        assert (sess.n[am.tile_pixels(h, w) > 0] == N).all() and (sess.n[am.tile_pixels(h, w) == 0] == 0).all()
        for gain in case["gains"]:
            for dest, want in ((ram.DEST_BUFFER, rm.output_plane), (ram.DEST_IMAGE, rm.image_plane)):
                got = sess.resolve(gain, dest)
                assert same(got[inside], want(plain.planes, N, gain)[inside]) and (bits(got[~inside]) == 0).all()
        summary = sess.update()
        rec = sess.records
        assert (rec["samples"] == sess.n).all() and (rec["samples_snapshot"] == sess.n).all() and (sess.m == sess.n).all()
        if N >= K:
            p = case["params"]
            want = rem.estimate(plain.planes, N, threshold=p["threshold"], floor=p["floor"], gain=p["gain"])["tiles"]
            for key in ("sum", "mse"):
                assert same(rec[key], want[key]), (name, key)
            for key in ("count", "converged"):
                assert (rec[key] == want[key]).all(), (name, key)
        else:
            assert not rec["count"].any() and not rec["converged"].any() and (bits(rec["sum"]) == 0).all() and (bits(rec["mse"]) == 0).all()
        assert summary["samples_total"] == N * s["fh"] * s["fw"] and summary["samples_min"] == summary["samples_max"] == N


# ---------------------------------------------------------------------------------------------- 2. a scalar restatement, with seeded defects

def lum1(p):
    return (f32(0.25) * p[0] + f32(0.5) * p[1]) + f32(0.25) * p[2]


def keys_ranks_G(b, K):
    """steps 1-6 of rtgl_robust_resolve for one pixel's K buckets (K, 4)"""
    key = []
    for j in range(K):
        l = lum1(b[j])
        key.append(l if np.isfinite(l) else INF)
    rank = [sum(1 for i in range(K) if i != j and (key[i] < key[j] or (key[i] == key[j] and i < j))) for j in range(K)]
    S, A = f32(0), f32(0)
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
    return key, rank, G


def trim1(G, gain, K):
    cap = (K - 1) // 2
    u = (G * f32(gain)) * f32(K // 2)
    return cap if u >= f32(cap) else int(u)


def resolve_pixel(b, N, K, gain, zero_below=True):
    """steps 7-9: (out (4,), G)"""
    _, rank, G = keys_ranks_G(b, K)
    t = trim1(G, gain, K)
    if N < K and zero_below:
        t = 0
    W, C = f32(0), [f32(0)] * 4
    for j in range(K):
        nj = N // K + (1 if j < N % K else 0)
        if nj > 0 and t <= rank[j] <= K - 1 - t:
            W = W + f32(nj)
            C = [C[c] + f32(nj) * b[j][c] for c in range(4)]
    return [C[c] / W for c in range(4)], G


def error_pixel(b, K, gain, floor):
    """steps 1-9 of rtgl_robust_error_estimate for one pixel: (e, counts)"""
    key, rank, G = keys_ranks_G(b, K)
    t = trim1(G, gain, K)
    lo = [key[j] for j in range(K) if rank[j] == t][0]
    hi = [key[j] for j in range(K) if rank[j] == K - 1 - t][0]
    wins = []
    for j in range(K):
        v = lo if key[j] < lo else key[j]
        wins.append(hi if v > hi else v)
    M, T = f32(0), f32(0)
    for j in range(K):
        M = M + wins[j]
        if t <= rank[j] <= K - 1 - t:
            T = T + key[j]
    mw = M / f32(K)
    D = f32(0)
    for j in range(K):
        d = wins[j] - mw
        D = D + d * d
    hk = K - 2 * t
    mu = T / f32(hk)
    v = D / f32(hk * (hk - 1))
    den = (mu if mu > 0 else f32(0)) + f32(floor)
    e = v / (den * den)
    return e, bool(e - e == 0)


class ScalarSession:
    """robust_adaptive_mirror.Session pixel by pixel and tile by tile, written from the header; `defect` seeds one mistake"""

    def __init__(self, h, w, defect=None, **params):
        self.h, self.w, self.defect, self.params = h, w, defect, params
        self.s = am.shape(h, w)
        self.K = params["buckets"]
        nt = self.s["ty"] * self.s["tx"]
        self.planes = np.zeros((self.K, h, w, 4), f32)
        self.n, self.m = [0] * nt, [0] * nt
        self.records = np.zeros((self.s["ty"], self.s["tx"]), ram.TILE_DTYPE)
        self.folds = 0
        self.mask = [1 if self.pixels(t) else 0 for t in range(nt)]

    def pixels(self, t):
        """the footprint pixels (y, x) of tile t, row-major"""
        y0, x0 = t // self.s["tx"] * 16, t % self.s["tx"] * 16
        return [(y, x) for y in range(y0, min(y0 + 16, self.s["fh"])) for x in range(x0, min(x0 + 16, self.s["fw"]))]

    def set_mask(self, tiles):
        flat = np.asarray(tiles).ravel()
        self.mask = [1 if flat[t] and self.pixels(t) else 0 for t in range(len(self.n))]

    def fold(self, image):
        K = self.K
        with np.errstate(all="ignore"):
            for t, on in enumerate(self.mask):
                if not on:
                    continue
                n = self.n[t]
                j, k = n % K, n // K
                if self.defect == "k_is_n":
                    k = n
                if self.defect == "j_from_frame_count":
                    j = self.folds % K
                for y, x in self.pixels(t):
                    for c in range(4):
                        self.planes[j, y, x, c] = (image[y, x, c] + self.planes[j, y, x, c] * f32(k)) / f32(k + 1)
                self.n[t] = n + 1
        self.folds += 1

    def update(self):
        p, K = self.params, self.K
        thr = f32(p["threshold"])
        with np.errstate(all="ignore"):
            for t in range(len(self.n)):
                n = self.n[t]
                if n == self.m[t] and self.defect != "stale_reestimated":
                    continue
                rec = np.zeros((), ram.TILE_DTYPE)
                rec["samples"] = rec["samples_snapshot"] = n
                if n >= K:
                    leaves, count = [f32(0)] * 256, 0
                    y0, x0 = t // self.s["tx"] * 16, t % self.s["tx"] * 16
                    for y, x in self.pixels(t):
                        e, counts = error_pixel(self.planes[:, y, x], K, p["gain"], p["floor"])
                        if counts:
                            leaves[(y - y0) * 16 + (x - x0)] = e
                            count += 1
                    while len(leaves) > 1:
                        leaves = [leaves[i] + leaves[i + 1] for i in range(0, len(leaves), 2)]
                    if count:
                        mse = leaves[0] / f32(count)
                        rec["sum"], rec["mse"], rec["count"], rec["converged"] = leaves[0], mse, count, int(mse <= thr * thr)
                elif self.defect == "short_marked_valid":
                    rec["count"], rec["converged"] = len(self.pixels(t)), 1
                self.records[t // self.s["tx"], t % self.s["tx"]] = rec
                if self.defect != "m_not_updated":
                    self.m[t] = n
        self.mask = list(am.rule(self.h, self.w, self.records, p["min_samples"], p["max_samples"]).ravel())
        return am.summary(self.h, self.w, self.records, np.array(self.mask, np.uint8), p["max_samples"])

    def resolve(self, gain, dest):
        out = np.zeros((self.h, self.w, 4), f32)
        with np.errstate(all="ignore"):
            if self.defect == "outside_is_nan":
                out[:] = f32(0) / f32(0)
            for t in range(len(self.n)):
                N = max(self.n) if self.defect == "nj_from_largest_n" else self.n[t]
                if self.n[t] == 0:
                    continue
                for y, x in self.pixels(t):
                    v, G = resolve_pixel(self.planes[:, y, x], N, self.K, gain, zero_below=self.defect != "t_not_zeroed")
                    out[y, x] = v if dest == ram.DEST_IMAGE else v[:3] + [G]
        return out


def trace(case, session):
    """everything a case lets one observe, in order: (label, array or summary)"""
    seen = []

    def on_step(index, step, result):
        if step[0] == "fold":
            seen.append((f"{index} buckets", session.planes.copy()))
        elif step[0] == "update":
            rec = session.records
            seen.append((f"{index} records", np.stack([rec["sum"], rec["mse"]] + [rec[k].astype(f32) for k in ("count", "converged", "samples", "samples_snapshot")])))
            seen.append((f"{index} mask", np.array(session.mask, f32).ravel()))
            seen.append((f"{index} summary", result))
        elif step[0] == "resolve":
            for key, picture in result.items():
                seen.append((f"{index} resolve {key}", picture))
    rai.run(case, session, on_step)
    return seen


def differences(a, b):
    assert [label for label, _ in a] == [label for label, _ in b]
    bad = []
    for (label, x), (_, y) in zip(a, b):
        if isinstance(x, dict):
            if am.same_summary(x, y):
                bad.append(label)
        elif not same(x, y):
            bad.append(label)
    return bad


SCALAR_CASES = [(name, (8, 8), K) for name in rai.NAMES for K in rai.BUCKETS] + [(name, (70, 53), 4) for name in ("counts", "stale", "specials", "nonfinite")]


@pytest.mark.parametrize("name,size,K", SCALAR_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_the_mirror_equals_the_scalar_restatement(name, size, K):
    w, h = size
    case = rai.make(name, h, w, K)
    got = trace(case, ram.Session(h, w, **case["params"]))
    want = trace(case, ScalarSession(h, w, **case["params"]))
    assert differences(got, want) == []


@pytest.mark.parametrize("defect", sorted(rai.DEFECT_CASES))
def test_every_seeded_defect_is_caught_by_its_named_case(defect):
    w, h, K = 24, 40, 4                                      # 2 x 3 tiles: one of each target count
    case = rai.make(rai.DEFECT_CASES[defect], h, w, K)
    good = trace(case, ram.Session(h, w, **case["params"]))
    bad = trace(case, ScalarSession(h, w, defect=defect, **case["params"]))
    assert differences(good, bad) != [], defect


def test_a_tile_with_n_equal_m_is_not_read():
    """the buckets changed behind the session's back: the records of the tiles that did not move stay what they were"""
    w, h, K = 24, 40, 4
    case = rai.make("uniform-K+1", h, w, K)
    sess = ram.Session(h, w, **case["params"])
    rai.run(case, sess)
    before = sess.records.copy()
    sess.planes = (sess.planes[::-1] * f32(3)).copy()
    sess.update()
    assert sess.records.tobytes() == before.tobytes()
    sess.set_mask(rai.named_masks(h, w)["one"])
    sess.fold(case["steps"][0][1])
    sess.update()
    moved = sess.records.tobytes() != before.tobytes()
    changed = np.array([sess.records.ravel()[t].tobytes() != before.ravel()[t].tobytes() for t in range(before.size)]).reshape(before.shape)
    assert moved and (changed == (rai.named_masks(h, w)["one"] != 0)).all()


# ---------------------------------------------------------------------------------------------- 3. special values

@pytest.mark.parametrize("name,size,K", rai.listed_cases(), ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_non_finite_outputs_only_where_they_were_injected_and_finite_records(name, size, K):
    w, h = size
    case = rai.make(name, h, w, K)
    assert case["injected"].sum() * 4 <= h * w
    sess = ram.Session(h, w, **case["params"])

    def on_step(index, step, result):
        if step[0] == "update":
            rec = sess.records
            assert np.isfinite(rec["sum"]).all() and np.isfinite(rec["mse"]).all(), (index, rec)
            if name != "stale":                              # (whose records are overwritten with a sentinel on purpose)
                assert (rec["count"] <= am.tile_pixels(h, w)).all() and (rec["converged"] <= 1).all()
        elif step[0] == "resolve":
            for key, picture in result.items():
                assert np.isfinite(picture[~case["injected"]]).all(), (index, key)
    rai.run(case, sess, on_step)
    if name in ("nonfinite", "overflow") and h * w >= 64:
        assert not np.isfinite(sess.resolve(1.0, ram.DEST_IMAGE)).all()      # (the family does reach the output)


def test_t_reaches_zero_and_its_cap():
    h, w, K = 16, 16, 8
    for name, want in (("equal", 0), ("overflow", rm.trim_cap(K))):
        case = rai.make(name, h, w, K)
        sess = ram.Session(h, w, **case["params"])
        rai.run(case, sess)
        _, _, t = rm.resolve(sess.planes, int(sess.n[0, 0]), 1.0)
        assert (t[case["injected"]] == want).all(), name


# ---------------------------------------------------------------------------------------------- 4. refusals, lists, defaults

def test_the_mirror_refuses_every_invalid_record():
    assert ram.valid_params(**ram.DEFAULTS)
    for K in rai.BUCKETS:
        assert ram.valid_params(**rai.params_of(K))
    for bad in rai.invalid_params():
        record = dict(ram.DEFAULTS, flags=0, reserved=0)
        record.update(bad)
        assert not ram.valid_params(**record), bad
    assert ram.valid_params(**dict(ram.DEFAULTS, max_samples=1 << 24)) and ram.valid_params(**dict(ram.DEFAULTS, min_samples=8, max_samples=8))
    for gain, dest in ((np.nan, 0), (np.inf, 0), (-1.0, 0), (1.0, 2)):
        assert not rm.valid_resolve_params(gain, dest)


def test_mask_rule_and_lists_are_adaptive_samplings():
    h, w = 53, 70
    sess = ram.Session(h, w, buckets=4, min_samples=4, max_samples=6)
    assert (sess.mask == am.full_mask(h, w)).all() and (sess.blocks() == am.block_list(h, w, am.full_mask(h, w))).all()
    assert not sess.mask[3].any() and not sess.mask[:, 4].any() and sess.mask[:3, :4].all()     # tiles without footprint pixels are never active
    sess.set_mask(np.ones((4, 5), np.uint8))
    assert (sess.mask == am.full_mask(h, w)).all() and (sess.tiles() == am.tile_list(am.full_mask(h, w))).all()
    rng = np.random.default_rng(5)
    for k in range(7):
        sess.fold(rng.random((h, w, 4), f32))
        summary = sess.update()
        n = k + 1
        assert (sess.mask == am.rule(h, w, sess.records, 4, 6)).all()
        if n < 4:
            assert summary["tiles_active"] == 12 and not sess.records["count"].any()
        if n >= 6:
            assert summary["converged"] == 1 and not sess.mask.any()
            break
    assert (sess.n[:3, :4] == 6).all() and not sess.n[3].any() and not sess.n[:, 4].any()
