"""tests/post_sequence_inputs.py and tests/post_sequence_model.py on the CPU: the generator is deterministic and meets its alphabet and its
hazards, the model predicts both refusal classes for every feature, and on synthetic traced inputs -- the families of the *_inputs.py
modules, no device, no oracle -- the model driven through ONE feature gives, step for step, what that feature's own mirror or stateful
class gives when driven alone: the composition adds nothing."""
import numpy as np
import pytest

import adaptive_mirror as am
import denoise_guided_mirror as dgm
import denoise_inputs as di
import denoise_mirror as dm
import error_inputs as ei
import error_mirror as em
import post_sequence_inputs as ps
import post_sequence_model as pm
import robust_adaptive_mirror as ram
import robust_denoise_inputs as rdi
import robust_denoise_mirror as rdm
import robust_error_mirror as rem
import robust_inputs as ri
import robust_mirror as rm
import temporal_clip_inputs as tci
import temporal_clip_mirror as tcm
import temporal_inputs as ti
import temporal_moments_inputs as mi
import tonemap_inputs as toi
import tonemap_mirror as tmm

f32 = np.float32
S = ps.S
NAN_CAP = ti.NAN_CAP                    # the share the value cases allow (tests/test_denoise_guided_mirror.py, tests/test_temporal_clip_mirror.py)
assert NAN_CAP == tci.NAN_CAP == 0.02
H, W = 53, 70


def words(a):
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool((words(a) == words(b)).all()) if a.dtype == f32 else a.tobytes() == b.tobytes()


class Synthetic:
    """a tracer without a device: every frame is a view of temporal_inputs' step scene through the frame's camera, with an albedo plane of
    temporal_moments_inputs; no NaN anywhere"""

    def __init__(self, seq):
        self.seq, self.k = seq, 0

    def __call__(self, step, params, model):
        if step.kind not in pm.FRAMES:
            return None
        self.k += 1
        rng = np.random.default_rng([self.seq.seed, self.k])
        image, normal, position = ti.view(ps.CAMERAS[step.args["camera"]], self.seq.W, self.seq.H, ti.STEP, rng)
        if step.kind in ps.MASKED_FRAMES:
            return dict(sample=image)
        planes = {pm.A: mi.albedo_plane(self.seq.H, self.seq.W, self.k), pm.N: normal, pm.P: position, pm.IDS: np.zeros(image.shape, np.int32)}
        return dict(image=image, planes=planes)


_walks = {}


def synthetic_walk(seed):
    if seed not in _walks:
        seq = ps.sequence(seed)
        steps = [ps.resolved(seq, s) for s in seq.steps]
        _walks[seed] = (seq, pm.walk(pm.PostModel(seq.H, seq.W), steps, Synthetic(seq), lambda s: ps.frame_params(seq.base, s.args)))
    return _walks[seed]


# ------------------------------------------------------------------------------------------------ the generator

def test_the_generator_is_deterministic():
    for seed in (0, 5, 17):
        a, b = ps.sequence(seed), ps.sequence(seed)
        assert (a.W, a.H, a.units) == (b.W, b.H, b.units) and repr(a.steps) == repr(b.steps)
        assert ps.MIN_STEPS <= len(a.steps) <= ps.MAX_STEPS
    assert repr(ps.sequence(0).steps) != repr(ps.sequence(9).steps), "seeds that share a row differ in their parameters"


@pytest.mark.parametrize("start", [0, 7])
def test_every_alphabet_entry_and_every_hazard_twice(start):
    seqs = [ps.sequence(s) for s in ps.default_seeds(start=start)]
    missing = [name for name, pred in ps.ALPHABET if not any(pred(s) for q in seqs for s in q.steps)]
    assert not missing, f"alphabet entries that never occur: {missing}"
    rare = [(name, n) for name, n in ((name, sum(bool(pred(q.steps)) for q in seqs)) for name, pred in ps.HAZARDS) if n < 2]
    assert not rare, f"hazards in fewer than two sequences: {rare}"
    assert all(ps.MIN_STEPS <= len(q.steps) <= ps.MAX_STEPS for q in seqs)


def test_five_default_sequences_per_size():
    """eight since the robust adaptive session's nine rows joined: five per size as before among the first fifteen, three among the new"""
    sizes = [(q.W, q.H) for q in (ps.sequence(s) for s in ps.default_seeds())]
    assert sorted(set(sizes)) == sorted(ps.SIZES) and all(sizes.count(s) == 8 for s in ps.SIZES)
    assert all(sizes[:15].count(s) == 5 for s in ps.SIZES)
    assert ps.DEFAULT_SEQUENCES == len(ps.ROWS) == 8 * len(ps.SIZES)


def test_the_robust_denoise_hazards_read_the_context_as_the_model_does():
    """the predicates of post_sequence_inputs.RD_HAZARDS work out from the steps whether a call is accepted; the model says the same of
    every one, so a hazard that is met is met with the statuses its name promises"""
    n = accepted = 0
    for seed in ps.default_seeds():
        seq, walk = synthetic_walk(seed)
        for c in ps._rd_calls(seq.steps):
            assert (walk[c.i][0] == 0) == ps._rd_accepted(c), (seed, c.i)
            assert walk[c.i][0] in (0, pm.STATE)
            n += 1
            accepted += walk[c.i][0] == 0
    # six of the hazards ask for a refusal (three restarts, N < K, after robust_end, a second begin), each in two sequences; every one of
    # the nineteen asks for an accepted call, some share one
    assert n - accepted >= 12 and accepted >= 24, (n, accepted)


def test_the_robust_adaptive_hazards_read_the_context_as_the_model_does():
    """post_sequence_inputs._ra_trace works out from the steps the status of every step of RA_JUDGED, and the predicates of RA_HAZARDS
    go by it; the model says the same of every one, and of which sessions are open, K and whether the output is readable"""
    seen = {k: set() for k in ps.RA_JUDGED}
    for seed in ps.default_seeds():
        seq, walk = synthetic_walk(seed)
        for t in ps._ra_trace(seq.steps):
            if t.status is not None:
                assert walk[t.i][0] == t.status, (seed, t.i, t.step.kind, walk[t.i][0], t.status)
                seen[t.step.kind].add(t.status)
            before = walk[t.i - 1][1] if t.i else None
            if before is not None and t.ra:
                assert not isinstance(before["robust_adaptive_mask"], str), (seed, t.i)
                assert isinstance(before["robust_adaptive_output"], str) != t.buffer, (seed, t.i)
                assert before["robust_adaptive_buckets"].shape[0] == t.K, (seed, t.i)
            elif before is not None:
                assert before["robust_adaptive_mask"] == pm.REFUSED, (seed, t.i)
            if before is not None:
                assert isinstance(before["adaptive_mask"], str) != t.ad, (seed, t.i)
    assert all({0, pm.STATE} <= v for k, v in seen.items() if k != "robust_adaptive_begin"), seen      # (the begin is refused for the state on a tiled context only)
    assert all(pm.INVALID in seen[k] for k in ("robust_adaptive_begin", "robust_adaptive_resolve") + ps.MASKED_FRAMES), seen


def test_the_counts_of_the_trace_are_the_models():
    """the per-class counts of post_sequence_inputs._ra_trace against the n of the model's session, read off the records after an
    accepted update: every known count is the count of the tiles of that class"""
    checked = 0
    for seed in ps.default_seeds():
        seq, walk = synthetic_walk(seed)
        trace = ps._ra_trace(seq.steps)
        for t in trace[:-1]:
            if t.step.kind == "robust_adaptive_update" and t.status == 0:
                records = walk[t.i][1]["robust_adaptive_tiles"]
                for c, n in t.n.items():
                    tiles = (ps.mask_tiles("checker", seq.H, seq.W) == c[0]) & (ps.mask_tiles("left", seq.H, seq.W) == c[1]) & (am.tile_pixels(seq.H, seq.W) > 0)
                    if n is not None and tiles.any():
                        assert (records["samples"][tiles] == n).all(), (seed, t.i, c, n)
                        checked += 1
    assert checked >= 40, checked


def test_every_K_has_an_accepted_robust_adaptive_update_with_a_record_that_is_not_zero():
    """a fill that folded one source K times would give mse = 0 in every tile and a rule with nothing to go by; the updates of a row
    both stop tiles and keep tiles going, in five of the nine rows, and three updates do both at once.  Not in all nine, and which five
    depends on the seed: between min_samples = K and max_samples = K + 2 the threshold decides, and it comes in turn from the seed.
    With 0.05 the synthetic frames meet it at n = K, so every tile of rows 16 and 22 stops at the first update and folds from then on
    only under explicit masks; with 0.002 no tile meets it, and rows 21 and 23 end their session before any tile reaches K + 2 (their
    units fold at most once more).  Only the two ends of the rule are free of the data -- below K a tile goes on, at K + 2 it stops --
    and "ra_resolves" (rows 15 and 17) is the unit that puts both into one update; a second fold in the others does not fit 40 steps"""
    spread = {K: 0 for K in ps.BUCKETS}
    mixed, rows = 0, 0
    for seed in ps.default_seeds():
        seq, walk = synthetic_walk(seed)
        stops = keeps = False
        for s, (status, out, summary) in zip(seq.steps, walk):
            if s.kind == "robust_adaptive_update" and status == 0:
                spread[out["robust_adaptive_buckets"].shape[0]] += bool((out["robust_adaptive_tiles"]["mse"] != 0).any())
                mixed += 0 < summary["tiles_active"] < summary["tiles_total"]
                stops |= summary["tiles_active"] < summary["tiles_total"]
                keeps |= summary["tiles_active"] > 0
        rows += stops and keeps
    assert all(spread[K] >= 2 for K in ps.BUCKETS), spread
    assert mixed >= 3 and rows >= 5, (mixed, rows)


@pytest.mark.parametrize("defect", pm.DEFECTS)
def test_every_seeded_defect_is_told_apart(defect):
    """for every name of post_sequence_model.DEFECTS the model with that one rule wrong, walked over the default sequences on the same
    synthetic frames, differs from the model in a status, a read-out or an update's summary, in at least two sequences: the device test
    compares exactly these, so a library with that mistake would fail it.  (No defective library is built.)"""
    def differs(a, b):
        for (sa, oa, ma), (sb, ob, mb) in zip(a, b):
            if sa != sb or (ma is None) != (mb is None) or (ma is not None and am.same_summary(ma, mb)):
                return True
            for name in pm.READOUTS:
                x, y = oa[name], ob[name]
                if name == "planes":
                    if any(not same_readout(x[bit], y[bit]) for bit in pm.BITS):
                        return True
                elif not same_readout(x, y):
                    return True
        return False

    told = []
    for seed in ps.default_seeds():
        seq, walk = synthetic_walk(seed)
        if not any(s.kind.startswith("robust_adaptive") for s in seq.steps):
            continue                                                   # (every defect is a rule of the robust adaptive session: the model is the model without one)
        steps = [ps.resolved(seq, s) for s in seq.steps]
        other = pm.walk(pm.PostModel(seq.H, seq.W, defect=defect), steps, Synthetic(seq), lambda s: ps.frame_params(seq.base, s.args))
        if differs(walk, other):
            told.append(seed)
    assert len(told) >= 2, f"told apart in fewer than two sequences: {told}"


def test_the_seeded_defects_are_named_once_each():
    assert len(pm.DEFECTS) >= 15 and len(set(pm.DEFECTS)) == len(pm.DEFECTS)
    with pytest.raises(AssertionError):
        pm.PostModel(16, 16, defect="no such rule")


def same_readout(x, y):
    if x is y:
        return True
    if isinstance(x, str) or isinstance(y, str):
        return isinstance(x, str) and isinstance(y, str) and x == y
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(same_readout(x[k], y[k]) for k in x)
    if isinstance(x, tuple):
        return isinstance(y, tuple) and len(x) == len(y) and all(same_readout(p, q) for p, q in zip(x, y))
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype.names:
        return x.shape == y.shape and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
    return same(x, y) if x.dtype == f32 and y.dtype == f32 else x.shape == y.shape and bool((x == y).all())


def test_the_buckets_of_an_accepted_robust_denoise_differ_for_every_K():
    """a fill that folded one frame K times would give v0 = 0 everywhere and a filter with nothing to go by"""
    spread = {K: 0 for K in ps.BUCKETS}
    for seed in ps.default_seeds():
        seq, walk = synthetic_walk(seed)
        for s, (status, out, _) in zip(seq.steps, walk):
            if s.kind == "robust_denoise" and status == 0:
                spread[out["robust_frames"][1]] += bool((out["variance"][..., 1] != 0).any())
    assert all(spread[K] >= 1 for K in ps.BUCKETS), spread


def test_both_refusal_classes_are_predicted_for_every_feature():
    seen = {f: set() for f in ps.FEATURES}
    accepted = refused = 0
    for seed in ps.default_seeds():
        seq, walk = synthetic_walk(seed)
        for s, (status, _, _) in zip(seq.steps, walk):
            accepted += status == 0
            refused += status != 0
            for f, kinds in ps.FEATURES.items():
                if s.kind in kinds:
                    seen[f].add(status)
    lacking = {f: sorted(v) for f, v in seen.items() if not {0, pm.INVALID, pm.STATE} <= v}
    assert not lacking, f"features without an accepted step, a -1 and a -4: {lacking}"
    assert refused * 10 >= accepted and accepted > 2 * refused, (accepted, refused)


def test_a_refused_step_changes_no_read_out():
    """rows 0 to 2, and two of the robust adaptive session's: a refused begin, a masked frame with samples = 2, a resolve with dest = 2 and
    the calls after the end leave the session's four read-outs the very arrays they were"""
    for seed in ps.default_seeds()[:3] + [16, 23]:
        seq, walk = synthetic_walk(seed)
        for k in range(1, len(walk)):
            if walk[k][0] != 0:
                before, after = walk[k - 1][1], walk[k][1]
                unchanged = lambda a, b: a is b or (isinstance(a, tuple) and a == b)
                assert all(all(unchanged(after[name][b], before[name][b]) for b in pm.BITS) if name == "planes" else unchanged(after[name], before[name])
                           for name in pm.READOUTS), (seed, k)


def test_the_nan_share_of_the_expected_outputs_stays_under_the_cap():
    total = nans = 0
    for seed in ps.default_seeds():
        for _, out, _ in synthetic_walk(seed)[1]:
            for name in ("image", "denoised", "variance", "history", "moments", "robust_buckets", "robust_output", "robust_adaptive_buckets", "robust_adaptive_output"):
                if not isinstance(out[name], str):
                    total += out[name].size
                    nans += int(np.isnan(out[name]).sum())
    assert total > 0 and nans <= NAN_CAP * total, (nans, total)


# ------------------------------------------------------------------------------------------------ one feature at a time

def planes_of(albedo, normal, position):
    return {pm.A: albedo, pm.N: normal, pm.P: position, pm.IDS: np.zeros(position.shape, np.int32)}


def drive(model, steps, frames):
    """frames: the traced inputs of the render steps, in order"""
    it = iter(frames)
    return pm.walk(model, steps, lambda s, p, m: next(it) if s.kind == "render" else None, lambda s: s.args.get("camera"))


def render(camera=None, frames=0, reset_flag=1):
    return S("render", frames=frames, reset_flag=reset_flag, camera=camera)


def test_the_denoisers_alone():
    image, albedo, normal, position = di.make("benign", H, W, {}, seed=3)
    frame = dict(image=image, planes=planes_of(albedo, normal, position))
    steps = [S("set_aov", mask=7), render()]
    want = []
    for passes in (0, 1, 5):
        for demod in (True, False):
            steps.append(S("denoise", passes=passes, demodulate=demod, sigma_color=16.0, sigma_normal=0.3, sigma_position=0.05))
            want.append(("denoised", dm.denoise(image, albedo, normal, position, passes=passes, demodulate=demod)))
            steps.append(S("denoise_guided", passes=passes, demodulate=demod, sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05, firefly_ratio=1.0))
            want.append(("guided",) + dgm.denoise_guided(image, albedo, normal, position, passes=passes, demodulate=demod))
    walk = drive(pm.PostModel(H, W), steps, [frame])
    for (status, out, _), w in zip(walk[2:], want):
        assert status == 0
        assert same(out["denoised"], w[1]) and (w[0] == "denoised" or same(out["variance"], w[2]))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("family", ["translate", "dolly"])
def test_the_temporal_calls_alone(family, mode):
    seq = mi.make(family, H, W, seed=1)
    steps, frames = [S("set_aov", mask=7), S("set_option", key="temporal_moments", value=mode)], []
    for image, normal, position, camera, albedo in seq:
        steps += [render(camera), S("temporal_accumulate", **tcm.tm.DEFAULTS), S("temporal_clip", **tcm.DEFAULTS)]
        frames.append(dict(image=image, planes=planes_of(albedo, normal, position)))
    walk = drive(pm.PostModel(H, W), steps, frames)
    for k, (H0, H1, M0, M1) in enumerate(tcm.run(seq, mode=mode, clip_params={})):
        after_acc, after_clip = walk[2 + 3 * k + 1][1], walk[2 + 3 * k + 2][1]
        assert same(after_acc["history"], H0) and same(after_clip["history"], H1), k
        if mode:
            assert same(after_acc["moments"], M0) and same(after_clip["moments"], M1), k
        else:
            assert after_acc["moments"] == pm.REFUSED


def test_the_display_transform_alone():
    images = [toi.family(name, H, W) for name in ("hdr", "bin_edges", "hdr", "black")]
    calls = [dict(auto=True, adapt=0.5, op=1), dict(auto=False, exposure=0.5, op=2), dict(auto=True, adapt=0.25, op=0), dict(auto=True, adapt=0.5, op=1)]
    steps, alone, want = [], tmm.Tonemapper(), []
    for img, c in zip(images, calls):
        c = dict(dict(source=0, exposure=1.0, adapt=1.0), **c)
        steps += [render(), S("tonemap", **c)]
        want.append(alone(img, **{k: v for k, v in c.items() if k != "source"}))
    steps.insert(6, S("tonemap_reset"))
    alone2, want = tmm.Tonemapper(), []
    for k, (img, c) in enumerate(zip(images, calls)):
        if k == 3:
            alone2.reset()
        want.append(alone2(img, **c))
    walk = drive(pm.PostModel(H, W), steps, [dict(image=i, planes={}) for i in images])
    got = [out for (status, out, _), s in zip(walk, steps) if s.kind == "tonemap"]
    hist = None
    for g, w in zip(got, want):
        hist = (w["hist"], w["ignored"]) if w["hist"] is not None else hist
        assert same(g["display"], w["display"]) and words(g["exposure"]) == words(w["exposure"])
        assert (g["histogram"][0] == hist[0]).all() and g["histogram"][1] == hist[1]


@pytest.mark.parametrize("family", ["gauss1", "gauss0", "one_noisy_tile"])
def test_the_error_estimate_alone(family):
    fam = ei.family(family, H, W)
    steps = []
    for s in fam:
        steps += [render(frames=s["frames"], reset_flag=0), S("error_estimate", keep_snapshot=False, first_frames=s["params"].get("first_frames", 1))]
    walk = drive(pm.PostModel(H, W), steps, [dict(image=s["image"], planes={}) for s in fam])
    want = ei.run([dict(s, params=dict(first_frames=s["params"].get("first_frames", 1))) for s in fam])
    for k, w in enumerate(want):
        status, out, _ = walk[2 * k + 1]
        assert status == 0 and em.same_result(out["error_summary"], w) == [], k
    assert any(w["valid"] == 1 for w in want)


def test_the_adaptive_session_alone():
    samples = ri.noisy(np.random.default_rng(5), H, W, 6, firefly=0.0)
    params = dict(threshold=0.5, min_samples=2, max_samples=4)
    alone = am.Session(H, W, **params)
    steps = [S("adaptive_begin", **params)]
    results = []
    for k, smp in enumerate(samples):
        if k == 2:
            tiles = ps.mask_tiles("checker", H, W)
            steps.append(S("adaptive_set_mask", tiles=tiles))
            alone.set_mask(tiles)
            results.append(None)
        steps.append(S("adaptive_frame", camera=None))
        alone.frame(smp)
        results.append((alone.image, None))
        if k % 2:
            steps.append(S("adaptive_update"))
            results.append((alone.image, alone.update(), alone.records.copy(), alone.mask.copy()))
    it = iter(samples)
    walk = pm.walk(pm.PostModel(H, W), steps, lambda s, p, m: dict(sample=next(it)) if s.kind == "adaptive_frame" else None)
    for (status, out, summary), w in zip(walk[1:], results):
        assert status == 0
        if w is None:
            continue
        assert same(out["image"], w[0])
        if w[1] is not None:
            assert am.same_summary(summary, w[1]) == [] and out["adaptive_tiles"].tobytes() == w[2].tobytes() and (out["adaptive_mask"] == w[3]).all()


@pytest.mark.parametrize("K", rm.BUCKETS)
def test_the_robust_session_alone(K):
    case = ri.make("ragged", H, W, K)
    alone = rm.Session(H, W, K)
    steps, want = [S("robust_begin", buckets=K)], []
    for smp in case["samples"]:
        steps += [render(), S("robust_accumulate")]
        alone.accumulate(smp)
        want.append(alone.planes.copy())
    for gain in case["gains"]:
        steps += [S("robust_resolve", gain=gain, dest=0), S("robust_error_estimate", threshold=0.05, floor=0.01, gain=gain), S("robust_resolve", gain=gain, dest=1)]
    walk = drive(pm.PostModel(H, W), steps, [dict(image=s, planes={}) for s in case["samples"]])
    for k, w in enumerate(want):
        assert same(walk[2 + 2 * k][1]["robust_buckets"], w), k
    base = 1 + 2 * len(want)
    for k, gain in enumerate(case["gains"]):
        a, b, c = (walk[base + 3 * k + j][1] for j in range(3))
        assert same(a["robust_output"], alone.resolve(gain)) and same(c["image"], alone.resolve(gain, rm.DEST_IMAGE))
        assert em.same_result(b["robust_error_summary"], rem.estimate(alone.planes, alone.N, gain=gain)) == []
        assert c["robust_frames"] == (alone.N, K)


@pytest.mark.parametrize("K", ram.BUCKETS)
def test_the_robust_adaptive_session_alone(K):
    """begin, folds of both kinds, masks, updates and both resolves: what a bare robust_adaptive_mirror.Session gives, fed the same
    samples; every RTGL_ERR_INVALID and RTGL_ERR_STATE of the header's block; a tiled context"""
    samples = ri.noisy(np.random.default_rng(7 + K), H, W, K + 3, firefly=0.0)
    params = dict(buckets=K, threshold=0.05, floor=0.01, gain=1.0, min_samples=K, max_samples=K + 2)
    begin = lambda **over: S("robust_adaptive_begin", **dict(params, **over))
    frame = lambda **over: S("robust_adaptive_frame", camera=None, **over)
    kinds = ("frame", "accumulate", "update", "set_mask", "resolve", "end")
    call = {"frame": frame(), "accumulate": S("robust_adaptive_accumulate"), "update": S("robust_adaptive_update"), "end": S("robust_adaptive_end"),
            "set_mask": S("robust_adaptive_set_mask", tiles=ps.mask_tiles("checker", H, W)), "resolve": S("robust_adaptive_resolve", gain=1.0, dest=0)}
    written = ps.written_image(H, W, 3)
    # without a session: -4 of every call but begin, and the four read-outs refused; the bad arguments of begin and resolve come first
    steps = [call[k] for k in kinds] + [begin(min_samples=K - 1), begin(buckets=5), begin(threshold=0.0), begin(floor=float("nan")), begin(gain=-1.0),
                                       begin(max_samples=K - 1, min_samples=K), begin(max_samples=(1 << 24) + 1), S("robust_adaptive_resolve", gain=1.0, dest=2),
                                       S("write_image", pixels=written), begin()]
    want = [pm.STATE] * 6 + [pm.INVALID] * 8 + [None, None]
    alone, checks = ram.Session(H, W, **params), {}

    def then(step, check=None, status=None):
        steps.append(step)
        want.append(status)
        if check is not None:
            checks[len(steps) - 1] = check

    state = lambda: (alone.planes.copy(), alone.records.copy(), alone.mask.copy())
    then(S("robust_adaptive_resolve", gain=1.0, dest=0), ("output", alone.resolve(1.0)))           # N = 0 everywhere: zeros
    fed = []
    for k, smp in enumerate(samples):
        if k == 2:
            tiles = ps.mask_tiles("checker", H, W)
            alone.set_mask(tiles)
            then(S("robust_adaptive_set_mask", tiles=tiles), ("state", state()))
        if k % 2:
            alone.fold(smp)
            fed.append(smp)
            then(frame(), ("state", state()))
        else:                                                          # the image as it stands: a written one
            alone.fold(written)
            then(S("robust_adaptive_accumulate"), ("state", state()))
        if k >= K - 2:
            summary = alone.update()
            then(S("robust_adaptive_update"), ("update", summary, state()))
    then(frame(samples=2), status=pm.INVALID)                          # in an open session with "aov" 0
    then(S("set_aov", mask=4))
    then(frame(), status=pm.STATE)
    then(frame(samples=2), status=pm.STATE)                            # the state comes first
    then(S("set_aov", mask=0))
    for gain in (1.0, 0.0, 2.5):
        then(S("robust_adaptive_resolve", gain=gain, dest=0), ("output", alone.resolve(gain)))
        then(S("robust_adaptive_resolve", gain=gain, dest=1), ("image", alone.resolve(gain, ram.DEST_IMAGE)))
    then(S("robust_adaptive_resolve", gain=-1.0, dest=0), status=pm.INVALID)
    then(begin(min_samples=K - 1), ("state", state()), status=pm.INVALID)       # a refused begin leaves the session as it is
    alone = ram.Session(H, W, **params)
    then(begin(), ("restarted", state()))                              # a second begin: zeroed, every tile active, the output refused, the image kept
    then(S("robust_adaptive_end"))
    then(S("robust_adaptive_end"), status=pm.STATE)
    it = iter(fed)
    model = pm.PostModel(H, W)
    walk = pm.walk(model, steps, lambda s, p, m: dict(sample=next(it)) if s.kind == "robust_adaptive_frame" else None)
    assert len(walk) == len(want) == len(steps)
    updates = 0
    for k, ((status, out, summary), w) in enumerate(zip(walk, want)):
        assert status == (0 if w is None else w), (k, steps[k].kind, status, w)
        c = checks.get(k)
        if c is None:
            continue
        if c[0] == "output":
            assert same(out["robust_adaptive_output"], c[1]), k
        elif c[0] == "image":
            assert same(out["image"], c[1]), k
        else:
            planes, records, mask = c[-1]
            assert same(out["robust_adaptive_buckets"], planes) and out["robust_adaptive_tiles"].tobytes() == records.tobytes() and (out["robust_adaptive_mask"] == mask).all(), k
        if c[0] == "update":
            assert am.same_summary(summary, c[1]) == [], k
            updates += 1
        if c[0] == "restarted":
            assert out["robust_adaptive_output"] == pm.REFUSED and not out["robust_adaptive_buckets"].any() and same(out["image"], walk[k - 1][1]["image"]), k
    assert updates == 5 and (walk[len(steps) - 4][1]["robust_adaptive_tiles"]["mse"] != 0).any()
    names = ("robust_adaptive_buckets", "robust_adaptive_output", "robust_adaptive_tiles", "robust_adaptive_mask")
    assert all(walk[k][1][n] == pm.REFUSED for k in (0, 13, len(steps) - 1) for n in names)           # no session: all four read-outs
    assert walk[15][1]["robust_adaptive_output"] == pm.REFUSED and not isinstance(walk[15][1]["robust_adaptive_mask"], str)       # begun, not resolved
    assert same(walk[15][1]["image"], written), "the begin does not touch the image"
    it = iter(fed)
    tiled = pm.walk(pm.PostModel(H, W, tiled=True), steps, lambda s, p, m: dict(sample=next(it)) if s.kind == "robust_adaptive_frame" else None)
    for s, (status, out, _), w in zip(steps, tiled, want):
        if s.kind.startswith("robust_adaptive"):
            assert status == (pm.INVALID if w == pm.INVALID and s.kind != "robust_adaptive_frame" else pm.STATE), (s.kind, status)
            assert all(out[n] == pm.REFUSED for n in names)


@pytest.mark.parametrize("K", rm.BUCKETS)
def test_robust_denoise_alone(K):
    """begin, frames and folds, rtgl_robust_denoise: what robust_denoise_mirror gives when fed robust_mirror.Session's planes; the three
    RTGL_ERR_STATE reasons and RTGL_ERR_INVALID"""
    for buckets, guides in (("ragged", "benign"), ("specials", "edges")):
        case = rdi.make(buckets, guides, H, W, K)
        alb, nrm, pos = case["albedo"], case["normal"], case["position"]
        frames = [dict(image=s, planes=planes_of(alb, nrm, pos)) for s in case["samples"]]
        call = lambda **over: S("robust_denoise", **dict(rdm.DEFAULTS, **over))
        alone = rm.Session(H, W, K)
        steps = [S("set_aov", mask=7), call(), S("robust_begin", buckets=K)]
        want = [None, pm.STATE, None]                                  # no session
        for k, smp in enumerate(case["samples"]):
            steps += [render(), S("robust_accumulate"), call(passes=1)]
            alone.accumulate(smp)
            want += [None, None, rdm.robust_denoise(alone.planes, alone.N, alb, nrm, pos, **dict(rdm.DEFAULTS, passes=1)) if k + 1 >= K else pm.STATE]      # N < K
        for ps_ in case["params"]:
            for passes in rdi.PASSES:
                steps.append(call(passes=passes, **ps_))
                want.append(rdm.robust_denoise(alone.planes, alone.N, alb, nrm, pos, **dict(rdm.DEFAULTS, passes=passes, **ps_)))
        steps += [call(passes=9), call(sigma_lum=0.0), call(gain=-1.0), call(sigma_normal=float("inf")), S("set_aov", mask=5), call(),
                  call(sigma_normal=0.0), render(), call(sigma_normal=0.0), S("set_aov", mask=0), call(sigma_normal=0.0, sigma_position=0.0, demodulate=False),
                  S("robust_end"), call(sigma_normal=0.0, sigma_position=0.0, demodulate=False)]
        plain = dict(rdm.DEFAULTS, sigma_normal=0.0, sigma_position=0.0, demodulate=False)
        want += [pm.INVALID] * 4 + [None, pm.STATE,                    # the normal plane is not enabled
                                    pm.STATE, None,                    # the planes restarted
                                    rdm.robust_denoise(alone.planes, alone.N, alb, None, pos, **dict(rdm.DEFAULTS, sigma_normal=0.0)), None,
                                    rdm.robust_denoise(alone.planes, alone.N, **plain),      # no plane needed: the restart does not refuse
                                    None, pm.STATE]
        walk = drive(pm.PostModel(H, W), steps, frames + [frames[-1]])
        assert len(walk) == len(want)
        last, checked = None, 0
        for k, ((status, out, _), w) in enumerate(zip(walk, want)):
            if w is None:
                assert status == 0, k
            elif isinstance(w, int):
                assert status == w, (k, status, w)
            else:
                assert status == 0 and same(out["denoised"], w[0]) and same(out["variance"], w[1]), k
                last, checked = w, checked + 1
                continue
            if last is not None:                                       # a refused call, and every other one, leaves the two buffers as they were
                assert same(out["denoised"], last[0]) and same(out["variance"], last[1]), k
        assert checked >= len(case["samples"]) - K + 1 + len(case["params"]) * len(rdi.PASSES) + 2
        tiled = drive(pm.PostModel(H, W, tiled=True), steps[:3 + 3 * K], frames)
        assert all(status == pm.STATE for (status, _, _), s in zip(tiled, steps) if s.kind == "robust_denoise")
