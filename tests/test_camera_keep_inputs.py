"""tests/camera_keep_inputs.py on the CPU: the Python restatement of widening(), decide() and lean() equals the header's (through
tests/cpp/camera_keep_shim.cpp) on every frame of every default sequence and on 10,000 random key / frame pairs with every single-field
change; the context model gives the hand-written expectations of tests/test_gpu_camera_lean.py; the default sequences cover every event
kind twice, reuse the bits on at least a third of their frames and rebuild them on at least a fifth; and the oracle's images of the
default sequences hold no NaN, so that the device comparison (bits, no tolerance) cannot be weakened by one."""
import ctypes as C

import numpy as np
import pytest

import camera_keep_inputs as ck
import scene_fuzz_inputs as sf
from test_camera_keep_rays import build_shim, shim_widening

sc = ck.sc


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("camera_keep_inputs"))


def shim_decide(lib, key, frame, opt_lean, aov):
    k = np.array([key.valid, key.n0, key.words, key.scene], np.uint64)
    f = np.array([frame.culled, frame.single, frame.enabled, frame.room, frame.n0, frame.words, frame.scene], np.uint64)
    kc, fc = np.frombuffer(key.camera, np.uint32).copy(), np.frombuffer(frame.camera, np.uint32).copy()
    out, add = np.zeros(3, np.int32), np.zeros(2, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.camera_keep_decide(p(k), p(kc), p(f), p(fc), int(opt_lean), int(aov), p(out), p(add))
    return bool(out[0]), bool(out[1]), bool(out[2]), add[0], add[1]


def python_decide(key, frame, opt_lean, aov):
    d = ck.decide(key, frame)
    return d.cached, d.have_bits, ck.lean(d, opt_lean, aov), d.ro_add, d.sigma_add


def same(a, b):
    return a[:3] == b[:3] and np.float32(a[3]).tobytes() == np.float32(b[3]).tobytes() and np.float32(a[4]).tobytes() == np.float32(b[4]).tobytes()


# ------------------------------------------------------------------------------------------------ the restatement against the header

def test_python_widening_equals_the_header(shim):
    rng = np.random.default_rng(5)
    words = [ck.camera_words(c.fields) for c in ck.cameras()]
    for _ in range(3000):                                  # drawn around the refusal edges as well: aperture / focal near 1 / 4, jitter near the ulp of |pos|
        w = words[int(rng.integers(len(words)))].copy()
        f = w.view(np.float32)
        f[3] = np.float32(10.0 ** rng.uniform(-3, 2)) * np.float32(rng.choice([1.0, -1.0]))
        f[2] = np.float32(abs(f[3]) * rng.choice([0.2499, 0.25, 0.2501, 10.0 ** rng.uniform(-4, -0.6)]))
        f[4:7] = (sf._unit(rng.normal(size=3)) * 10.0 ** rng.uniform(0, 8)).astype(np.float32)
        w[0] = int(rng.random() < 0.9)
        words.append(w)
    accepted = 0
    for w in words:
        got, want = ck.widening(w), shim_widening(shim, w)
        assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes(), (w.view(np.float32)[1:7], got, want)
        accepted += got[0]
    assert len(words) // 4 < accepted < 3 * len(words) // 4 + len(words) // 8


def test_python_decide_equals_the_header_on_random_pairs(shim):
    rng = np.random.default_rng(6)
    cams = [ck.camera_words(c.fields) for c in ck.cameras()]
    n = reused = changed_fields = 0
    while n < 10000:
        w = cams[int(rng.integers(len(cams)))].copy()
        frame = ck.Frame(*(bool(rng.random() < 0.9) for _ in range(4)), int(rng.choice([3072, 6144, 12288])), int(rng.integers(1, 4)), int(rng.integers(1, 4)), w.tobytes())
        for field in [None] + list(range(16)) + ["n0", "words", "scene", "valid"]:      # the key of this very frame, then every single-field change
            kw = w.copy()
            key = ck.Key(True, frame.n0, frame.words, frame.scene, None)
            if isinstance(field, int):
                if field == 0:
                    kw[0] ^= 1
                else:
                    how = int(rng.integers(4))
                    f = kw.view(np.float32)
                    if how == 0:
                        kw[field] ^= 0x80000000            # the sign alone: 0.0 against -0.0 where the field is zero
                    elif how == 1:
                        f[field] = np.float32(np.nan)
                    elif how == 2:
                        kw[field] += 1                     # one ulp
                    else:
                        f[field] = f[field] + np.float32(0.0009765625)
                changed_fields += 1
            elif field == "n0":
                key = key._replace(n0=frame.n0 + 128)
            elif field == "words":
                key = key._replace(words=frame.words + 1)
            elif field == "scene":
                key = key._replace(scene=frame.scene + (1 << 32))      # (a 64-bit version)
            elif field == "valid":
                key = key._replace(valid=False)
            key = key._replace(camera=kw.tobytes())
            opt_lean, aov = int(rng.integers(2)), int(rng.random() < 0.2)
            got, want = python_decide(key, frame, opt_lean, aov), shim_decide(shim, key, frame, opt_lean, aov)
            assert same(got, want), (field, key, frame, got, want)
            reused += got[1]
            n += 1
    assert reused > 200 and changed_fields > 5000


def test_model_equals_the_header_on_every_frame_of_the_default_sequences(shim):
    decided = 0
    for seed in ck.default_seeds():
        seq = ck.sequence(seed)
        for variant in ((), (("camera_lean", 0),), (("cull", 0),)):
            for r in ck.trace(seq, options=variant):
                if not r.decided:
                    assert not r.decision.cached and not r.lean
                    continue
                decided += 1
                s = seq.steps[r.step]
                opt_lean = int(r.lean or not (r.decision.cached and r.decision.have_bits))      # what makes lean() agree is checked on its own below
                want = shim_decide(shim, r.key, r.frame, opt_lean, 0)
                assert (r.decision.cached, r.decision.have_bits) == want[:2], (seed, r.step, s.kinds)
                assert r.decision.ro_add.tobytes() == want[3].tobytes() and r.decision.sigma_add.tobytes() == want[4].tobytes()
                for lean_opt in (0, 1):
                    for aov in (0, 1):
                        assert ck.lean(r.decision, lean_opt, aov) == shim_decide(shim, r.key, r.frame, lean_opt, aov)[2]
    assert decided > 300


def test_model_on_the_hand_written_sequence():
    """the twelve steps of tests/test_gpu_camera_lean.py (test_one_context_against_the_oracle_after_every_frame) with the expectations
    written there by hand: the model is not only compared with itself"""
    scene_a, scene_b = sc.scene_mesh(36, 18, env_size=16), sc.scene_mesh(20, 28, env_size=16)
    base = sc.params_c2().replace(max_bounce=4)
    stand = dict(camera_aperture=0.5, camera_focal_length=38.0)
    moved = dict(stand, camera_position=(2.0, 1.0, -33.0))
    wide = dict(camera_aperture=12.0, camera_focal_length=10.0)
    plan = [(stand, False), (stand, True), (stand, True), (moved, False), (moved, True), (dict(use_dof=0), False), (dict(use_dof=0), True),
            ("scene_b", None), (dict(camera_aperture=0.001), False), (dict(camera_aperture=0.001), True), (wide, False), (wide, False)]
    steps, pre = [], []
    for what, _ in plan:
        if what == "scene_b":
            pre = [("upload", "meshes", scene_b.meshes), ("upload", "vertices", scene_b.vertices)]
            continue
        steps.append(ck.Step(tuple(pre), base.replace(frames=len(steps) + 1, **what), True, True, False, ()))
        pre = []
    seq = ck.Sequence(296, 184, scene_a, (), tuple(steps), "hand")
    want = [reuses for what, reuses in plan if what != "scene_b"]
    assert ck.model(seq) == want
    assert [r.lean for r in ck.trace(seq)] == want and not any(r.lean for r in ck.trace(seq, options=(("camera_lean", 0),)))
    assert [r.decision.cached for r in ck.trace(seq)] == [True] * 9 + [False] * 2
    assert not any(ck.model(seq, options=(("cull", 0),)))
    # other frame forms leave the bits alone: first-hit planes reuse them without the lean bounce, two samples and kernel 2 pass them by
    def with_pre(i, *acts):
        s = list(steps[:4])
        s[i] = s[i]._replace(pre=tuple(acts))
        return ck.Sequence(296, 184, scene_a, (), tuple(s), "hand")
    t = ck.trace(with_pre(1, ("option", "aov", 15)))
    assert [(r.decision.have_bits, r.lean) for r in t] == [(False, False), (True, False), (True, False), (False, False)]
    s4 = list(steps[:3])
    s4[1] = s4[1]._replace(params=s4[1].params.replace(samples=2))
    assert [(r.decision.cached, r.decision.have_bits) for r in ck.trace(ck.Sequence(296, 184, scene_a, (), tuple(s4), "hand"))] == [(True, False), (False, False), (True, True)]
    t = ck.trace(ck.Sequence(296, 184, scene_a, (), (steps[0], steps[1]._replace(pre=(("option", "kernel", 2),)), steps[2]._replace(pre=(("option", "kernel", 4),))), "hand"))
    assert [(r.decided, r.decision.have_bits) for r in t] == [(True, False), (False, False), (True, True)]
    # a changed mf_group_quads rebuilds the triangles: a new scene version; the same value again does not
    t = ck.trace(ck.Sequence(296, 184, scene_a, (), (steps[0], steps[1]._replace(pre=(("option", "mf_group_quads", 8),)), steps[2]._replace(pre=(("option", "mf_group_quads", 8),))), "hand"))
    assert [r.decision.have_bits for r in t] == [False, False, True] and [r.frame.scene for r in t] == [1, 2, 2]
    # a batch of two is one set of launches for both frames: not single; submitted without waiting but one by one: single
    pair = (steps[0], steps[1]._replace(pre=(("option", "frame_batch", 2),), sync=False, check=False), steps[2]._replace(sync=False), steps[3]._replace(pre=(("option", "frame_batch", 1),)))
    t = ck.trace(ck.Sequence(296, 184, scene_a, (), pair, "hand"))
    assert [(r.batched, r.decision.cached, r.decision.have_bits) for r in t] == [(False, True, False), (True, False, False), (True, False, False), (False, True, False)]
    assert t[3].key.valid and t[3].frame.camera != t[3].key.camera      # (frame 4 is the moved camera: it finds the standing camera's bits still valid)


# ------------------------------------------------------------------------------------------------ the sequences

def test_sequences_are_deterministic_and_keep_their_conditions():
    odd = 0
    for seed in range(24):
        a, b = ck.sequence(seed), ck.sequence(seed)
        assert (a.W, a.H, a.options, a.camera) == (b.W, b.H, b.options, b.camera) and len(a.steps) == len(b.steps)
        for s, t in zip(a.steps, b.steps):
            assert s.params == t.params and s.kinds == t.kinds and (s.sync, s.check, s.refused) == (t.sync, t.check, t.refused) and len(s.pre) == len(t.pre)
            assert all(x[0] == y[0] and len(x) == len(y) and all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(x[1:], y[1:])) for x, y in zip(s.pre, t.pre))
        assert 40 <= a.W <= 136 and 24 <= a.H <= 88 and 50 <= a.scene.n_triangles <= 1500
        frames = [s for s in a.steps if not s.refused]
        assert 10 <= len(frames) <= 16 and len(ck.replay(a)) == len(frames)
        assert frames[-1].check and frames[-1].sync and frames[-1].params.samples == 1 and not frames[-1].kinds
        opts = dict(a.options)
        for i, s in enumerate(a.steps):
            for act in s.pre:
                if act[0] == "option":
                    opts[act[1]] = act[2]
            if s.refused:                                  # the cycle is in place, nothing is held back, and a sane node buffer follows
                assert opts.get("frame_batch", 1) == 1 and sf.walk(s.pre[-1][2]).visits > 1 << 20
                nxt = a.steps[i + 1]
                assert [x[1] for x in nxt.pre[:2]] == ["spheres", "nodes"] and sf.walk(nxt.pre[1][2], sf.VISIT_BOUND) is not None
        assert (opts["rng_state"], opts["counters"], opts.get("frame_batch", 1), opts.get("aov", 0), opts["kernel"]) == (1, 1, 1, 0, 4)
        odd += bool(a.W % 8 or a.H % 8)
    assert odd > 16


def test_default_sequences_cover_every_event_and_both_kinds_of_frame():
    cov = ck.coverage()
    assert set(cov) == set(ck.EVENT_KINDS) and min(cov.values()) >= 2, {k: v for k, v in cov.items() if v < 2}
    frames = reused = rebuilt = lean = not_cached = 0
    for seed in ck.default_seeds():
        t = ck.trace(ck.sequence(seed))
        frames += len(t)
        reused += sum(r.decision.have_bits for r in t)
        rebuilt += sum(r.decision.cached and not r.decision.have_bits for r in t)
        lean += sum(r.lean for r in t)
        not_cached += sum(not r.decision.cached for r in t)
    print("frames", frames, "reused", reused, "rebuilt", rebuilt, "lean", lean, "not cached", not_cached)
    assert 3 * reused >= frames and 5 * rebuilt >= frames
    assert lean < reused and not_cached >= 12            # bits reused without the lean bounce, and frames the cache does not cover
    assert len(ck.default_seeds()) == 12 and len(ck.SKIPPED_SEEDS) <= 2 and not {s for s, _ in ck.SKIPPED_SEEDS} & set(ck.default_seeds())


def test_no_nan_in_the_oracles_images_of_the_default_sequences(oracle):
    """every seed that default_seeds() yields: no NaN after any frame (a seed that breaks this goes to SKIPPED_SEEDS with its reason)"""
    bad = {}
    for seed in ck.default_seeds():
        seq = ck.sequence(seed)
        img = np.zeros((seq.H, seq.W, 4), np.float32)
        for scene, p, written in ck.replay(seq):
            if written is not None:
                img = written.copy()
            oracle.render(scene, sf.shader_params(scene, p), img, threads=16)
            n = int(np.isnan(img).any(axis=2).sum())
            if n:
                bad[seed] = bad.get(seed, 0) + n
    assert not bad, f"NaN pixels per seed: {bad}"
