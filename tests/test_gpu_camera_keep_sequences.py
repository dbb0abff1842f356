"""The kept bits of the camera-ray bounce (rtgl_amd.hip, d_keep0; rt_camera_keep.hpp) on the device over whole lives of a context: the
sequences and cameras of tests/camera_keep_inputs.py against the CPU oracle, bit for bit.

  * every default sequence (KEEP_FUZZ_CASES, default 12, from KEEP_FUZZ_SEED, default 0) through one context, 10..16 frames with
    uploads, image writes, camera moves, option switches, batched and unsynced pairs and a refused frame in between: after every frame
    that can be read out the oracle's image and the model's count of lean frames; at the end the oracle's RNG states over the 8 x 8-aligned
    footprint and its paths, segments and env_lookups of the last frame.  One printed line per differing frame.
  * the same sequence with camera_lean pinned to 0, and with cull pinned to 0 (no bits at all): the same final image bits.
  * the named far and limit cameras standing for 12 frames over a scene placed around them: cull 1 and 3, camera_lean 0 and 1, one and two
    scan waves; 11 lean frames where widening() accepts the camera (none where it refuses: aperture from focal / 4 on, and far_5e5_x,
    whose jitter is 1.6 ulps of its position), the oracle's image after frames 1, 2, 6 and 12.
  * one sequence as rank 1 of 2 with strips of 8 rows: lean on and off agree bit for bit and the lean count is the model's.

The refused frame is the host's argument check (a node buffer that expands past the visit cap, tests/test_gpu_scene_fuzz.py): it returns
the invalid-argument error before anything is enqueued.  The oracle's images hold no NaN (tests/test_camera_keep_inputs.py)."""
import os

import numpy as np
import pytest

import camera_keep_inputs as ck
import scene_fuzz_inputs as sf
from test_gpu_scene_fuzz import ERR_INVALID, differences

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "segments", "env_lookups")
UPLOADS = dict(spheres="upload_spheres", materials="upload_materials", nodes="upload_nodes", envmap="upload_envmap", vertices="upload_vertices", meshes="upload_meshes")
STANDING = [c for c in ck.cameras() if c.family == "limit" or c.name in {n[0] for n in ck.FAR_NAMED}]


def fuzz_seeds():
    return ck.default_seeds(int(os.environ.get("KEEP_FUZZ_CASES", str(ck.DEFAULT_SEQUENCES))), int(os.environ.get("KEEP_FUZZ_SEED", "0")))


_oracle_cache = {}


def oracle_sequence(oracle, seed, seq):
    """step index -> the oracle's image after that step's frame; and (image, RNG states, counters) of the last frame.  Computed once per
    seed, never written to"""
    if seed not in _oracle_cache:
        img = np.zeros((seq.H, seq.W, 4), np.float32)
        after, cnt, seeds = {}, None, None
        frames = [i for i, s in enumerate(seq.steps) if not s.refused]
        for i, (scene, p, written) in zip(frames, ck.replay(seq)):
            if written is not None:
                img = written.copy()
            cnt, seeds = oracle.render(scene, sf.shader_params(scene, p), img, threads=16, want_seeds=True)
            after[i] = img.copy()
            after[i].setflags(write=False)
        seeds.setflags(write=False)
        _oracle_cache[seed] = (after, (after[frames[-1]], seeds, cnt))
    return _oracle_cache[seed]


def run_sequence(rt, seq, pinned=(), want=None, lean_counts=None, who="", **tiling):
    """one context through the sequence.  -> (differing frames, one line each; final image; RNG states; counters; lean frames).
    want: step -> expected image (compared wherever the step reads out); lean_counts: step -> expected camera_lean_frames"""
    ctx = rt.host.Context(seq.W, seq.H, **tiling)
    rows = ctx.global_rows()
    for k, v in seq.options + tuple(pinned):
        ctx.set_option(k, v)
    fixed = {k for k, _ in pinned}
    ctx.upload_scene(seq.scene)
    lines = []
    for i, s in enumerate(seq.steps):
        for act in s.pre:
            if act[0] == "option":
                if act[1] not in fixed:
                    ctx.set_option(act[1], act[2])
            elif act[0] == "upload":
                getattr(ctx, UPLOADS[act[1]])(act[2])
            else:
                ctx.write_image(act[1][rows])
        if s.refused:
            ctx.set_params(s.params)
            rc = ctx.lib.rtgl_render_frame(ctx.h)
            assert rc == ERR_INVALID and b"node buffer expands to more than 2^20 sphere tests per ray" in ctx.lib.rtgl_last_error(ctx.h), f"{who} step {i}: the frame was not refused ({rc})"
            continue
        ctx.render(s.params, sync=s.sync)
        if not s.check:
            continue
        got = ctx.read_image()
        n_lean = ctx.get_option("camera_lean_frames")
        d = differences((got, None, None), (want[i][rows], None, None), seq.W, seq.H) if want is not None else []
        if lean_counts is not None and n_lean != lean_counts[i]:
            d.append(f"lean frames {n_lean}, the model says {lean_counts[i]}")
        if d:
            lines.append(f"{who} step {i} {s.kinds}: " + "; ".join(d) + f" | {seq.W} x {seq.H} camera {seq.camera} triangles {seq.scene.n_triangles}")
            print(lines[-1], flush=True)
    out = (lines, ctx.read_image(), ctx.read_rng_state(), ctx.counters(), ctx.get_option("camera_lean_frames"))
    ctx.close()
    return out


# ------------------------------------------------------------------------------------------------ sequences

def test_sequences_match_the_oracle_after_every_frame(rt, oracle):
    seeds = fuzz_seeds()
    bad = frames = lean = 0
    for seed in seeds:
        seq = ck.sequence(seed)
        after, last = oracle_sequence(oracle, seed, seq)
        counts = ck.lean_counts(seq)
        lines, img, rng, cnt, n_lean = run_sequence(rt, seq, want=after, lean_counts=counts, who=f"sequence {seed}")
        d = differences((img, rng, cnt), last, seq.W, seq.H, COUNTERS)
        if d:
            lines.append(f"sequence {seed} at its end: " + "; ".join(d))
            print(lines[-1], flush=True)
        bad += len(lines)
        frames += len(after)
        lean += n_lean
    print("sequences", len(seeds), "frames", frames, "lean frames", lean, "| differing frames:", bad)
    assert bad == 0, f"{bad} frames of {len(seeds)} sequences differ from the oracle or the model (see the lines printed above)"
    assert lean * 4 >= frames, "the lean bounce hardly ran"


def test_sequences_without_the_lean_bounce_and_without_culling_end_on_the_same_bits(rt, oracle):
    seeds = fuzz_seeds()
    bad = 0
    for seed in seeds:
        seq = ck.sequence(seed)
        after, last = oracle_sequence(oracle, seed, seq)
        for pinned in ((("camera_lean", 0),), (("cull", 0),)):
            counts = ck.lean_counts(seq, options=pinned)
            assert max(counts.values()) == 0
            lines, img, rng, cnt, n_lean = run_sequence(rt, seq, pinned=pinned, lean_counts=counts, who=f"sequence {seed} {dict(pinned)}")
            d = differences((img, rng, cnt), last, seq.W, seq.H, COUNTERS)
            if d:
                lines.append(f"sequence {seed} {dict(pinned)} at its end: " + "; ".join(d))
                print(lines[-1], flush=True)
            bad += len(lines)
    assert bad == 0, f"{bad} control runs of {len(seeds)} sequences differ (see the lines printed above)"


# ------------------------------------------------------------------------------------------------ far and limit cameras, standing

STAND_W, STAND_H, STAND_FRAMES, STAND_CHECK = 72, 44, 12, (1, 2, 6, 12)
_standing = {}


def standing_case(oracle, cam):
    """(scene, frames, {frame number: oracle image}) computed once per camera"""
    if cam.name not in _standing:
        rng = np.random.default_rng([ck.cameras().index(cam), 17, 20262])
        scene = ck.scene_around(rng, cam.fields, 300, spheres=True, env=True)
        g = ck.sc.GlibcRand(3)
        base = ck.sc.params_c2().replace(max_bounce=3, **cam.fields)
        frames = [base.replace(frames=k + 1, random=g.rand()) for k in range(STAND_FRAMES)]
        img, after = np.zeros((STAND_H, STAND_W, 4), np.float32), {}
        for k, p in enumerate(frames):
            oracle.render(scene, sf.shader_params(scene, p), img, threads=16)
            if k + 1 in STAND_CHECK:
                assert not np.isnan(img).any()
                after[k + 1] = img.copy()
        _standing[cam.name] = (scene, frames, after)
    return _standing[cam.name]


@pytest.mark.parametrize("cam", STANDING, ids=[c.name for c in STANDING])
def test_a_standing_far_or_limit_camera_reuses_its_bits_for_eleven_frames(cam, rt, oracle):
    scene, frames, after = standing_case(oracle, cam)
    accepted = ck.widening(ck.camera_words(cam.fields))[0]
    bad = []
    for cull in (1, 3):
        for lean in (0, 1):
            for waves in (1, 2):
                what = f"{cam.name} cull {cull} camera_lean {lean} scan_waves {waves}"
                ctx = rt.host.Context(STAND_W, STAND_H)
                for k, v in (("kernel", 4), ("cull", cull), ("camera_lean", lean), ("scan_waves", waves)):
                    ctx.set_option(k, v)
                ctx.upload_scene(scene)
                for k, p in enumerate(frames):
                    ctx.render(p)
                    if k + 1 in after:
                        d = differences((ctx.read_image(), None, None), (after[k + 1], None, None), STAND_W, STAND_H)
                        if d:
                            bad.append(f"{what} frame {k + 1}: " + "; ".join(d))
                            print(bad[-1], flush=True)
                n_lean = ctx.get_option("camera_lean_frames")
                ctx.close()
                assert n_lean == (STAND_FRAMES - 1 if lean and accepted else 0), f"{what}: {n_lean} lean frames"
    assert not bad, f"{len(bad)} read-outs differ from the oracle (see the lines printed above)"


def test_standing_cameras_split_as_documented():
    refused = {c.name for c in STANDING if not ck.widening(ck.camera_words(c.fields))[0]}
    assert refused == {"limit_0.25", "limit_above", "limit_neg_aperture_above", "far_5e5_x"} and len(STANDING) == 14


# ------------------------------------------------------------------------------------------------ a tile of a striped image

def test_a_sequence_as_rank_one_of_two(rt):
    seed = fuzz_seeds()[1]
    seq = ck.sequence(seed)
    tiling = dict(rank=1, world=2, strip_rows=8)
    probe = rt.host.Context(seq.W, seq.H, **tiling)
    rows = probe.global_rows()
    probe.close()
    n0 = (seq.W // 8 * 8) * int((rows < seq.H // 8 * 8).sum())
    assert 0 < n0 < ck.footprint(seq.W, seq.H)
    counts = ck.lean_counts(seq, n0=n0)
    assert max(counts.values()) >= 3
    lines_on, on, rng_on, _, lean_on = run_sequence(rt, seq, lean_counts=counts, who=f"sequence {seed} rank 1 of 2", **tiling)
    off_counts = ck.lean_counts(seq, n0=n0, options=(("camera_lean", 0),))
    lines_off, off, rng_off, _, lean_off = run_sequence(rt, seq, pinned=(("camera_lean", 0),), lean_counts=off_counts, who=f"sequence {seed} rank 1 of 2, camera_lean 0", **tiling)
    assert not lines_on and not lines_off, "\n".join(lines_on + lines_off)
    assert lean_off == 0 and on.any()
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    inside = rows < seq.H // 8 * 8                      # (outside the dispatch footprint the RNG buffer is never written)
    assert np.array_equal(rng_on[inside, :seq.W // 8 * 8], rng_off[inside, :seq.W // 8 * 8])
