"""rtgl_error_estimate on the device (include/rtgl_amd.h, "error estimate").

The reference is the numpy restatement, tests/error_mirror.py, pinned by tests/test_error_mirror.py.  No output can be a NaN, so the
comparison is exact and has no budget: the bits of the summary and every tile record."""
import ctypes as C

import numpy as np
import pytest

import error_inputs as ei
import error_mirror as em
import golden_cases as gc
from test_gpu_denoise import ALBEDO, ALL, IDS, MIRROR_CASES, NORMAL, POSITION, differing, golden_path, same
from test_oracle_golden import load_case

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


class _DeviceArray:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}


def prepared(rt, w, h, **kw):
    """a context that can render a trivial frame: the four spheres, one bounce"""
    ctx = rt.host.Context(w, h, **kw)
    ctx.upload_scene(rt.scenes.scene_c1(False))
    return ctx


def put(rt, ctx, image, frames):
    """Put `image` in front of the kernel as the accumulation image after a frame rendered with u_frames = `frames`: render a trivial frame
    with that count, then copy the array over the image through rtgl_device_image (rtgl_write_image_f32 would drop the snapshot), and read
    it back: a case cannot silently run on other data."""
    import torch
    ctx.render(rt.scenes.params_c1().replace(frames=int(frames), max_bounce=1))
    ptr = ctx.device_image_ptr()
    assert ptr
    image = np.ascontiguousarray(image, np.float32)
    torch.as_tensor(_DeviceArray(ptr, image.shape, "<f4"), device="cuda:0").copy_(torch.from_numpy(image))
    torch.cuda.synchronize()
    assert same(ctx.read_image(), image)


def result(ctx):
    out = ctx.read_error_summary()
    out["tiles"] = ctx.read_error_tiles()
    return out


def check(ctx, want, label):
    got = result(ctx)
    bad = em.same_result(got, want)
    if bad:
        detail = {k: (got[k], want[k]) for k in bad if k != "tiles"}
        if "tiles" in bad and got["tiles"].shape == want["tiles"].shape:
            at = np.argwhere(got["tiles"].view(np.uint32).reshape(got["tiles"].shape + (4,)) != want["tiles"].view(np.uint32).reshape(want["tiles"].shape + (4,)))
            detail["tiles"] = f"{len(at)} words differ, first in tile (row, column) {tuple(at[0][:2])}: device {got['tiles'][tuple(at[0][:2])]}, mirror {want['tiles'][tuple(at[0][:2])]}"
        raise AssertionError(f"{label}: {detail}")
    assert not np.isnan(got["tiles"]["sum"]).any() and not np.isnan(got["tiles"]["mse"]).any()
    return got


def run_steps(rt, ctx, steps, label):
    """a family's steps on the context against the mirror's Estimator, from a dropped snapshot"""
    ctx.error_reset()
    est = em.Estimator()
    for k, s in enumerate(steps):
        put(rt, ctx, s["image"], s["frames"])
        ctx.error_estimate(**s["params"])
        est.frame(s["frames"])
        with np.errstate(all="ignore"):
            want = est(s["image"], **s["params"])
        check(ctx, want, f"{label}, call {k}")
        assert same(ctx.read_image(), s["image"]), f"{label}: the call changed the image"


# ---------------------------------------------------------------------------------------------- 1. bit-identical to the mirror

@pytest.mark.parametrize("size", ei.SIZES, ids=[f"{w}x{h}" for h, w in ei.SIZES])
def test_every_family_is_bit_identical_to_the_mirror(size, rt):
    h, w = size
    ctx = prepared(rt, w, h)
    for name in ei.FAMILIES:
        run_steps(rt, ctx, ei.family(name, h, w), f"{name} {w} x {h}")
    assert result(ctx)["tiles"].shape == ((h + 15) // 16, (w + 15) // 16)
    ctx.close()


def test_a_1080p_pair(rt):
    """8,160 tiles: the solve's strided loop runs 32 times; the last tile row holds 8 footprint rows"""
    h, w = ei.FULL
    steps = ei.gaussian_steps(h, w, (16, 32), 1, seed=7)
    steps[1]["image"][5:9, 100:300, :3] = np.nan
    steps[1]["image"][700, ::3, 1] = np.inf
    ctx = prepared(rt, w, h)
    run_steps(rt, ctx, steps, "1080p")
    got = result(ctx)
    assert got["tiles_valid"] == 68 * 120 and got["pixels_ignored"] == 4 * 200 + 640
    ctx.close()


def test_a_rendered_sequence_against_the_mirror_fed_with_the_contexts_own_images(rt):
    """c1 at 64 x 64, the reference's loop (frames 1, 2, ...): estimates at 16, 32 and 48 (both keeping the snapshot of 16), 64 and 80"""
    sc = rt.scenes
    ctx = rt.host.Context(64, 64)
    ctx.upload_scene(sc.scene_c1(False))
    est, seen = em.Estimator(), []
    calls = {16: dict(), 32: dict(keep_snapshot=True), 48: dict(keep_snapshot=True, threshold=0.1), 64: dict(), 80: dict(quantile_permille=500)}
    for p in gc.frame_sequence(sc, sc.params_c1(), 80):
        ctx.render(p, sync=False)
        est.frame(p.frames, p.reset_flag)
        if p.frames in calls:
            ctx.error_estimate(**calls[p.frames])
            seen.append(check(ctx, est(ctx.read_image(), **calls[p.frames]), f"frame {p.frames}"))
    assert [(s["valid"], s["frames_now"], s["frames_snapshot"]) for s in seen] == [(0, 0, 0), (1, 32, 16), (1, 48, 16), (1, 64, 16), (1, 80, 64)]
    assert all(s["tiles_valid"] == 16 and s["pixels_ignored"] == 0 and 0 < s["mse"] < 0.01 for s in seen[1:])
    assert seen[3]["mse"] < seen[1]["mse"]                              # 64 frames are cleaner than 32
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. the snapshot rules, through the entry points

def test_every_dropping_event_through_the_real_entry_points(rt):
    import torch
    h, w = 24, 40
    n_list = tuple(range(8, 8 * 24, 8))
    img = dict(zip(n_list, (s["image"] for s in ei.gaussian_steps(h, w, n_list, 1, seed=11))))
    ctx = prepared(rt, w, h)
    est = em.Estimator()
    own = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")

    def call(F, **params):
        put(rt, ctx, img[F], F)
        est.frame(F)
        ctx.error_estimate(**params)
        return check(ctx, est(img[F], **params), f"frame {F} {params}")

    assert call(8)["valid"] == 0 and call(16)["valid"] == 1
    F = 16
    events = [("rtgl_error_reset", ctx.error_reset), ("rtgl_clear_image", ctx.clear_image), ("rtgl_write_image_f32", lambda: ctx.write_image(img[8])),
              ("rtgl_bind_device_image", lambda: ctx.bind_device_image(own.data_ptr())), ("rtgl_bind_device_image(NULL)", lambda: ctx.bind_device_image(0))]
    for name, event in events:
        event()
        est.drop()
        F += 8
        assert call(F)["valid"] == 0, name                              # a first call again
        F += 8
        assert call(F)["valid"] == 1, name
    # a rendered frame with reset_flag != 0
    ctx.render(rt.scenes.params_c1().replace(frames=F + 1, max_bounce=1, reset_flag=1))
    est.frame(F + 1, reset_flag=1)
    F += 8
    assert call(F)["valid"] == 0
    F += 8
    assert call(F)["valid"] == 1
    # a call that is not later than the snapshot, and one that counts the frames differently
    assert call(F)["valid"] == 0
    assert call(F - 8)["valid"] == 0
    assert call(F, first_frames=0)["valid"] == 0
    got = call(F + 8, first_frames=0)
    assert got["valid"] == 1 and got["frames_snapshot"] == F
    # the keep flag without a snapshot takes one; with one it leaves it
    ctx.error_reset()
    est.drop()
    assert call(F + 16, keep_snapshot=True)["valid"] == 0
    assert call(F + 24, keep_snapshot=True)["frames_snapshot"] == F + 16
    assert call(F + 32)["frames_snapshot"] == F + 16
    assert call(F + 40)["frames_snapshot"] == F + 32
    ctx.close()


def test_two_live_contexts_taking_turns(rt):
    h, w = 53, 70
    a_steps, b_steps = ei.gaussian_steps(h, w, (8, 16, 24, 32), 1, seed=21), ei.gaussian_steps(h, w, (4, 20, 36, 52), 0, seed=22, threshold=0.1)
    a, b = prepared(rt, w, h), prepared(rt, w, h)
    ea, eb = em.Estimator(), em.Estimator()
    for k in range(4):
        for ctx, est, s in ((a, ea, a_steps[k]), (b, eb, b_steps[k])):
            put(rt, ctx, s["image"], s["frames"])
            ctx.error_estimate(**s["params"])
            est.frame(s["frames"])
        for ctx, est, s, label in ((a, ea, a_steps[k], "a"), (b, eb, b_steps[k], "b")):     # read after both have been enqueued
            check(ctx, est(s["image"], **s["params"]), f"context {label}, call {k}")
    assert a.device_error_tiles_ptr() and a.device_error_tiles_ptr() != b.device_error_tiles_ptr()
    a.close()
    b.close()


def test_frames_held_by_a_batching_context_are_submitted_first(rt):
    """frame_batch = 8 on a scene with triangles: the estimates at frames 12 and 26 fall inside a batch; summaries and tile records equal
    those of a context that renders frame by frame, and the mirror fed with that context's images"""
    sc = rt.scenes
    scene, frames = sc.scene_mesh(10, 5, env_size=16), gc.frame_sequence(sc, sc.params_c2(), 26)

    def run(batch):
        ctx = rt.host.Context(96, 64)
        ctx.set_option("frame_batch", batch)
        ctx.upload_scene(scene)
        out = []
        for p in frames:
            ctx.render(p, sync=False)
            if p.frames in (12, 26):
                ctx.error_estimate()
                out.append((result(ctx), ctx.read_image()))
        ctx.close()
        return out

    batched, plain = run(8), run(1)
    est = em.Estimator()
    for (got, img), (want, img1), F in zip(batched, plain, (12, 26)):
        assert same(img, img1)
        assert em.same_result(got, want) == [], F
        est.frame(F)
        assert em.same_result(got, est(img1)) == [], F
    assert (batched[1][0]["valid"], batched[1][0]["frames_now"], batched[1][0]["frames_snapshot"]) == (1, 26, 12)


# ---------------------------------------------------------------------------------------------- 3. render until the picture is this clean

def test_render_until(rt):
    sc = rt.scenes

    def run(threshold, max_frames, **kw):
        r = rt.host.HeadlessRenderer(64, 64)
        r.params = sc.params_c1()
        r.set_scene(sc.scene_c1(False))
        frames, summary = r.render_until(threshold, max_frames, **kw)
        img = r.ctx.read_image()
        r.ctx.close()
        return frames, summary, img

    loose, tight = run(0.08, 512), run(0.04, 512)
    print(f"render_until at 64 x 64: threshold 0.08 stops after {loose[0]} frames (mse {float(loose[1]['mse']):.3g}), 0.04 after {tight[0]} (mse {float(tight[1]['mse']):.3g})")
    assert loose[1]["converged"] == 1 and loose[0] % 16 == 0 and 32 <= loose[0] < 512
    assert loose[0] <= tight[0]                                         # a looser threshold stops no later
    assert loose[1]["frames_now"] == loose[0] and loose[1]["frames_snapshot"] == loose[0] - 16
    frames, summary, _ = run(1e-6, 40, check_every=16)                  # unreachable: runs to max_frames, the last round is 8 frames
    assert frames == 40 and summary["valid"] == 1 and summary["converged"] == 0 and (summary["frames_now"], summary["frames_snapshot"]) == (40, 32)
    frames, summary, _ = run(0.08, 10, check_every=16)                  # too few frames for two moments: a snapshot, no estimate
    assert frames == 10 and summary["valid"] == 0


# ---------------------------------------------------------------------------------------------- 4. nothing else changes

@pytest.mark.parametrize("name", MIRROR_CASES)
def test_the_frame_path_does_not_notice_the_calls(name, rt):
    """rtgl_error_estimate and rtgl_error_reset between the frames of a golden case: the image stays the reference shader's, bit for bit;
    the RNG states, all four planes, the denoised, the variance and the display buffer stay those of a run without the calls"""
    meta, scene, frames, expected = load_case(golden_path(name), rt)
    W, H = meta["width"], meta["height"]

    def run(calls):
        ctx = rt.host.Context(W, H)
        ctx.set_option("rng_state", 1)
        ctx.set_aov(ALL)
        ctx.upload_scene(scene)
        ctx.write_image(gc.initial_image(meta["init"], W, H))
        for k, p in enumerate(frames):
            ctx.render(p, sync=False)
            if k == 0:
                ctx.denoise_guided()
                ctx.tonemap()
            if calls:
                ctx.error_estimate(first_frames=min(p.frames, 1))
                ctx.error_estimate(keep_snapshot=True, first_frames=min(p.frames, 1))
                if k == 0:
                    ctx.error_reset()
        if calls:
            assert ctx.read_error_summary()["valid"] in (0, 1) and ctx.read_error_tiles().shape == ((H + 15) // 16, (W + 15) // 16)
        out = dict(img=ctx.read_image(), seeds=ctx.read_rng_state(), planes={p: ctx.read_aov(p) for p in (ALBEDO, NORMAL, POSITION, IDS)},
                   denoised=ctx.read_denoised(), variance=ctx.read_denoise_variance(), display=ctx.read_display())
        ctx.close()
        return out

    with_calls, without = run(True), run(False)
    assert same(with_calls["img"], expected), differing(with_calls["img"], expected)
    assert same(without["img"], expected)
    fh, fw = H // 8 * 8, W // 8 * 8                      # (outside the dispatch footprint the RNG buffer is never written)
    assert (with_calls["seeds"][:fh, :fw] == without["seeds"][:fh, :fw]).all()
    for p in (ALBEDO, NORMAL, POSITION, IDS):
        assert same(with_calls["planes"][p], without["planes"][p]), f"plane {p}"
    assert same(with_calls["denoised"], without["denoised"]) and same(with_calls["variance"], without["variance"])
    assert (with_calls["display"] == without["display"]).all()


# ---------------------------------------------------------------------------------------------- 5. errors

def test_state_and_argument_errors_on_a_live_context(rt):
    H_ = rt.host
    lib = H_.load_library()
    ctx = prepared(rt, 16, 16)
    s, tiles, tx, ty = H_.CErrorSummary(), (C.c_uint32 * 4)(), C.c_uint32(), C.c_uint32()
    assert lib.rtgl_error_estimate(ctx.h, None) == ERR_STATE and b"no frame" in lib.rtgl_last_error(ctx.h)
    assert lib.rtgl_read_error_summary(ctx.h, C.byref(s)) == ERR_STATE
    assert lib.rtgl_read_error_tiles(ctx.h, tiles, C.byref(tx), C.byref(ty)) == ERR_STATE
    assert ctx.device_error_tiles_ptr() == 0
    assert lib.rtgl_error_reset(ctx.h) == 0
    ctx.render(rt.scenes.params_c1().replace(frames=3, max_bounce=1))
    p = H_.CErrorParams()
    lib.rtgl_error_defaults(C.byref(p))
    for field, value in (("threshold", 0.0), ("threshold", float("nan")), ("floor", float("inf")), ("floor", -1.0), ("quantile_permille", 0),
                         ("quantile_permille", 1001), ("first_frames", -1), ("first_frames", 5), ("flags", 2)):
        q = H_.CErrorParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert lib.rtgl_error_estimate(ctx.h, C.byref(q)) == ERR_INVALID, field      # (first_frames 5 > frames + 1: the image would hold no frame)
    q = H_.CErrorParams.from_buffer_copy(p)
    q.reserved[1] = 1
    assert lib.rtgl_error_estimate(ctx.h, C.byref(q)) == ERR_INVALID
    assert lib.rtgl_read_error_summary(ctx.h, C.byref(s)) == ERR_STATE                # none of them counted as a call
    assert lib.rtgl_error_estimate(ctx.h, None) == 0                                  # NULL: the defaults
    assert lib.rtgl_read_error_summary(ctx.h, None) == ERR_INVALID
    assert lib.rtgl_read_error_tiles(ctx.h, None, C.byref(tx), C.byref(ty)) == ERR_INVALID
    assert lib.rtgl_read_error_tiles(ctx.h, tiles, None, None) == 0                   # tx and ty may be NULL
    assert lib.rtgl_read_error_tiles(ctx.h, tiles, C.byref(tx), C.byref(ty)) == 0 and (tx.value, ty.value) == (1, 1)
    assert lib.rtgl_read_error_summary(ctx.h, C.byref(s)) == 0 and s.valid == 0
    ctx.close()
    # tiled and multi-device contexts: out of scope, and the message says so
    for kw in (dict(rank=0, world=2, strip_rows=16), dict(devices=[0, 0], strip_rows=8)):
        ctx = prepared(rt, 32, 32, **kw)
        ctx.render(rt.scenes.params_c1().replace(frames=1, max_bounce=1))
        assert lib.rtgl_error_estimate(ctx.h, None) == ERR_STATE and b"out of scope" in lib.rtgl_last_error(ctx.h), kw
        assert lib.rtgl_read_error_summary(ctx.h, C.byref(s)) == ERR_STATE and ctx.device_error_tiles_ptr() == 0
        ctx.close()
