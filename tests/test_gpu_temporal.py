"""rtgl_temporal_accumulate on the device (include/rtgl_amd.h, "temporal accumulation").

The reference is the numpy restatement, tests/temporal_mirror.py, pinned by tests/test_temporal_mirror.py.  The comparison rule (`check`, the
rule of tests/test_gpu_denoise_guided.py), for all four components of every call's history: where the mirror's component is not a NaN the
kernel's has the same bits, no tolerance; where it is a NaN, any NaN will do.  The mirror's NaN share is held to
temporal_inputs.nan_budget, so the rule cannot hide a failure.  Injected sequences, rendered sequences, the denoisers filtering the history,
the host path, the frame path left alone, and the point of it: closer to the converged image than a single frame."""
import ctypes as C
import math

import numpy as np
import pytest

import denoise_guided_mirror as gm
import denoise_mirror as dm
import golden_cases as gc
import raytracer_glsl_amd
import temporal_inputs as ti
import temporal_mirror as tm
from test_gpu_denoise import (ALBEDO, ALL, ERR_INVALID, ERR_STATE, GUIDES, IDS, MIRROR_CASES, NORMAL, POSITION, bits, differing, golden_path, named_case, same)
from test_gpu_denoise_guided import check as check_guided
from test_gpu_denoise_inputs import check as check_plain
from test_gpu_denoise_inputs import plane_tensor
from test_oracle_golden import load_case

pytestmark = pytest.mark.gpu

H_ = raytracer_glsl_amd.host


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


def check(got, want, budget, label):
    """got, want: one call's history"""
    check_guided((got,), (want,), budget, label)


def prepared(rt, W, H, aov=NORMAL | POSITION):
    """a context in the state the call asks for: the planes on and one frame of a trivial scene rendered (as tests/test_gpu_denoise_inputs.py)"""
    sc = rt.scenes
    ctx = rt.host.Context(W, H)
    ctx.set_aov(aov)
    ctx.upload_scene(sc.scene_mesh(10, 5, env_size=16))
    ctx.render(gc.frame_sequence(sc, sc.params_c2(), 1)[0])
    return ctx


def inject(ctx, image, normal, position):
    """put the arrays in front of the kernel (image through rtgl_write_image_f32, planes by host-to-device copies) and read them back"""
    import torch
    ctx.synchronize()
    ctx.write_image(np.ascontiguousarray(image, np.float32))
    aov = ctx.get_option("aov")
    for plane, a in ((NORMAL, normal), (POSITION, position)):
        if aov & plane:
            plane_tensor(ctx, plane).copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    torch.cuda.synchronize()
    assert same(ctx.read_image(), image) and same(ctx.read_aov(POSITION), position) and (not aov & NORMAL or same(ctx.read_aov(NORMAL), normal))


def look(rt, camera):
    return rt.scenes.params_c2().replace(**camera)


def step(rt, ctx, item, ps):
    image, normal, position, camera = item
    inject(ctx, image, normal, position)
    ctx.set_params(look(rt, camera))
    ctx.temporal_accumulate(**ps)
    return ctx.read_temporal()


def run_sequence(rt, ctx, seq, ps, label, budget=0.0):
    """the sequence from a reset on, every call's history against the mirror"""
    want = tm.run(seq, **ps)
    ctx.temporal_reset()
    for k, item in enumerate(seq):
        check(step(rt, ctx, item, ps), want[k], budget, f"{label} {ps} call {k}")
    image, normal, position, _ = seq[-1]
    assert same(ctx.read_image(), image) and same(ctx.read_aov(POSITION), position), f"{label}: the calls changed the image or a plane"


# ---------------------------------------------------------------------------------------------- 1. injected sequences

@pytest.mark.parametrize("size", ti.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", sorted(ti.FAMILIES))
def test_injected_sequences_are_bit_identical_to_the_mirror(family, size, rt):
    """every family (resting camera, translation, rotation, dolly through a depth step, all-miss, points behind the previous camera, a
    non-unit and slightly non-orthogonal basis, special values) x every parameter set, at the sizes about the 64 x 4 block tile"""
    W, H = size
    ctx = prepared(rt, W, H)
    seq = ti.make(family, H, W)
    for ps in ti.PARAMETER_SETS:
        run_sequence(rt, ctx, seq, ps, f"{family} {W} x {H}", ti.nan_budget(family))
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. rendered sequences

def moved(p, k):
    """the camera of p a little further along: displaced and turned about the vertical"""
    a = 0.02 * k
    f, r = np.array(p.camera_forward, np.float64), np.array(p.camera_right, np.float64)
    f2, r2 = f * math.cos(a) - r * math.sin(a), r * math.cos(a) + f * math.sin(a)
    pos = np.array(p.camera_position, np.float64) + 0.4 * k * r + 0.15 * k * np.array(p.camera_up, np.float64) + 0.5 * k * f
    t = lambda v: tuple(float(np.float32(x)) for x in v)
    return p.replace(camera_position=t(pos), camera_forward=t(f2), camera_right=t(r2))


def own_frames(rt, base, poses, seed=0):
    """one frame per pose, each the frame's own radiance: reset_flag = 1, frames = 0"""
    g = rt.scenes.GlibcRand(seed)
    return [moved(base, k).replace(reset_flag=1, frames=0, random=g.rand()) for k in poses]


def context_arrays(ctx):
    aov = ctx.get_option("aov")
    return ctx.read_image(), (ctx.read_aov(NORMAL) if aov & NORMAL else None), ctx.read_aov(POSITION)


@pytest.mark.parametrize("kernel", [0, 4])
@pytest.mark.parametrize("name", ["camera_moved", "mesh_env_dof", "c1_256"])
def test_rendered_sequences_are_bit_identical_to_the_mirror(name, kernel, rt):
    """six frames, the camera rests, moves, rests; the arrays are read from the context before each call"""
    case, scene, W, H = named_case(rt, name)
    ctx = rt.host.Context(W, H)
    ctx.set_option("kernel", kernel)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    state, lengths = None, []
    for k, p in enumerate(own_frames(rt, case["frames"][0], (0, 0, 1, 2, 2, 2))):
        ctx.render(p)
        arrays = context_arrays(ctx)
        ctx.temporal_accumulate()
        state = tm.accumulate(state, *arrays, p, **tm.DEFAULTS)
        got = ctx.read_temporal()
        check(got, state["H"], 0.0, f"{name}, kernel {kernel}, frame {k}")
        lengths.append(float(got[..., 3].mean()))
    ctx.close()
    assert lengths[0] == 1.0 and lengths[1] > 1.0 and lengths[5] > lengths[3] > 1.0, lengths


# ---------------------------------------------------------------------------------------------- 3. "denoise_source"

def test_denoisers_filter_the_history_when_asked(rt):
    case, scene, W, H = named_case(rt, "mesh_env_dof")
    ctx = rt.host.Context(W, H)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    assert ctx.get_option("denoise_source") == 0
    for bad in (2, -1):
        assert ctx.lib.rtgl_set_option(ctx.h, b"denoise_source", bad) == ERR_INVALID
    frames = own_frames(rt, case["frames"][0], (0, 1, 1))
    ctx.render(frames[0])
    ctx.set_option("denoise_source", 1)
    assert ctx.lib.rtgl_denoise(ctx.h, None) == ERR_STATE and b"rtgl_temporal_accumulate" in ctx.lib.rtgl_last_error(ctx.h)
    assert ctx.lib.rtgl_denoise_guided(ctx.h, None) == ERR_STATE
    ctx.set_option("denoise_source", 0)
    for p in frames:
        ctx.render(p)
        ctx.temporal_accumulate()
    image, albedo, normal, position = ctx.read_image(), ctx.read_aov(ALBEDO), ctx.read_aov(NORMAL), ctx.read_aov(POSITION)
    history = ctx.read_temporal()
    assert not same(history, image) and (history[..., 3] > 1).any()
    for source, src in ((1, history), (0, image), (1, history)):
        ctx.set_option("denoise_source", source)
        assert ctx.get_option("denoise_source") == source
        for ps in (dict(), dict(passes=2, demodulate=False), dict(passes=0, demodulate=False)):
            ctx.denoise(**ps)
            check_plain(ctx.read_denoised(), dm.denoise(src, albedo, normal, position, **dict(dm.DEFAULTS, **ps)), 0.0, f"rtgl_denoise, source {source}, {ps}")
        for ps in (dict(), dict(passes=1, firefly_ratio=0.0), dict(passes=0, demodulate=False)):
            ctx.denoise_guided(**ps)
            check_guided((ctx.read_denoised(), ctx.read_denoise_variance()), gm.denoise_guided(src, albedo, normal, position, **dict(gm.DEFAULTS, **ps)), 0.0,
                         f"rtgl_denoise_guided, source {source}, {ps}")
        if source:
            assert same(ctx.read_denoised()[..., 3], history[..., 3]), "the result's alpha is the history length"
    assert same(ctx.read_temporal(), history) and same(ctx.read_image(), image)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 4. host path

def raw_temporal(ctx, **fields):
    p = H_.CTemporalParams()
    assert ctx.lib.rtgl_temporal_defaults(C.byref(p)) == 0
    for k, v in fields.items():
        setattr(p, k, v)
    return ctx.lib.rtgl_temporal_accumulate(ctx.h, C.byref(p))


def test_errors(rt):
    sc = rt.scenes
    W, H = 64, 64
    scene = sc.scene_mesh(10, 5, env_size=16)
    frames = gc.frame_sequence(sc, sc.params_c2(), 4)
    buf = np.zeros((H, W, 4), np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    ctx = rt.host.Context(W, H)
    lib = ctx.lib
    ctx.upload_scene(scene)
    assert lib.rtgl_read_temporal_f32(ctx.h, ptr) == ERR_STATE and ctx.device_temporal_ptr() == 0
    ctx.render(frames[0])
    # planes missing
    assert lib.rtgl_temporal_accumulate(ctx.h, None) == ERR_STATE and b"aov" in lib.rtgl_last_error(ctx.h)
    ctx.set_aov(NORMAL | ALBEDO)
    ctx.render(frames[1])
    assert raw_temporal(ctx) == ERR_STATE and raw_temporal(ctx, sigma_normal=0.0, sigma_position=0.0) == ERR_STATE
    ctx.set_aov(POSITION | IDS)
    ctx.render(frames[1])
    assert raw_temporal(ctx) == ERR_STATE and b"normal" in lib.rtgl_last_error(ctx.h)
    assert lib.rtgl_read_temporal_f32(ctx.h, ptr) == ERR_STATE and ctx.device_temporal_ptr() == 0
    assert raw_temporal(ctx, sigma_normal=0.0) == 0
    assert lib.rtgl_read_temporal_f32(ctx.h, ptr) == 0 and ctx.device_temporal_ptr() != 0
    # no frame since the planes restarted: after the option was set, after rtgl_clear_image
    ctx.set_aov(NORMAL | POSITION)
    assert lib.rtgl_temporal_accumulate(ctx.h, None) == ERR_STATE and b"frame" in lib.rtgl_last_error(ctx.h)
    ctx.render(frames[2])
    assert lib.rtgl_temporal_accumulate(ctx.h, None) == 0
    ctx.clear_image()
    assert lib.rtgl_temporal_accumulate(ctx.h, None) == ERR_STATE
    ctx.render(frames[3])
    assert lib.rtgl_temporal_accumulate(ctx.h, None) == 0
    # bad parameters
    for field in ("max_history", "sigma_normal", "sigma_position"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert raw_temporal(ctx, **{field: bad}) == ERR_INVALID, (field, bad)
    for bad in (0.0, 0.999, -3.0):
        assert raw_temporal(ctx, max_history=bad) == ERR_INVALID
    assert raw_temporal(ctx, max_history=1.0, sigma_normal=-1.0, sigma_position=0.0) == 0
    assert raw_temporal(ctx, flags=1) == ERR_INVALID and raw_temporal(ctx, flags=1 << 31) == ERR_INVALID
    for k in range(4):
        r = [0, 0, 0, 0]
        r[k] = 1
        assert raw_temporal(ctx, reserved=(C.c_uint32 * 4)(*r)) == ERR_INVALID
    assert lib.rtgl_read_temporal_f32(ctx.h, None) == ERR_INVALID
    assert lib.rtgl_temporal_accumulate(None, None) == ERR_INVALID and lib.rtgl_temporal_reset(None) == ERR_INVALID
    with pytest.raises(rt.host.RtglError):
        ctx.temporal_accumulate(max_history=0.0)
    ctx.close()
    # tiled and multi-device contexts: out of scope, and the message says so
    for kw in (dict(rank=0, world=2, strip_rows=16), dict(devices=[0, 0], strip_rows=8)):
        ctx = rt.host.Context(W, H, **kw)
        ctx.set_aov(GUIDES)
        ctx.upload_scene(scene)
        ctx.render(frames[0])
        assert lib.rtgl_temporal_accumulate(ctx.h, None) == ERR_STATE and b"out of scope" in lib.rtgl_last_error(ctx.h), kw
        assert lib.rtgl_read_temporal_f32(ctx.h, ptr) == ERR_STATE and ctx.device_temporal_ptr() == 0
        ctx.close()


def test_first_call_pointer_turns_reset_and_the_normal_plane_switched_on(rt):
    import torch
    from test_gpu_denoise import _DeviceArray
    W, H = 70, 53
    seq = ti.make("translate", H, W)
    # the first call on a fresh context is not the default: no normal plane, its test off
    ctx = prepared(rt, W, H, aov=POSITION)
    ps = dict(sigma_normal=0.0)
    want = tm.run([(i, None, p, c) for i, _, p, c in seq[:2]], **ps)
    ptrs = []
    for k in range(2):
        check(step(rt, ctx, seq[k], ps), want[k], 0.0, f"no normal plane, call {k}")
        ptrs.append(ctx.device_temporal_ptr())
        t = torch.as_tensor(_DeviceArray(ptrs[-1], (H, W, 4), "<f4"), device="cuda:0")
        torch.cuda.synchronize()
        assert same(t.cpu().numpy(), want[k]), "the pointer does not name the latest result"
    assert ptrs[0] and ptrs[1] and ptrs[0] != ptrs[1]
    # the normal plane switched on between calls: this call needs Np, the previous one stored none: the history is dropped
    ctx.set_aov(NORMAL | POSITION)
    ctx.render(gc.frame_sequence(rt.scenes, rt.scenes.params_c2(), 1)[0])
    got = step(rt, ctx, seq[2], dict())
    assert (got[..., 3] == 1).all() and same(got[..., :3], seq[2][0][..., :3])
    assert ctx.device_temporal_ptr() == ptrs[0]
    check(step(rt, ctx, seq[3], dict()), tm.run(seq[2:4])[1], 0.0, "after the drop")
    assert ctx.device_temporal_ptr() == ptrs[1]
    # a reset in mid-sequence
    want = tm.run(seq[:2] + [tm.RESET] + seq[2:])
    ctx.temporal_reset()
    last = ctx.device_temporal_ptr()
    for k, item in enumerate(seq):
        if k == 2:
            before = ctx.read_temporal()
            ctx.temporal_reset()
            assert same(ctx.read_temporal(), before), "a reset leaves the latest buffer readable"
        check(step(rt, ctx, item, dict()), want[k], 0.0, f"reset in mid-sequence, call {k}")
        assert ctx.device_temporal_ptr() in ptrs and ctx.device_temporal_ptr() != last, "the two buffers do not take turns"
        last = ctx.device_temporal_ptr()
    ctx.close()


def test_two_live_contexts_take_turns(rt):
    a, b = prepared(rt, 70, 53), prepared(rt, 129, 9)
    sa, sb = ti.make("dolly", 53, 70), ti.make("rotate", 9, 129)
    wa, wb = tm.run(sa), tm.run(sb, max_history=2.5)
    for k in range(4):
        ga = step(rt, a, sa[k], dict())
        gb = step(rt, b, sb[k], dict(max_history=2.5))
        check(ga, wa[k], 0.0, f"context 70 x 53, call {k}")
        check(gb, wb[k], 0.0, f"context 129 x 9, call {k}")
        assert same(a.read_temporal(), ga)
    a.close()
    b.close()


def test_batching_and_the_headless_renderer(rt):
    sc = rt.scenes
    W, H = 72, 61
    scene = sc.scene_mesh(10, 5, env_size=16)
    base = sc.params_c2()
    # frame_batch set (with the planes on frames are rendered one by one; the call submits whatever is held back first)
    ctx = rt.host.Context(W, H)
    ctx.set_option("frame_batch", 8)
    ctx.set_aov(NORMAL | POSITION)
    ctx.upload_scene(scene)
    state = None
    for p in own_frames(rt, base, (0, 1, 1)):
        ctx.render(p, sync=False)
        ctx.temporal_accumulate()
        got = ctx.read_temporal()
        state = tm.accumulate(state, *context_arrays(ctx), p)
        check(got, state["H"], 0.0, "frame_batch 8")
    ctx.close()
    hr = rt.host.HeadlessRenderer(W, H, aov=NORMAL | POSITION)
    hr.set_scene(scene)
    hr.params = base
    state = None
    for _ in range(3):
        p = hr.render_frame()
        hr.temporal_accumulate(max_history=4.0)
        state = tm.accumulate(state, *context_arrays(hr.ctx), p, max_history=4.0)
    check(hr.read_temporal(), state["H"], 0.0, "headless")
    assert hr.device_temporal_ptr()
    hr.temporal_reset()
    hr.ctx.close()


# ---------------------------------------------------------------------------------------------- 5. nothing else changes

@pytest.mark.parametrize("name", MIRROR_CASES)
def test_the_frame_path_does_not_notice_the_calls(name, rt):
    """rtgl_temporal_accumulate and rtgl_temporal_reset between the frames of a golden case: the image stays the reference shader's, bit
    for bit; the RNG states, all four planes and the denoised buffer stay those of a run without the calls"""
    meta, scene, frames, expected = load_case(golden_path(name), rt)
    W, H = meta["width"], meta["height"]

    def run(calls):
        ctx = rt.host.Context(W, H)
        ctx.set_option("rng_state", 1)
        ctx.set_aov(ALL)
        ctx.upload_scene(scene)
        ctx.write_image(gc.initial_image(meta["init"], W, H))
        denoised = None
        for k, p in enumerate(frames):
            ctx.render(p, sync=False)
            if k == 0:
                ctx.denoise_guided()
            if calls:
                ctx.temporal_accumulate()
                ctx.temporal_accumulate(max_history=2.0, sigma_normal=0.0)
                if k % 2:
                    ctx.temporal_reset()
        out = dict(img=ctx.read_image(), seeds=ctx.read_rng_state(), planes={p: ctx.read_aov(p) for p in (ALBEDO, NORMAL, POSITION, IDS)},
                   denoised=ctx.read_denoised(), variance=ctx.read_denoise_variance())
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


# ---------------------------------------------------------------------------------------------- 6. it helps

def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def test_c1_256_history_is_closer_to_the_converged_image_than_a_frame(rt):
    """c1_256 at 256 x 256: the camera dollies a little each frame for 8 frames and then rests at the last pose for 4.  Reference: 256
    accumulated frames of a fresh context at that pose, times 257 / 256 (the running mean divides frame n by frames + 1: DESIGN.md 5.4;
    a frame rendered with reset_flag = 1, frames = 0 has no such factor).  RMSE(history) < RMSE(last single frame), strictly, no factor;
    the figures are printed, with those of rtgl_denoise_guided over the history and over the single frame."""
    case, scene, W, H = named_case(rt, "c1_256")
    base = case["frames"][0]
    g = rt.scenes.GlibcRand(0)

    def pose(k):
        f = np.array(base.camera_forward, np.float64)
        return tuple(float(np.float32(x)) for x in np.array(base.camera_position, np.float64) + 0.25 * k * f)

    ctx = rt.host.Context(W, H)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    for k in list(range(1, 9)) + [8] * 4:
        ctx.render(base.replace(camera_position=pose(k), reset_flag=1, frames=0, random=g.rand()), sync=False)
        ctx.temporal_accumulate()
    frame, history = ctx.read_image(), ctx.read_temporal()
    ctx.denoise_guided()
    frame_dn = ctx.read_denoised()
    ctx.set_option("denoise_source", 1)
    ctx.denoise_guided()
    history_dn = ctx.read_denoised()
    ctx.close()
    ref = rt.host.Context(W, H)
    ref.upload_scene(scene)
    for n in range(1, 257):
        ref.render(base.replace(camera_position=pose(8), frames=n, random=g.rand()), sync=False)
    target = ref.read_image().astype(np.float64) * (257.0 / 256.0)
    ref.close()
    assert np.isfinite(target).all() and np.isfinite(history).all() and np.isfinite(frame).all()
    e_frame, e_hist, e_frame_dn, e_hist_dn = (rmse(i, target) for i in (frame, history, frame_dn, history_dn))
    print(f"c1_256, 8 dolly frames + 4 at rest: RMSE single frame {e_frame:.5f}, history {e_hist:.5f} (ratio {e_hist / e_frame:.4f}); "
          f"rtgl_denoise_guided of the frame {e_frame_dn:.5f}, of the history {e_hist_dn:.5f} (ratio {e_hist_dn / e_frame_dn:.4f}); "
          f"mean history length {float(history[..., 3].mean()):.2f}")
    assert e_hist < e_frame
