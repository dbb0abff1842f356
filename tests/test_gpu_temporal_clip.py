"""rtgl_temporal_clip on the device (include/rtgl_amd.h, "temporal clip").

The reference is the numpy restatement, tests/temporal_clip_mirror.py, pinned by tests/test_temporal_clip_mirror.py.  The comparison rule is
that of tests/test_gpu_temporal.py (`check`): where the mirror's component is not a NaN the kernel's has the same bits, no tolerance; where
it is a NaN, any NaN will do.  The mirror's NaN share is held to temporal_clip_inputs.nan_budget, so the rule cannot hide a failure.
Injected sequences, rendered sequences, the denoisers filtering the clipped history, the host path, the frame path left alone, and the
point of it: after a change of lighting the clipped history is closer to the new converged image than the unclipped one."""
import ctypes as C

import numpy as np
import pytest

import denoise_guided_mirror as gm
import denoise_mirror as dm
import golden_cases as gc
import raytracer_glsl_amd
import temporal_clip_inputs as ci
import temporal_clip_mirror as cm
import temporal_mirror as tm
import temporal_moments_mirror as mm
from test_gpu_denoise import ALBEDO, ALL, ERR_INVALID, ERR_STATE, GUIDES, IDS, MIRROR_CASES, NORMAL, POSITION, bits, differing, golden_path, named_case, same
from test_gpu_denoise_guided import check as check_guided
from test_gpu_denoise_inputs import check as check_plain
from test_gpu_denoise_inputs import inject, prepared
from test_gpu_temporal import look, own_frames
from test_gpu_temporal_moments import check
from test_oracle_golden import load_case

pytestmark = pytest.mark.gpu

H_ = raytracer_glsl_amd.host


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


_sequences = {}


def sequence(family, size):
    """the family's arrays and the window sums the mirror has taken of them so far, shared by the cases of this module"""
    key = (family, size)
    if key not in _sequences:
        _sequences[key] = (ci.make(family, size[1], size[0]), {})
    return _sequences[key]


def moments_of(ctx):
    return ctx.read_temporal_moments() if ctx.get_option("temporal_moments") else None


def identical(a, b):
    """two read-outs of the device hold the same bits, NaN payloads included"""
    return (a is None and b is None) or same(a, b)


# ---------------------------------------------------------------------------------------------- 1. injected sequences

def run_sequence(rt, ctx, seq, cache, ps, mode, label, budget):
    """from a reset on, per frame: accumulate, clip, clip again; the history and the moments after each against the mirror"""
    want = cm.run(seq, mode, ps, cache)
    ctx.set_option("temporal_moments", mode)
    ctx.temporal_reset()
    for k, item in enumerate(seq):
        image, normal, position, camera, albedo = item
        inject(ctx, image, albedo, normal, position)
        ctx.set_params(look(rt, camera))
        ctx.temporal_accumulate()
        h0, m0 = ctx.read_temporal(), moments_of(ctx)
        H0, H1, M0, M1 = want[k]
        check(h0, H0, budget, f"{label} call {k}: history before the clip")
        ctx.temporal_clip(**ps)
        h1, m1 = ctx.read_temporal(), moments_of(ctx)
        check(h1, H1, budget, f"{label} call {k}: clipped history")
        if mode:
            check(m1[..., 3], M1[..., 3], budget, f"{label} call {k}: the moments' length")
            assert same(m1[..., :3], m0[..., :3]), f"{label} call {k}: m1, m2 or v changed"
            if budget == 0.0:
                check(m1, M1, 0.0, f"{label} call {k}: moments")
        ctx.temporal_clip(**ps)
        assert identical(ctx.read_temporal(), h1) and identical(moments_of(ctx), m1), f"{label} call {k}: a second clip is not the identity"
    image, normal, position, _, albedo = seq[-1]
    assert same(ctx.read_image(), image) and same(ctx.read_aov(POSITION), position) and same(ctx.read_aov(NORMAL), normal) and same(ctx.read_aov(ALBEDO), albedo), \
        f"{label}: the calls changed the image or a plane"


# one case per family and size with all three modes in it; above 10,000 pixels, where the mirror takes seconds, one case per mode
INJECTED = [(f, size, modes) for f in sorted(ci.FAMILIES) for size in ci.SIZES
            for modes in ([[m] for m in ci.MODES] if size[0] * size[1] > 10000 else [list(ci.MODES)])]


@pytest.mark.parametrize("family,size,modes", INJECTED, ids=[f"{f}-{s[0]}x{s[1]}" + ("" if len(m) > 1 else f"-mode{m[0]}") for f, s, m in INJECTED])
def test_injected_sequences_are_bit_identical_to_the_mirror(family, size, modes, rt):
    """every family (those of rtgl_temporal_accumulate, special values included, and relit, flat, edge and narrow-lens ones) x every
    parameter set x option "temporal_moments" 0, 1, 2, at the sizes about the 64 x 4 tile with its halo of 3"""
    W, H = size
    ctx = prepared(rt, W, H)
    seq, cache = sequence(family, size)
    for ps in ci.PARAMETER_SETS:
        for mode in modes:
            assert (family, size, ps, mode) in ci.listed_cases()
            run_sequence(rt, ctx, seq, cache, ps, mode, f"{family} {W} x {H} {ps} mode {mode}", ci.nan_budget(family))
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. rendered sequences

def context_arrays(ctx):
    return ctx.read_image(), ctx.read_aov(NORMAL), ctx.read_aov(POSITION)


@pytest.mark.parametrize("kernel", [0, 4])
@pytest.mark.parametrize("name", ["camera_moved", "c1_256"])
def test_rendered_sequences_are_bit_identical_to_the_mirror(name, kernel, rt):
    """six frames, the camera rests, moves, rests; the arrays are read from the context before each call, the mirror's next accumulation
    reprojects the mirror's clipped history"""
    case, scene, W, H = named_case(rt, name)
    ctx = rt.host.Context(W, H)
    ctx.set_option("kernel", kernel)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    state, touched = None, 0
    for k, p in enumerate(own_frames(rt, case["frames"][0], (0, 0, 1, 2, 2, 2))):
        ctx.render(p)
        arrays = context_arrays(ctx)
        ctx.temporal_accumulate()
        state = tm.accumulate(state, *arrays, p, **tm.DEFAULTS)
        check(ctx.read_temporal(), state["H"], 0.0, f"{name}, kernel {kernel}, frame {k}: history before the clip")
        ctx.temporal_clip()
        clipped, _ = cm.clip(state["H"], None, *arrays)
        touched += int((bits(clipped) != bits(state["H"])).any(-1).sum())
        state = dict(state, H=clipped)
        check(ctx.read_temporal(), clipped, 0.0, f"{name}, kernel {kernel}, frame {k}: clipped history")
        assert all(same(a, b) for a, b in zip(context_arrays(ctx), arrays)), "the call changed the image or a plane"
    ctx.close()
    assert touched > 0, "the clip never acted"


# ---------------------------------------------------------------------------------------------- 3. "denoise_source"

def test_denoisers_filter_the_clipped_history(rt):
    case, scene, W, H = named_case(rt, "mesh_env_dof")
    ctx = rt.host.Context(W, H)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    state = None
    for p in own_frames(rt, case["frames"][0], (0, 1, 1)):
        ctx.render(p)
        arrays = context_arrays(ctx)
        ctx.temporal_accumulate()
        ctx.temporal_clip(sigma_scale=1.0)
        state = tm.accumulate(state, *arrays, p, **tm.DEFAULTS)
        before = state["H"]
        state = dict(state, H=cm.clip(before, None, *arrays, sigma_scale=1.0)[0])
    history, albedo = state["H"], ctx.read_aov(ALBEDO)
    image, normal, position = arrays
    assert not same(history, before), "the clip did not act: the case shows nothing"
    check(ctx.read_temporal(), history, 0.0, "clipped history")
    ctx.set_option("denoise_source", 1)
    for ps in (dict(), dict(passes=2, demodulate=False), dict(passes=0, demodulate=False)):
        ctx.denoise(**ps)
        check_plain(ctx.read_denoised(), dm.denoise(history, albedo, normal, position, **dict(dm.DEFAULTS, **ps)), 0.0, f"rtgl_denoise over the clipped history, {ps}")
    for ps in (dict(), dict(passes=1, firefly_ratio=0.0), dict(passes=0, demodulate=False)):
        ctx.denoise_guided(**ps)
        check_guided((ctx.read_denoised(), ctx.read_denoise_variance()), gm.denoise_guided(history, albedo, normal, position, **dict(gm.DEFAULTS, **ps)), 0.0,
                     f"rtgl_denoise_guided over the clipped history, {ps}")
    assert same(ctx.read_denoised()[..., 3], history[..., 3]), "the result's alpha is the clipped history length"
    assert same(ctx.read_temporal(), history) and same(ctx.read_image(), image)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 4. host path

def raw_clip(ctx, **fields):
    p = H_.CTemporalClipParams()
    assert ctx.lib.rtgl_temporal_clip_defaults(C.byref(p)) == 0
    for k, v in fields.items():
        setattr(p, k, v)
    return ctx.lib.rtgl_temporal_clip(ctx.h, C.byref(p))


def test_errors(rt):
    sc = rt.scenes
    W, H = 64, 64
    scene = sc.scene_mesh(10, 5, env_size=16)
    frames = gc.frame_sequence(sc, sc.params_c2(), 5)
    ctx = rt.host.Context(W, H)
    lib = ctx.lib
    ctx.upload_scene(scene)
    ctx.set_aov(NORMAL | POSITION)
    ctx.render(frames[0])
    # no history yet
    assert lib.rtgl_temporal_clip(ctx.h, None) == ERR_STATE and b"rtgl_temporal_accumulate" in lib.rtgl_last_error(ctx.h)
    ctx.temporal_accumulate()
    assert lib.rtgl_temporal_clip(ctx.h, None) == 0
    # planes missing: the position plane always (the kind test), the normal plane for its term
    ctx.set_aov(NORMAL | ALBEDO)
    ctx.render(frames[1])
    assert raw_clip(ctx) == ERR_STATE and b"aov" in lib.rtgl_last_error(ctx.h)
    assert raw_clip(ctx, sigma_normal=0.0, sigma_position=0.0) == ERR_STATE
    ctx.set_aov(POSITION | IDS)
    ctx.render(frames[1])
    assert raw_clip(ctx) == ERR_STATE and b"normal" in lib.rtgl_last_error(ctx.h)
    assert raw_clip(ctx, sigma_normal=0.0) == 0
    # no frame since the planes restarted: after the option was set, after rtgl_clear_image
    ctx.set_aov(NORMAL | POSITION)
    assert lib.rtgl_temporal_clip(ctx.h, None) == ERR_STATE and b"frame" in lib.rtgl_last_error(ctx.h)
    ctx.render(frames[2])
    assert lib.rtgl_temporal_clip(ctx.h, None) == 0
    ctx.clear_image()
    assert lib.rtgl_temporal_clip(ctx.h, None) == ERR_STATE
    ctx.render(frames[3])
    assert lib.rtgl_temporal_clip(ctx.h, None) == 0
    # bad parameters
    for field in ("sigma_scale", "clip_history", "sigma_normal", "sigma_position"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert raw_clip(ctx, **{field: bad}) == ERR_INVALID, (field, bad)
    for bad in (0.0, -0.0, -2.0):
        assert raw_clip(ctx, sigma_scale=bad) == ERR_INVALID
    for bad in (0.0, 0.999, -3.0):
        assert raw_clip(ctx, clip_history=bad) == ERR_INVALID
    assert raw_clip(ctx, sigma_scale=1e-3, clip_history=1.0, sigma_normal=-1.0, sigma_position=0.0) == 0
    assert raw_clip(ctx, flags=1) == ERR_INVALID and raw_clip(ctx, flags=1 << 31) == ERR_INVALID
    for k in range(3):
        r = [0, 0, 0]
        r[k] = 1
        assert raw_clip(ctx, reserved=(C.c_uint32 * 3)(*r)) == ERR_INVALID
    assert lib.rtgl_temporal_clip(None, None) == ERR_INVALID
    with pytest.raises(rt.host.RtglError):
        ctx.temporal_clip(sigma_scale=0.0)
    ctx.close()
    # tiled and multi-device contexts: out of scope, and the message says so
    for kw in (dict(rank=0, world=2, strip_rows=16), dict(devices=[0, 0], strip_rows=8)):
        ctx = rt.host.Context(W, H, **kw)
        ctx.set_aov(GUIDES)
        ctx.upload_scene(scene)
        ctx.render(frames[0])
        assert lib.rtgl_temporal_clip(ctx.h, None) == ERR_STATE and b"out of scope" in lib.rtgl_last_error(ctx.h), kw
        ctx.close()


def test_keyword_arguments_batching_and_the_headless_renderer(rt):
    sc = rt.scenes
    W, H = 72, 61
    scene = sc.scene_mesh(10, 5, env_size=16)
    base = sc.params_c2()
    ps = dict(sigma_scale=0.75, clip_history=2.0, sigma_normal=0.2, sigma_position=0.1)
    # frame_batch set: the call submits whatever is held back first; option "temporal_moments" on: the length goes to both records
    ctx = rt.host.Context(W, H)
    ctx.set_option("frame_batch", 8)
    ctx.set_option("temporal_moments", 1)
    ctx.set_aov(NORMAL | POSITION)
    ctx.upload_scene(scene)
    state = None
    for p in own_frames(rt, base, (0, 1, 1)):
        ctx.render(p, sync=False)
        ctx.temporal_accumulate()
        ctx.temporal_clip(**ps)
        got, got_m = ctx.read_temporal(), ctx.read_temporal_moments()
        arrays = context_arrays(ctx)
        state = mm.accumulate(state, *arrays, p, mode=1)
        H1, M1 = cm.clip(state["H"], state["M"], *arrays, **ps)
        state = dict(state, H=H1, M=M1)
        check(got, H1, 0.0, "frame_batch 8: history")
        check(got_m, M1, 0.0, "frame_batch 8: moments")
    assert (got[..., 3] == 2.0).any(), "no pixel was clipped: the case shows nothing"
    ctx.close()
    hr = rt.host.HeadlessRenderer(W, H, aov=NORMAL | POSITION)
    hr.set_scene(scene)
    hr.params = base
    state = None
    for _ in range(3):
        p = hr.render_frame()
        hr.temporal_accumulate(max_history=4.0)
        hr.temporal_clip(sigma_scale=1.0)
        arrays = context_arrays(hr.ctx)
        state = tm.accumulate(state, *arrays, p, max_history=4.0)
        state = dict(state, H=cm.clip(state["H"], None, *arrays, sigma_scale=1.0)[0])
    check(hr.read_temporal(), state["H"], 0.0, "headless")
    hr.ctx.close()


# ---------------------------------------------------------------------------------------------- 5. nothing else changes

@pytest.mark.parametrize("name", MIRROR_CASES)
def test_the_frame_path_does_not_notice_the_calls(name, rt):
    """rtgl_temporal_accumulate and rtgl_temporal_clip between the frames of a golden case: the image stays the reference shader's, bit
    for bit; the RNG states, all four planes and the denoised buffer stay those of a run without the calls"""
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
            if calls:
                ctx.temporal_accumulate()
                ctx.temporal_clip()
                ctx.temporal_clip(sigma_scale=0.5, clip_history=1.0, sigma_normal=0.0)
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


RELIT_BACKGROUND = (1.2, 0.6, 0.2)


def test_c1_256_clipped_history_follows_a_change_of_the_background(rt):
    """c1_256 at 256 x 256, the camera at rest: 8 frames, then the `background` colour changes from (0.52, 0.80, 0.92) to (1.2, 0.6, 0.2)
    and 4 more frames follow.  The background colour is the change taken because it is this scene's only light (the scene has no cube map
    for `use_envmap` to switch to).  Reference: 256 accumulated frames of a fresh context under the new background, times 257 / 256
    (DESIGN.md 5.6).  RMSE(clipped history) < RMSE(unclipped history), strictly, no factor; the table for sigma_scale 1 / 1.5 / 2 / 3, with
    and without rtgl_denoise_guided on top, is printed."""
    case, scene, W, H = named_case(rt, "c1_256")
    base = case["frames"][0]

    def run(scale):
        g = rt.scenes.GlibcRand(0)
        ctx = rt.host.Context(W, H)
        ctx.set_aov(GUIDES)
        ctx.upload_scene(scene)
        ctx.set_option("denoise_source", 1)
        for k in range(12):
            p = base.replace(reset_flag=1, frames=0, random=g.rand())
            ctx.render(p if k < 8 else p.replace(background=RELIT_BACKGROUND), sync=False)
            ctx.temporal_accumulate()
            if scale is not None:
                ctx.temporal_clip(sigma_scale=scale)
        history = ctx.read_temporal()
        ctx.denoise_guided()
        out = history, ctx.read_denoised()
        ctx.close()
        return out

    results = {scale: run(scale) for scale in (None, 1.0, 1.5, 2.0, 3.0)}
    g = rt.scenes.GlibcRand(1)
    ref = rt.host.Context(W, H)
    ref.upload_scene(scene)
    for n in range(1, 257):
        ref.render(base.replace(background=RELIT_BACKGROUND, frames=n, random=g.rand()), sync=False)
    target = ref.read_image().astype(np.float64) * (257.0 / 256.0)
    ref.close()
    assert np.isfinite(target).all() and all(np.isfinite(h).all() for h, _ in results.values())
    for scale, (history, denoised) in results.items():
        print(f"c1_256, 8 frames + 4 under the new background, {'no clip' if scale is None else f'sigma_scale {scale:g}'}: RMSE history {rmse(history, target):.5f}, "
              f"rtgl_denoise_guided over it {rmse(denoised, target):.5f}, mean history length {float(history[..., 3].mean()):.2f}")
    assert rmse(results[2.0][0], target) < rmse(results[None][0], target)
