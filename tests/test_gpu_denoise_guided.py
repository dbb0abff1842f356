"""rtgl_denoise_guided on the device (include/rtgl_amd.h, "variance-guided denoiser").

The reference is the numpy restatement, tests/denoise_guided_mirror.py, pinned by tests/test_denoise_guided_mirror.py.  The comparison rule
(`check`), for the denoised image and for all four components of the variance buffer: where the mirror's component is not a NaN the
kernel's has the same bits, no tolerance; where it is a NaN, any NaN will do.  The mirror's NaN share is held to
denoise_guided_inputs.nan_budget, so the rule cannot hide a failure.  Rendered frames, inputs injected from the host (as
tests/test_gpu_denoise_inputs.py does), the host path, the frame path left alone, and the point of it: closer to the converged image."""
import ctypes as C

import numpy as np
import pytest

import denoise_guided_inputs as gi
import denoise_guided_mirror as gm
import denoise_mirror as dm
import golden_cases as gc
import raytracer_glsl_amd
from test_gpu_denoise import (ALBEDO, ALL, ERR_INVALID, ERR_STATE, GUIDES, IDS, MIRROR_CASES, NORMAL, POSITION, bits, c2, differing, golden_path, named_case,
                              same)
from test_gpu_denoise_inputs import holds, inject, prepared
from test_oracle_golden import load_case

pytestmark = pytest.mark.gpu

H_ = raytracer_glsl_amd.host


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


def check(got, want, budget, label):
    """got, want: (image, variance buffer)"""
    nans = sum(int(np.isnan(w).sum()) for w in want) / sum(w.size for w in want)
    assert nans <= budget, f"{label}: {nans:.4%} of the mirror's components are NaN, budget {budget:.0%}"
    for name, g, w in zip(("image", "variance"), got, want):
        nan = np.isnan(w)
        bad = np.where(nan, ~np.isnan(g), bits(g) != bits(w))
        assert not bad.any(), (f"{label}: {name}: {int(bad.sum())} of {bad.size} components differ ({int((bad & nan).sum())} of them not NaN where the "
                               f"mirror is), first at (row, column, channel) {list(zip(*np.nonzero(bad)))[:8]}")


def read_both(ctx):
    return ctx.read_denoised(), ctx.read_denoise_variance()


def context_arrays(ctx):
    aov = ctx.get_option("aov")
    return [ctx.read_image()] + [ctx.read_aov(p) if aov & p else None for p in (ALBEDO, NORMAL, POSITION)]


def mirror_each(arrays, params, passes_list):
    kw = {k: v for k, v in dict(gm.DEFAULTS, **params).items() if k != "passes"}
    return gm.denoise_guided_each(*arrays, passes_list=tuple(passes_list), **kw)


def run_case(ctx, family, params, passes_list, arrays=None):
    """inject the family's arrays and hold every pass count against the mirror, in the order given"""
    W, H = ctx.width, ctx.height
    if arrays is None:
        arrays = inject(ctx, *gi.make(family, H, W))
    want = mirror_each(arrays, params, passes_list)
    for k in passes_list:
        ps = dict(params, passes=k)
        ctx.denoise_guided(**ps)
        got = read_both(ctx)
        label = f"{family} {W} x {H} {ps}"
        full = dict(gm.DEFAULTS, **ps)
        if k == 0 and not full["demodulate"] and full["firefly_ratio"] <= 0:
            assert same(got[0], arrays[0]), f"{label}: not the identity: {differing(got[0], arrays[0])}"
        check(got, want[k], gi.nan_budget(family), label)
    assert holds(ctx, arrays), f"{family} {W} x {H} {params}: the calls changed the image or a plane"
    return arrays


# ---------------------------------------------------------------------------------------------- 1. rendered frames

PARAMETER_SETS = ([dict(passes=k) for k in (0, 1, 5, 8)]
                  + [dict(sigma_normal=0.0), dict(sigma_position=-1.0), dict(sigma_normal=0.0, sigma_position=0.0),        # each term off in turn
                     dict(firefly_ratio=0.0), dict(firefly_ratio=0.0, passes=1), dict(firefly_ratio=3.0, sigma_lum=8.0),    # clamp off / on
                     dict(demodulate=False), dict(demodulate=False, passes=0), dict(demodulate=False, firefly_ratio=0.0, passes=0),
                     dict(sigma_lum=2.0, sigma_normal=0.1, sigma_position=0.01), dict(passes=1, demodulate=False, sigma_normal=0.0, sigma_position=0.0)])


@pytest.mark.parametrize("name", MIRROR_CASES)
def test_image_and_variance_are_bit_identical_to_the_mirror(name, rt):
    """the golden scenes of tests/test_gpu_denoise.py after 1 frame and after 4 accumulated frames, every parameter set"""
    case, scene, W, H = named_case(rt, name)
    frames = gc.frame_sequence(rt.scenes, case["frames"][0].replace(reset_flag=0), 4)
    ctx = rt.host.Context(W, H)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    ctx.write_image(gc.initial_image(case["init"], W, H))
    for k, p in enumerate(frames):
        ctx.render(p)
        if k not in (0, 3):
            continue
        arrays = context_arrays(ctx)
        for ps in PARAMETER_SETS:
            ctx.denoise_guided(**ps)
            check(read_both(ctx), gm.denoise_guided(*arrays, **dict(gm.DEFAULTS, **ps)), 0.0, f"{name}, {k + 1} frame(s), {ps}")
    ctx.close()


def test_planes_the_parameters_do_not_need_may_be_off(rt):
    case, scene, W, H = named_case(rt, "mesh_env_dof")
    for mask, ps in ((ALBEDO, dict(sigma_normal=0.0, sigma_position=0.0)), (NORMAL, dict(demodulate=False, sigma_position=0.0)),
                     (POSITION | IDS, dict(demodulate=False, sigma_normal=0.0)), (0, dict(demodulate=False, sigma_normal=0.0, sigma_position=0.0))):
        ctx = rt.host.Context(W, H)
        ctx.set_aov(mask)
        ctx.upload_scene(scene)
        ctx.render(case["frames"][0])
        ctx.denoise_guided(**ps)
        check(read_both(ctx), gm.denoise_guided(*context_arrays(ctx), **dict(gm.DEFAULTS, **ps)), 0.0, f"aov {mask}, {ps}")
        ctx.close()


def test_kernel_variants_give_the_same_bits(rt):
    case, scene, W, H = named_case(rt, "mesh_env_dof")
    frames = gc.frame_sequence(rt.scenes, case["frames"][0], 3)
    out = {}
    for kernel in (0, 1, 2, 4):
        ctx = rt.host.Context(W, H)
        ctx.set_option("kernel", kernel)
        ctx.set_aov(GUIDES)
        ctx.upload_scene(scene)
        for p in frames:
            ctx.render(p)
        ctx.denoise_guided()
        out[kernel] = read_both(ctx)
        if kernel == 0:
            check(out[0], gm.denoise_guided(*context_arrays(ctx), **gm.DEFAULTS), 0.0, "kernel 0")
        ctx.close()
    for kernel in (1, 2, 4):
        assert same(out[kernel][0], out[0][0]) and same(out[kernel][1], out[0][1]), f"kernel {kernel}: {differing(out[kernel][0], out[0][0])}"


# ---------------------------------------------------------------------------------------------- 2. injected inputs

@pytest.mark.parametrize("size", gi.VALUE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", sorted(gi.VALUE_PARAMS))
def test_special_values_and_subnormal_weights(family, size, rt):
    """NaN, infinities, subnormals, negative colours, albedos around 2^-10, t that makes (sigma_position t)^2 underflow or overflow, 1e20 in
    normal and position; tap weights that are subnormal and matter.  Every parameter set x passes 0, 1, 5, 8."""
    ctx = prepared(rt, *size)
    for params in gi.VALUE_PARAMS[family]:
        run_case(ctx, family, params, gi.VALUE_PASSES)
    ctx.close()


@pytest.mark.parametrize("size", gi.SIZE_CASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_around_the_block_geometry(size, rt):
    """widths around the multiples of 64, heights around 4 step for every step and around the prepare kernel's tile of 64 x 4 with its halo,
    down to 1 x 1; passes 1 .. 8, each count a call of its own"""
    ctx = prepared(rt, *size)
    for family, params in gi.SIZE_RUNS:
        run_case(ctx, family, params, gi.SIZE_PASSES)
    ctx.close()


@pytest.mark.parametrize("size", gi.NARROW_HEIGHTS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_heights_around_every_chunk_of_rows(size, rt):
    ctx = prepared(rt, *size)
    run_case(ctx, "ramps", gi.RAMPS_OFF, gi.SIZE_PASSES)
    ctx.close()


def test_wide_steps_with_their_far_taps_inside_the_image(rt):
    """700 x 530: at steps 64 and 128 the taps at +-128 and +-256 are inside the image, in other blocks and other row chunks"""
    ctx = prepared(rt, *gi.WIDE_SIZE)
    for family, params in gi.WIDE_RUNS:
        run_case(ctx, family, params, gi.WIDE_PASSES)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 3. host path

@pytest.mark.parametrize("order", [(2, 3, 1, 8, 0), (1, 2, 8), (0, 5)], ids=lambda o: "-".join(map(str, o)))
def test_buffers_are_allocated_when_a_call_first_needs_them(order, rt):
    """a fresh context whose first call is not the default: passes = 0 needs no scratch buffer, 1 one, 2 both"""
    ctx = prepared(rt, 70, 53)
    for family, params in (("specials", dict()), ("ramps", gi.RAMPS_OPEN)):
        run_case(ctx, family, params, order)
    ctx.close()


def test_two_live_contexts_take_turns(rt):
    a, b = prepared(rt, 70, 53), prepared(rt, 321, 129)
    ina = inject(a, *gi.make("specials", 53, 70))
    inb = inject(b, *gi.make("ramps", 129, 321))
    counts = (2, 8, 5)
    want_a, want_b = mirror_each(ina, dict(), counts), mirror_each(inb, gi.RAMPS_OPEN, counts)
    for k in counts:
        a.denoise_guided(passes=k)
        b.denoise_guided(**dict(gi.RAMPS_OPEN, passes=k))
        got_a, got_b = read_both(a), read_both(b)
        check(got_a, want_a[k], gi.nan_budget("specials"), f"context 70 x 53, passes {k}")
        check(got_b, want_b[k], 0.0, f"context 321 x 129, passes {k}")
    assert holds(a, ina) and holds(b, inb)
    a.close()
    b.close()


def test_both_denoisers_alternate_on_one_context(rt):
    """they share the denoised buffer and the scratch buffers: the later call wins, neither disturbs the other's next result; the
    variance buffer is the guided call's alone"""
    ctx = prepared(rt, 200, 131)
    arrays = inject(ctx, *gi.make("specials", 131, 200))
    plain = {k: dm.denoise(*arrays, **dict(dm.DEFAULTS, passes=k)) for k in (5, 2)}
    guided = mirror_each(arrays, dict(), (5, 1, 0))
    budget = gi.nan_budget("specials")
    for k_plain, k_guided in ((5, 5), (2, 1), (5, 0), (2, 5)):
        ctx.denoise(passes=k_plain)
        nan = np.isnan(plain[k_plain])
        got = ctx.read_denoised()
        assert not np.where(nan, ~np.isnan(got), bits(got) != bits(plain[k_plain])).any(), f"rtgl_denoise passes {k_plain} after a guided call"
        ctx.denoise_guided(passes=k_guided)
        check(read_both(ctx), guided[k_guided], budget, f"rtgl_denoise_guided passes {k_guided} after rtgl_denoise passes {k_plain}")
        var = ctx.read_denoise_variance()
        ctx.denoise(passes=k_plain)
        assert same(ctx.read_denoise_variance(), var), "rtgl_denoise changed the variance buffer"
    assert holds(ctx, arrays)
    ctx.close()


def raw_guided(ctx, **fields):
    p = H_.CDenoiseGuidedParams()
    assert ctx.lib.rtgl_denoise_guided_defaults(C.byref(p)) == 0
    for k, v in fields.items():
        setattr(p, k, v)
    return ctx.lib.rtgl_denoise_guided(ctx.h, C.byref(p))


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
    # read-out before the first successful call; a successful rtgl_denoise does not count
    assert lib.rtgl_read_denoise_variance_f32(ctx.h, ptr) == ERR_STATE and ctx.device_denoise_variance_ptr() == 0
    ctx.render(frames[0])
    ctx.denoise(demodulate=False, sigma_normal=0.0, sigma_position=0.0)
    assert lib.rtgl_read_denoise_variance_f32(ctx.h, ptr) == ERR_STATE and ctx.device_denoise_variance_ptr() == 0
    # planes missing
    assert lib.rtgl_denoise_guided(ctx.h, None) == ERR_STATE and b"aov" in lib.rtgl_last_error(ctx.h)
    ctx.set_aov(ALBEDO | IDS)
    ctx.render(frames[1])
    assert raw_guided(ctx) == ERR_STATE
    assert raw_guided(ctx, sigma_normal=0.0) == ERR_STATE
    assert lib.rtgl_read_denoise_variance_f32(ctx.h, ptr) == ERR_STATE
    assert raw_guided(ctx, sigma_normal=0.0, sigma_position=0.0) == 0
    assert lib.rtgl_read_denoise_variance_f32(ctx.h, ptr) == 0 and ctx.device_denoise_variance_ptr() != 0
    assert raw_guided(ctx, flags=0, sigma_position=0.0) == ERR_STATE
    # no frame since the planes restarted: after the option was set, after rtgl_clear_image
    ctx.set_aov(GUIDES)
    assert lib.rtgl_denoise_guided(ctx.h, None) == ERR_STATE and b"frame" in lib.rtgl_last_error(ctx.h)
    ctx.render(frames[2])
    assert lib.rtgl_denoise_guided(ctx.h, None) == 0
    ctx.clear_image()
    assert lib.rtgl_denoise_guided(ctx.h, None) == ERR_STATE
    ctx.render(frames[3])
    assert lib.rtgl_denoise_guided(ctx.h, None) == 0
    # bad parameters
    assert raw_guided(ctx, passes=9) == ERR_INVALID
    assert raw_guided(ctx, passes=8) == 0
    for field in ("sigma_lum", "sigma_normal", "sigma_position", "firefly_ratio"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert raw_guided(ctx, **{field: bad}) == ERR_INVALID, (field, bad)
    assert raw_guided(ctx, sigma_lum=0.0) == ERR_INVALID and raw_guided(ctx, sigma_lum=-2.0) == ERR_INVALID
    assert raw_guided(ctx, sigma_normal=-1.0, sigma_position=0.0, firefly_ratio=-1.0) == 0
    assert raw_guided(ctx, flags=2) == ERR_INVALID and raw_guided(ctx, flags=3) == ERR_INVALID
    for k in range(2):
        r = [0, 0]
        r[k] = 1
        assert raw_guided(ctx, reserved=(C.c_uint32 * 2)(*r)) == ERR_INVALID
    assert lib.rtgl_read_denoise_variance_f32(ctx.h, None) == ERR_INVALID
    assert lib.rtgl_denoise_guided(None, None) == ERR_INVALID
    with pytest.raises(rt.host.RtglError):
        ctx.denoise_guided(passes=9)
    ctx.close()
    # tiled and multi-device contexts: out of scope, and the message says so
    for kw in (dict(rank=0, world=2, strip_rows=16), dict(devices=[0, 0], strip_rows=8)):
        ctx = rt.host.Context(W, H, **kw)
        ctx.set_aov(GUIDES)
        ctx.upload_scene(scene)
        ctx.render(frames[0])
        assert lib.rtgl_denoise_guided(ctx.h, None) == ERR_STATE and b"out of scope" in lib.rtgl_last_error(ctx.h), kw
        assert lib.rtgl_read_denoise_variance_f32(ctx.h, ptr) == ERR_STATE and ctx.device_denoise_variance_ptr() == 0
        ctx.close()


def test_batching_snapshot_and_device_pointer(rt):
    import torch
    from test_gpu_denoise import _DeviceArray
    sc = rt.scenes
    W, H = 72, 61
    scene = sc.scene_mesh(10, 5, env_size=16)
    frames = gc.frame_sequence(sc, sc.params_c2(), 6)
    # frame_batch = 8 without planes: the three frames are still held back when the call comes, and it submits them first
    ctx = rt.host.Context(W, H)
    ctx.set_option("frame_batch", 8)
    ctx.upload_scene(scene)
    ps = dict(demodulate=False, sigma_normal=0.0, sigma_position=0.0)
    for p in frames[:3]:
        ctx.render(p, sync=False)
    ctx.denoise_guided(**ps)
    first = read_both(ctx)
    img = ctx.read_image()
    assert (img[:56, :72, :3] != 0).any()
    check(first, gm.denoise_guided(img, **dict(gm.DEFAULTS, **ps)), 0.0, "three batched frames")
    # torch interop: a tensor on the device pointer reads what rtgl_read_denoise_variance_f32 copies
    vptr = ctx.device_denoise_variance_ptr()
    assert vptr
    t = torch.as_tensor(_DeviceArray(vptr, (H, W, 4), "<f4"), device="cuda:0")
    torch.cuda.synchronize()
    assert same(t.cpu().numpy(), first[1])
    # a snapshot: later frames leave both buffers alone, the next call replaces them, the pointers stay
    dptr = ctx.device_denoised_ptr()
    for p in frames[3:]:
        ctx.render(p)
    again = read_both(ctx)
    assert same(again[0], first[0]) and same(again[1], first[1])
    ctx.denoise_guided(**ps)
    assert not same(ctx.read_denoised(), first[0]) and ctx.device_denoised_ptr() == dptr and ctx.device_denoise_variance_ptr() == vptr
    ctx.close()
    # the headless renderer passes the calls through
    hr = rt.host.HeadlessRenderer(W, H, aov=GUIDES)
    hr.set_scene(scene)
    hr.params = sc.params_c2()
    hr.run(2)
    hr.denoise_guided(passes=3)
    check((hr.read_denoised(), hr.read_denoise_variance()), gm.denoise_guided(*context_arrays(hr.ctx), **dict(gm.DEFAULTS, passes=3)), 0.0, "headless")
    hr.ctx.close()


# ---------------------------------------------------------------------------------------------- 4. nothing else changes

@pytest.mark.parametrize("name", MIRROR_CASES)
def test_the_frame_path_does_not_notice_the_calls(name, rt):
    """rtgl_denoise_guided (and rtgl_denoise) between the frames of a golden case: the image stays the reference shader's, bit for bit; the
    RNG states and all four planes stay those of a run without the calls"""
    meta, scene, frames, expected = load_case(golden_path(name), rt)
    W, H = meta["width"], meta["height"]

    def run(calls):
        ctx = rt.host.Context(W, H)
        ctx.set_option("rng_state", 1)
        ctx.set_aov(ALL)
        ctx.upload_scene(scene)
        ctx.write_image(gc.initial_image(meta["init"], W, H))
        for p in frames:
            ctx.render(p, sync=False)
            if calls:
                ctx.denoise_guided()
                ctx.denoise()
                ctx.denoise_guided(passes=2, demodulate=False, firefly_ratio=0.0)
        out = dict(img=ctx.read_image(), seeds=ctx.read_rng_state(), planes={p: ctx.read_aov(p) for p in (ALBEDO, NORMAL, POSITION, IDS)})
        ctx.close()
        return out

    with_calls, without = run(True), run(False)
    assert same(with_calls["img"], expected), differing(with_calls["img"], expected)
    assert same(without["img"], expected)
    fh, fw = H // 8 * 8, W // 8 * 8                      # (outside the dispatch footprint the RNG buffer is never written)
    assert (with_calls["seeds"][:fh, :fw] == without["seeds"][:fh, :fw]).all()
    for p in (ALBEDO, NORMAL, POSITION, IDS):
        assert same(with_calls["planes"][p], without["planes"][p]), f"plane {p}"


# ---------------------------------------------------------------------------------------------- 5. it denoises

def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def errors_after(rt, W, H, scene, frames, counts):
    """{n: (RMSE of the raw image, of rtgl_denoise's, of rtgl_denoise_guided's)} after n frames, each against the context's own image 256
    frames later scaled by n / (n + 1): the running mean divides frame n by frames + 1, so after n frames on a zeroed image the picture
    is n / (n + 1) as bright as the converged one, a bias no filter may remove"""
    frames = iter(frames)
    ctx = rt.host.Context(W, H)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    got, converged = {}, {}
    for n in range(1, max(counts) + 257):
        ctx.render(next(frames), sync=False)
        if n in counts:
            ctx.denoise()
            plain = ctx.read_denoised()
            ctx.denoise_guided()
            got[n] = (ctx.read_image(), plain, ctx.read_denoised())
        if n - 256 in counts:
            converged[n - 256] = ctx.read_image()
    ctx.close()
    out = {}
    for n, images in got.items():
        assert np.isfinite(converged[n]).all() and all(np.isfinite(i).all() for i in images)
        target = converged[n].astype(np.float64) * (n / (n + 1))
        out[n] = tuple(rmse(i, target) for i in images)
    return out


def closer_to_the_converged_image(label, errs):
    for n, (raw, plain, guided) in errs.items():
        print(f"{label}, {n} frame(s): RMSE raw {raw:.5f}, rtgl_denoise {plain:.5f}, rtgl_denoise_guided {guided:.5f} (ratio to raw {guided / raw:.4f})")
    for n, (raw, plain, guided) in errs.items():
        assert guided < raw, f"{label}, {n} frame(s)"


def test_c2_scene_at_640x360_is_closer_to_the_converged_image(rt):
    """after 1 and after 4 frames, defaults: RMSE(guided) < RMSE(raw), strictly, no factor (the figures are printed)"""
    sc = rt.scenes
    cfg = sc.CONFIGS["C2"]
    g = sc.GlibcRand(0)
    frames = (cfg["params"]().replace(frames=f, random=g.rand()) for f in range(1, 100000))
    closer_to_the_converged_image("C2 scene 640 x 360", errors_after(rt, 640, 360, cfg["scene"](), frames, (1, 4)))


def test_c1_256_is_closer_to_the_converged_image(rt):
    case, scene, W, H = named_case(rt, "c1_256")
    g = rt.scenes.GlibcRand(0)
    frames = (case["frames"][0].replace(frames=f, random=g.rand()) for f in range(1, 100000))
    closer_to_the_converged_image("c1_256", errors_after(rt, W, H, scene, frames, (1, 4)))


def test_c2_full_frame_matches_the_mirror(rt):
    """1920 x 1080, one rendered frame, defaults"""
    W, H, scene, frames = c2(rt)
    ctx = rt.host.Context(W, H)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    ctx.render(next(frames))
    ctx.denoise_guided()
    got, want = read_both(ctx), gm.denoise_guided(*context_arrays(ctx), **gm.DEFAULTS)
    ctx.close()
    check(got, want, 0.0, "C2, defaults")
