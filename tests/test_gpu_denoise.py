"""rtgl_denoise on the device (include/rtgl_amd.h, "denoiser").

The reference for the filter is its numpy restatement, tests/denoise_mirror.py (pinned by tests/test_denoise_mirror.py): the kernel must
return the same bits, no tolerance.  The frame path must not notice the calls: image, RNG states and planes stay what they are without
them.  And the point of it all: after one frame the denoised image is closer to the converged one than the raw image is."""
import ctypes as C

import numpy as np
import pytest

import denoise_mirror as dm
import golden_cases as gc
import raytracer_glsl_amd
from test_oracle_golden import CASE_FILES, load_case

pytestmark = pytest.mark.gpu

H_ = raytracer_glsl_amd.host
ALBEDO, NORMAL, POSITION, IDS, ALL = H_.AOV_ALBEDO, H_.AOV_NORMAL, H_.AOV_POSITION, H_.AOV_IDS, H_.AOV_ALL
GUIDES = ALBEDO | NORMAL | POSITION
ERR_INVALID, ERR_STATE = -1, -4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and (bits(a) == bits(b)).all()


def differing(a, b):
    d = (bits(a) != bits(b)).any(axis=2)
    return f"{int(d.sum())} of {d.size} pixels differ, first at (row, column) {list(zip(*np.nonzero(d)))[:8]}"


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_aov.py does)"""
    import torch
    torch.cuda.init()


def mirror_of(ctx, **params):
    """the restatement applied to what the context holds now"""
    aov = ctx.get_option("aov")
    planes = [ctx.read_aov(p) if aov & p else None for p in (ALBEDO, NORMAL, POSITION)]
    return dm.denoise(ctx.read_image(), *planes, **dict(dm.DEFAULTS, **params))


def named_case(rt, name):
    case = gc.build_cases(rt.scenes)[name]
    return case, case["scene"](), case["width"], case["height"]


def c2(rt):
    sc = rt.scenes
    cfg = sc.CONFIGS["C2"]
    g = sc.GlibcRand(0)
    return cfg["width"], cfg["height"], cfg["scene"](), (cfg["params"]().replace(frames=f, random=g.rand()) for f in range(1, 100000))


# ---------------------------------------------------------------------------------------------- 1. bit-identical to the mirror

PARAMETER_SETS = ([dict()] + [dict(passes=k) for k in (1, 2, 3, 4, 8)]
                  + [dict(sigma_color=0.0), dict(sigma_normal=0.0), dict(sigma_position=-1.0), dict(demodulate=False),
                     dict(sigma_color=0.5, sigma_normal=0.1, sigma_position=0.01), dict(passes=0), dict(passes=0, demodulate=False),
                     dict(passes=1, demodulate=False), dict(passes=2, sigma_normal=0.0, sigma_position=0.0, demodulate=False)])
MIRROR_CASES = ["c1_256", "c1_ragged_70x53", "mesh_env_dof", "glass_inside_tir", "env_disabled_background"]


@pytest.mark.parametrize("name", MIRROR_CASES)
def test_denoised_image_is_bit_identical_to_the_mirror(name, rt):
    """after 1 frame and after 4 accumulated frames, every parameter set (the defaults are passes = 5)"""
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
        for ps in PARAMETER_SETS:
            ctx.denoise(**ps)
            got, want = ctx.read_denoised(), mirror_of(ctx, **ps)
            assert same(got, want), f"{name}, {k + 1} frame(s), {ps}: {differing(got, want)}"
    ctx.close()


def test_planes_the_parameters_do_not_need_may_be_off(rt):
    case, scene, W, H = named_case(rt, "mesh_env_dof")
    for mask, ps in ((ALBEDO, dict(sigma_normal=0.0, sigma_position=0.0)), (NORMAL, dict(demodulate=False, sigma_position=0.0)),
                     (POSITION | IDS, dict(demodulate=False, sigma_normal=0.0)), (0, dict(demodulate=False, sigma_normal=0.0, sigma_position=0.0))):
        ctx = rt.host.Context(W, H)
        ctx.set_aov(mask)
        ctx.upload_scene(scene)
        ctx.render(case["frames"][0])
        ctx.denoise(**ps)
        got, want = ctx.read_denoised(), mirror_of(ctx, **ps)
        assert same(got, want), f"aov {mask}, {ps}: {differing(got, want)}"
        ctx.close()


# ---------------------------------------------------------------------------------------------- 2. nothing else changes

def golden_path(name):
    return next(p for p in CASE_FILES if p.endswith("/" + name + ".npz"))


@pytest.mark.parametrize("name", MIRROR_CASES)
def test_the_frame_path_does_not_notice_the_calls(name, rt):
    """rtgl_denoise between the frames of a golden case: the image stays the reference shader's, bit for bit; the RNG states and all
    four planes stay those of a run without the calls"""
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
                ctx.denoise()
                ctx.denoise(passes=2, demodulate=False)
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


# ---------------------------------------------------------------------------------------------- 3. every kernel variant

def test_kernel_variants_give_the_same_denoised_bits(rt):
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
        ctx.denoise()
        out[kernel] = ctx.read_denoised()
        if kernel == 0:
            want = mirror_of(ctx)
            assert same(out[0], want), differing(out[0], want)
        ctx.close()
    for kernel in (1, 2, 4):
        assert same(out[kernel], out[0]), f"kernel {kernel}: {differing(out[kernel], out[0])}"


# ---------------------------------------------------------------------------------------------- 4 + 5. full size; it denoises

def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def one_frame_then_converge(rt, W, H, scene, frames, check_mirror):
    """(RMSE of the raw first frame, RMSE of its denoised image) against the context's own image after 256 more frames"""
    frames = iter(frames)
    ctx = rt.host.Context(W, H)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    ctx.render(next(frames))
    ctx.denoise()
    raw, den = ctx.read_image(), ctx.read_denoised()
    if check_mirror:
        want = mirror_of(ctx)
        assert same(den, want), differing(den, want)
    for _ in range(256):
        ctx.render(next(frames), sync=False)
    converged = ctx.read_image()
    assert same(ctx.read_denoised(), den), "later frames changed the denoised buffer: it is a snapshot"
    ctx.close()
    assert np.isfinite(converged).all() and np.isfinite(den).all()
    return rmse(raw, converged), rmse(den, converged)


def test_c2_full_frame_matches_the_mirror_and_is_closer_to_the_converged_image(rt):
    """1920 x 1080, one frame, defaults: the whole frame against the mirror bit for bit; then RMSE(denoised) < RMSE(raw) against the
    image 256 frames later (strict improvement, no factor; the ratio is printed and recorded in DESIGN.md 5.4)"""
    W, H, scene, frames = c2(rt)
    e_raw, e_den = one_frame_then_converge(rt, W, H, scene, frames, check_mirror=True)
    print(f"C2: RMSE raw {e_raw:.5f}, denoised {e_den:.5f}, ratio {e_den / e_raw:.4f}")
    assert e_den < e_raw


def test_c1_256_is_closer_to_the_converged_image(rt):
    case, scene, W, H = named_case(rt, "c1_256")
    sc = rt.scenes
    g = sc.GlibcRand(0)
    frames = (case["frames"][0].replace(frames=f, random=g.rand()) for f in range(1, 100000))
    e_raw, e_den = one_frame_then_converge(rt, W, H, scene, frames, check_mirror=False)
    print(f"c1_256: RMSE raw {e_raw:.5f}, denoised {e_den:.5f}, ratio {e_den / e_raw:.4f}")
    assert e_den < e_raw


# ---------------------------------------------------------------------------------------------- 6. errors and lifetime

class _DeviceArray:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}


def raw_denoise(ctx, **fields):
    p = H_.CDenoiseParams()
    assert ctx.lib.rtgl_denoise_defaults(C.byref(p)) == 0
    for k, v in fields.items():
        setattr(p, k, v)
    return ctx.lib.rtgl_denoise(ctx.h, C.byref(p))


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
    # read-out before the first successful call
    assert lib.rtgl_read_denoised_f32(ctx.h, ptr) == ERR_STATE and ctx.device_denoised_ptr() == 0
    # planes missing
    ctx.render(frames[0])
    assert lib.rtgl_denoise(ctx.h, None) == ERR_STATE and b"aov" in lib.rtgl_last_error(ctx.h)
    ctx.set_aov(ALBEDO | IDS)
    ctx.render(frames[1])
    assert raw_denoise(ctx) == ERR_STATE
    assert raw_denoise(ctx, sigma_normal=0.0) == ERR_STATE
    assert raw_denoise(ctx, sigma_normal=0.0, sigma_position=0.0) == 0
    assert raw_denoise(ctx, flags=0, sigma_position=0.0) == ERR_STATE
    # no frame since the planes restarted: after the option was set, after rtgl_clear_image
    ctx.set_aov(GUIDES)
    assert lib.rtgl_denoise(ctx.h, None) == ERR_STATE and b"frame" in lib.rtgl_last_error(ctx.h)
    ctx.render(frames[2])
    assert lib.rtgl_denoise(ctx.h, None) == 0
    ctx.clear_image()
    assert lib.rtgl_denoise(ctx.h, None) == ERR_STATE
    ctx.render(frames[3])
    assert lib.rtgl_denoise(ctx.h, None) == 0
    # bad parameters
    assert raw_denoise(ctx, passes=9) == ERR_INVALID
    assert raw_denoise(ctx, passes=8) == 0
    for field in ("sigma_color", "sigma_normal", "sigma_position"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert raw_denoise(ctx, **{field: bad}) == ERR_INVALID
    assert raw_denoise(ctx, flags=2) == ERR_INVALID and raw_denoise(ctx, flags=3) == ERR_INVALID
    for k in range(3):
        r = [0, 0, 0]
        r[k] = 1
        assert raw_denoise(ctx, reserved=(C.c_uint32 * 3)(*r)) == ERR_INVALID
    assert lib.rtgl_read_denoised_f32(ctx.h, None) == ERR_INVALID
    with pytest.raises(rt.host.RtglError):
        ctx.denoise(passes=9)
    ctx.close()
    # tiled and multi-device contexts: out of scope, and the message says so
    for kw in (dict(rank=0, world=2, strip_rows=16), dict(devices=[0, 0], strip_rows=8)):
        ctx = rt.host.Context(W, H, **kw)
        ctx.set_aov(GUIDES)
        ctx.upload_scene(scene)
        ctx.render(frames[0])
        assert lib.rtgl_denoise(ctx.h, None) == ERR_STATE and b"out of scope" in lib.rtgl_last_error(ctx.h), kw
        assert lib.rtgl_read_denoised_f32(ctx.h, ptr) == ERR_STATE and ctx.device_denoised_ptr() == 0
        ctx.close()


def test_lifetime_batching_and_device_pointer(rt):
    import torch
    sc = rt.scenes
    W, H = 72, 61
    scene = sc.scene_mesh(10, 5, env_size=16)
    frames = gc.frame_sequence(sc, sc.params_c2(), 6)
    # frame_batch = 8 and the planes on (frames are then rendered one by one): the call sees every submitted frame
    ctx = rt.host.Context(W, H)
    ctx.set_option("frame_batch", 8)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    for p in frames[:3]:
        ctx.render(p, sync=False)
    ctx.denoise()
    first = ctx.read_denoised()
    want = mirror_of(ctx)
    assert same(first, want), differing(first, want)
    # the same inputs again: the same bits
    ctx.denoise()
    assert same(ctx.read_denoised(), first)
    # torch interop: a tensor on the device pointer reads what rtgl_read_denoised_f32 copies
    dptr = ctx.device_denoised_ptr()
    assert dptr
    t = torch.as_tensor(_DeviceArray(dptr, (H, W, 4), "<f4"), device="cuda:0")
    torch.cuda.synchronize()
    assert same(t.cpu().numpy(), first)
    # a snapshot: later frames leave it alone, the next call replaces it, the pointer stays
    for p in frames[3:]:
        ctx.render(p)
    assert same(ctx.read_denoised(), first)
    ctx.denoise()
    assert not same(ctx.read_denoised(), first) and ctx.device_denoised_ptr() == dptr
    ctx.close()

    # frame_batch = 8 without planes: the three frames are still held back when the call comes, and it submits them first
    ctx = rt.host.Context(W, H)
    ctx.set_option("frame_batch", 8)
    ctx.upload_scene(scene)
    ps = dict(demodulate=False, sigma_normal=0.0, sigma_position=0.0)
    for p in frames[:3]:
        ctx.render(p, sync=False)
    ctx.denoise(**ps)
    got = ctx.read_denoised()
    img = ctx.read_image()
    ctx.close()
    ref = rt.host.Context(W, H)
    ref.upload_scene(scene)
    for p in frames[:3]:
        ref.render(p)
    assert same(img, ref.read_image())
    ref.close()
    assert (img[:56, :72, :3] != 0).any()
    want = dm.denoise(img, **dict(dm.DEFAULTS, **ps))
    assert same(got, want), differing(got, want)

    # the headless renderer passes the calls through
    hr = rt.host.HeadlessRenderer(W, H, aov=GUIDES)
    hr.set_scene(scene)
    hr.params = sc.params_c2()
    hr.run(2)
    hr.denoise(passes=3)
    assert same(hr.read_denoised(), mirror_of(hr.ctx, passes=3)) and hr.device_denoised_ptr()
    hr.ctx.close()
