"""rtgl_denoise on inputs that no renderer produces (include/rtgl_amd.h, "denoiser").

tests/test_gpu_denoise.py only ever shows the kernel rendered frames.  Here the image and the three guide planes are overwritten from the
host with the families of tests/denoise_inputs.py: NaN, infinities, subnormals, albedos around the floor, subnormal tap weights,
position-coded ramps; at the sizes where the block geometry has its edges (64 columns, four rows `step` apart, chunks of 4 step rows), with
the wide steps' far taps inside the image, and through the host path's lazy allocations.  The reference is the numpy restatement,
tests/denoise_mirror.py, pinned on exactly these inputs by tests/test_denoise_inputs.py, which also proves for every plausible kernel
defect that a case of this module sees it.

The comparison rule (`check`): where the mirror's component is not a NaN the kernel's has the same bits, signs of zero and infinities
included, no tolerance; where it is a NaN the kernel's is a NaN of any sign and payload (the contract reserves exactly that).  The mirror's
NaN share is asserted to stay within denoise_inputs.nan_budget, so the rule cannot hide a failure."""
import numpy as np
import pytest

import denoise_inputs as di
import denoise_mirror as dm
import golden_cases as gc
from test_gpu_denoise import ALBEDO, GUIDES, NORMAL, POSITION, _DeviceArray, bits, c2, differing, mirror_of, same

pytestmark = pytest.mark.gpu

PLANES = (ALBEDO, NORMAL, POSITION)


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


def prepared(rt, W, H):
    """A context in the state rtgl_denoise asks for: the guide planes on and one frame of a trivial scene rendered.  This also holds below
    8 x 8, where the dispatch footprint of the frame is empty: the frame counts, the filter takes all width x height pixels."""
    sc = rt.scenes
    ctx = rt.host.Context(W, H)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(sc.scene_mesh(10, 5, env_size=16))
    ctx.render(gc.frame_sequence(sc, sc.params_c2(), 1)[0])
    return ctx


def plane_tensor(ctx, plane):
    import torch
    ptr = ctx.device_aov_ptr(plane)
    assert ptr
    return torch.as_tensor(_DeviceArray(ptr, (ctx.height, ctx.width, 4), "<f4"), device="cuda:0")


def holds(ctx, arrays):
    """image and planes of the context are bit for bit the arrays"""
    held = [ctx.read_image()] + [ctx.read_aov(p) for p in PLANES]
    return all(same(h, a) for h, a in zip(held, arrays))


def inject(ctx, image, albedo, normal, position, image_tensor=None):
    """Put the arrays in front of the kernel: the image through rtgl_write_image_f32 (or, bound to a tensor, like the planes), each plane by a
    host-to-device copy into a tensor over its device pointer (copies, not a kernel's stores: DESIGN.md 5.2).  Then read everything back: a
    case cannot silently run on other data."""
    import torch
    arrays = [np.ascontiguousarray(a, np.float32) for a in (image, albedo, normal, position)]
    ctx.synchronize()
    if image_tensor is None:
        ctx.write_image(arrays[0])
    else:
        image_tensor.copy_(torch.from_numpy(arrays[0]))
    for plane, a in zip(PLANES, arrays[1:]):
        plane_tensor(ctx, plane).copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    assert holds(ctx, arrays), "the context does not hold the injected bits"
    return arrays


def check(got, want, budget, label):
    nan = np.isnan(want)
    share = float(nan.mean())
    assert share <= budget, f"{label}: {share:.4%} of the mirror's components are NaN, budget {budget:.0%}"
    bad = np.where(nan, ~np.isnan(got), bits(got) != bits(want))
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {bad.size} components differ ({int((bad & nan).sum())} of them not NaN where the mirror is), "
                           f"first at (row, column, channel) {list(zip(*np.nonzero(bad)))[:8]}")


def run_case(ctx, family, params, passes_list, arrays=None):
    """inject the family's arrays for this parameter set and hold every pass count, in increasing order, against the mirror: the first
    count that fails names the step (2^(passes - 1))"""
    W, H = ctx.width, ctx.height
    if arrays is None:
        arrays = inject(ctx, *di.make(family, H, W, params))
    for k in passes_list:
        ps = dict(params, passes=k)
        ctx.denoise(**ps)
        got = ctx.read_denoised()
        label = f"{family} {W} x {H} {ps}"
        if k == 0 and not dict(dm.DEFAULTS, **ps)["demodulate"]:
            assert same(got, arrays[0]), f"{label}: not the identity: {differing(got, arrays[0])}"
        check(got, dm.denoise(*arrays, **dict(dm.DEFAULTS, **ps)), di.nan_budget(family, ps), label)
    assert holds(ctx, arrays), f"{family} {W} x {H} {params}: the calls changed the image or a plane"
    return arrays


# ---------------------------------------------------------------------------------------------- 1. values

@pytest.mark.parametrize("size", di.VALUE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", sorted(di.VALUE_PARAMS))
def test_special_values_and_subnormal_weights(family, size, rt):
    """NaN, infinities, subnormals, negative colours, albedos around 2^-10, t that makes (sigma_position t)^2 underflow or overflow, 1e20 in
    normal and position; tap weights that are subnormal and matter.  Every parameter set x passes 0, 1, 5, 8."""
    ctx = prepared(rt, *size)
    for params in di.VALUE_PARAMS[family]:
        run_case(ctx, family, params, di.VALUE_PASSES)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. sizes

@pytest.mark.parametrize("size", di.SIZE_CASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_around_the_block_geometry(size, rt):
    """widths around the multiples of 64 and heights around 4 step for every step, down to 1 x 1; passes 1 .. 8, each count on its own"""
    ctx = prepared(rt, *size)
    for family, params in di.SIZE_RUNS:
        run_case(ctx, family, params, di.SIZE_PASSES)
    ctx.close()


@pytest.mark.parametrize("size", di.NARROW_HEIGHTS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_heights_around_every_chunk_of_rows(size, rt):
    ctx = prepared(rt, *size)
    run_case(ctx, "ramps", di.RAMPS_OFF, di.SIZE_PASSES)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 3. wide steps inside the image

def test_wide_steps_with_their_far_taps_inside_the_image(rt):
    """700 x 530: at steps 64 and 128 the taps at +-128 and +-256 are inside the image, in other blocks and other row chunks"""
    ctx = prepared(rt, *di.WIDE_SIZE)
    for family, params in di.WIDE_RUNS:
        run_case(ctx, family, params, di.WIDE_PASSES)
    ctx.close()


def test_c2_full_frame_with_eight_passes(rt):
    """1920 x 1080, one rendered frame, passes = 8 (tests/test_gpu_denoise.py holds the same frame at the default 5)"""
    W, H, scene, frames = c2(rt)
    ctx = rt.host.Context(W, H)
    ctx.set_aov(GUIDES)
    ctx.upload_scene(scene)
    ctx.render(next(frames))
    ctx.denoise(passes=8)
    got, want = ctx.read_denoised(), mirror_of(ctx, passes=8)
    ctx.close()
    check(got, want, 0.0, "C2, passes 8")


# ---------------------------------------------------------------------------------------------- 4. host path

@pytest.mark.parametrize("order", [(2, 3, 1, 8, 0), (1, 2, 8)], ids=lambda o: "-".join(map(str, o)))
def test_scratch_buffers_are_allocated_when_a_call_first_needs_them(order, rt):
    """a fresh context whose first call is not the default: passes = 2 needs one scratch buffer, 3 the second, 1 none"""
    ctx = prepared(rt, 70, 53)
    for family, params in (("specials", dict()), ("ramps", di.RAMPS_OPEN)):
        arrays = inject(ctx, *di.make(family, 53, 70, params))
        run_case(ctx, family, params, order, arrays=arrays)
    ctx.close()


def test_two_live_contexts_take_turns(rt):
    a, b = prepared(rt, 70, 53), prepared(rt, 321, 129)
    ina = inject(a, *di.make("specials", 53, 70, dict()))
    inb = inject(b, *di.make("ramps", 129, 321, di.RAMPS_OPEN))
    for k in (2, 8, 5):
        a.denoise(passes=k)
        b.denoise(**dict(di.RAMPS_OPEN, passes=k))
        got_a, got_b = a.read_denoised(), b.read_denoised()
        check(got_a, dm.denoise(*ina, **dict(dm.DEFAULTS, passes=k)), di.nan_budget("specials", dict()), f"context 70 x 53, passes {k}")
        check(got_b, dm.denoise(*inb, **dict(dm.DEFAULTS, **di.RAMPS_OPEN, passes=k)), 0.0, f"context 321 x 129, passes {k}")
    assert holds(a, ina) and holds(b, inb)
    a.close()
    b.close()


def test_an_image_bound_to_a_tensor_and_the_same_inputs_twice(rt):
    import torch
    W, H = 200, 131
    image = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    sc = rt.scenes
    ctx = rt.host.Context(W, H)
    ctx.bind_device_image(image.data_ptr())
    ctx.set_aov(GUIDES)
    ctx.upload_scene(sc.scene_mesh(10, 5, env_size=16))
    ctx.render(gc.frame_sequence(sc, sc.params_c2(), 1)[0])
    arrays = inject(ctx, *di.make("specials", H, W, dict()), image_tensor=image)
    assert same(image.cpu().numpy(), arrays[0])
    run_case(ctx, "specials", dict(), (5, 8), arrays=arrays)
    ctx.denoise()
    first = ctx.read_denoised()
    ctx.denoise(passes=8)
    ctx.denoise()
    assert same(ctx.read_denoised(), first), "the same inputs twice: NaN signs and payloads included"
    ctx.bind_device_image(0)
    ctx.close()
