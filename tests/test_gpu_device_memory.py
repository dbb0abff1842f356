"""What a context holds on the device: option "device_mbytes" is the sum over the context's buffer ledger (rt_buffers.hpp), and buffers
that grow between frames leave the images as they were.

One 512 x 512 context: a 16-byte plane is exactly 4 MiB and a 4-byte plane exactly 1 MiB, so every step's share of the rounded-up total is
exact (ceil(a + k MiB) = ceil(a) + k).  Where a call also allocates small buffers that together stay under 1 MiB (tone state, error
tiles and summary) the total may round up by one more MiB and by nothing else.  No free-memory query: other tenants of the device would
make it flaky, and the ledger's leak logic is proven without a GPU (tests/test_buffer_ledger.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def scene(rt):
    return rt.scenes.scene_mesh(20, 10, env_size=16)


def frame(rt, k, **kw):
    """frame k of a progressive render"""
    return rt.scenes.params_c2().replace(max_bounce=5, frames=k, random=1000 + 7 * k, **kw)


def test_every_step_adds_exactly_its_buffers(rt, scene):
    ctx = rt.host.Context(512, 512)
    ctx.upload_scene(scene)
    mb = lambda: ctx.get_option("device_mbytes")

    def step(label, call, added, slack=0):
        before = mb()
        call()
        got = mb() - before
        print(f"{label}: {before} -> {before + got} MiB")
        assert added <= got <= added + slack, f"{label}: {got} MiB more, expected {added}" + (f" (+{slack})" if slack else "")

    ctx.render(frame(rt, 1))
    ctx.render(frame(rt, 2))
    base = mb()
    step("aov, four planes", lambda: ctx.set_aov(15), 16)
    ctx.set_aov(0)
    assert mb() == base, "the planes' memory did not go with them"
    step("aov, four planes again", lambda: ctx.set_aov(15), 16)
    ctx.render(frame(rt, 1))
    step("read_image_u8", ctx.read_image_u8, 1)
    step("read_image_u8, second", ctx.read_image_u8, 0)
    step("denoise", ctx.denoise, 12)                          # the denoised buffer and two scratch buffers
    step("denoise, second", ctx.denoise, 0)
    step("denoise_guided", ctx.denoise_guided, 5)             # the variance buffer and one word per pixel; the other three are shared
    step("denoise_guided, second", ctx.denoise_guided, 0)
    step("temporal_accumulate", ctx.temporal_accumulate, 24)  # two each of history, position and normal
    step("temporal_accumulate, second", ctx.temporal_accumulate, 0)
    ctx.set_option("temporal_moments", 1)
    step("temporal_accumulate with moments", ctx.temporal_accumulate, 8)
    step("temporal_accumulate with moments, second", ctx.temporal_accumulate, 0)
    step("tonemap", ctx.tonemap, 1, slack=1)                  # the display buffer (+ the tone state)
    step("tonemap, second", ctx.tonemap, 0)
    step("error_estimate", ctx.error_estimate, 1, slack=1)    # the snapshot (+ tiles and summary)
    step("error_estimate, second", ctx.error_estimate, 0)
    ctx.close()


def same(a, b):
    """bit for bit (np.array_equal over the words: a NaN equals itself)"""
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def standalone(rt, k, max_bounce):
    """a frame that does not read the image before it"""
    return frame(rt, k, reset_flag=1).replace(frames=1, max_bounce=max_bounce)


def render_alone(rt, scene, width, height, frames, batch=1):
    ctx = rt.host.Context(width, height)
    ctx.upload_scene(scene)
    ctx.set_option("frame_batch", batch)
    for p in frames:
        ctx.render(p, sync=False)
    img = ctx.read_image()
    ctx.close()
    return img


@pytest.mark.parametrize("width,height", [(64, 64), (96, 64)], ids=["64x64", "96x64"])
def test_buffers_that_grow_between_frames_leave_the_images_alone(rt, scene, width, height):
    """Both growth paths on both sizes.  max_bounce 2 -> 9: the ray counts (device and pinned host) and the scan's work counters grow; the
    queues, the keep bits and the staging queue do not, at either size: they are sized by the rays of a frame, not by its depth.  What grows
    those is the batch: two frames in one set of launches behind single ones, on the same context, make them twice as long."""
    shallow, deep = standalone(rt, 1, 2), standalone(rt, 2, 9)
    pair = [frame(rt, 1, reset_flag=1), frame(rt, 2)]
    ctx = rt.host.Context(width, height)
    ctx.upload_scene(scene)
    ctx.set_option("frame_batch", 1)
    held = []
    ctx.render(shallow)
    first = ctx.read_image(); held.append(ctx.get_option("device_mbytes"))
    ctx.render(deep)
    second = ctx.read_image(); held.append(ctx.get_option("device_mbytes"))
    ctx.set_option("frame_batch", 2)
    for p in pair:
        ctx.render(p, sync=False)
    third = ctx.read_image(); held.append(ctx.get_option("device_mbytes"))
    ctx.close()
    print(f"{width} x {height}: device_mbytes {held}")
    assert held == sorted(held), f"device_mbytes shrank: {held}"
    assert same(first, render_alone(rt, scene, width, height, [shallow]))
    assert same(second, render_alone(rt, scene, width, height, [deep]))
    assert same(third, render_alone(rt, scene, width, height, pair, batch=2))
    assert not same(first, second) and not same(second, third)


def test_thirty_contexts_in_a_row(rt, scene):
    """every call of every context succeeds (a failure raises): what one context held is gone when the next one asks"""
    for k in range(30):
        ctx = rt.host.Context(64, 64)
        ctx.upload_scene(scene)
        ctx.set_aov(15)
        ctx.render(frame(rt, 1))
        ctx.denoise()
        ctx.tonemap()
        ctx.synchronize()
        ctx.close()
