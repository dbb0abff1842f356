"""rtgl_tonemap on the device (include/rtgl_amd.h, "display transform").

The reference is the numpy restatement, tests/tonemap_mirror.py, pinned by tests/test_tonemap_mirror.py.  Every output is an integer or an
exposure that is never a NaN, so the comparison is exact and has no budget: the display bytes, the 256 bins, `ignored`, and the bits of
the exposure."""
import ctypes as C

import numpy as np
import pytest

import golden_cases as gc
import tonemap_inputs as ti
import tonemap_mirror as tm

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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and (bits(a) == bits(b)).all()


def compare(ctx, want, label):
    """the context's read-outs after a call against the mirror's dict"""
    disp = ctx.read_display()
    wrong = np.argwhere((disp != want["display"]).any(-1))
    assert len(wrong) == 0, f"{label}: {len(wrong)} pixels differ, first at {wrong[0]}: device {disp[tuple(wrong[0])]}, mirror {want['display'][tuple(wrong[0])]}"
    e = ctx.read_tonemap_exposure()
    assert bits(e) == bits(want["exposure"]), f"{label}: exposure {float(e)!r}, mirror {float(want['exposure'])!r}"
    if want["hist"] is not None:
        hist, ignored = ctx.read_tonemap_histogram()
        assert (hist == want["hist"]).all() and ignored == want["ignored"], f"{label}: histogram differs in bins {np.nonzero(hist != want['hist'])[0]}, ignored {ignored} / {want['ignored']}"
        assert int(hist.sum()) + ignored == disp.shape[0] * disp.shape[1]


@pytest.mark.parametrize("size", ti.SIZES, ids=[f"{w}x{h}" for h, w in ti.SIZES])
def test_every_family_operator_and_exposure_mode_is_bit_identical_to_the_mirror(size, rt):
    h, w = size
    ctx = rt.host.Context(w, h)
    for name in ti.FAMILIES:
        img = ti.family(name, h, w)
        ctx.write_image(img)
        for params in ti.parameter_sets():
            ctx.tonemap(**params)
            compare(ctx, tm.tonemap(img, **params), f"{name} {w} x {h} {params}")
        assert same(ctx.read_image(), img), f"{name}: the calls changed the image"
    ctx.close()


_full = {}


def full_case():
    """the one 1080p picture and its mirror result, computed once"""
    if not _full:
        h, w = ti.FULL
        img = ti.hdr(h, w)
        img[:7] = ti.specials(7, w)
        img[7:9] = ti.bin_edges(2, w)
        _full["img"] = img
        _full["auto"] = tm.tonemap(img)
        _full["manual"] = tm.tonemap(img, op=2, auto=False, exposure=0.5)
    return _full


def test_a_1080p_picture_with_many_blocks_adding_to_the_same_bins(rt):
    case = full_case()
    h, w = ti.FULL
    ctx = rt.host.Context(w, h)
    ctx.write_image(case["img"])
    ctx.tonemap()
    compare(ctx, case["auto"], "1080p defaults")
    first = ctx.read_display()
    ctx.tonemap()                                                      # a second identical call: the other histogram set, the same answer
    compare(ctx, case["auto"], "1080p defaults, second call")
    assert (ctx.read_display() == first).all()
    ctx.tonemap(op=2, auto=False, exposure=0.5)
    compare(ctx, case["manual"], "1080p manual ACES")
    hist, ignored = ctx.read_tonemap_histogram()                       # a manual call leaves the histogram of the latest auto call readable
    assert (hist == case["auto"]["hist"]).all() and ignored == case["auto"]["ignored"]
    assert (ctx.read_display(flip=True) == case["manual"]["display"][::-1]).all()
    assert same(ctx.read_image(), case["img"])
    ctx.close()


def test_adapt_over_a_sequence_with_a_reset_in_the_middle(rt):
    h, w = 131, 200
    dark, bright = ti.hdr(h, w), ti.hdr(h, w)
    bright[..., :3] *= np.float32(16.0)
    ctx = rt.host.Context(w, h)
    mirror = tm.Tonemapper()
    seen = []
    for k, img in enumerate([dark, bright, bright, bright, bright]):
        if k == 3:
            ctx.tonemap_reset(); mirror.reset()
        ctx.write_image(img)
        ctx.tonemap(adapt=0.25)
        want = mirror(img, adapt=0.25)
        compare(ctx, want, f"adapt 0.25, call {k}")
        seen.append(float(want["exposure"]))
    assert seen[0] > seen[1] > seen[2] > seen[3] == seen[4]            # two steps towards the brighter picture's exposure, then the reset jumps there
    # a manual call in between neither reads nor replaces the stored exposure
    ctx.tonemap(auto=False, exposure=3.0)
    compare(ctx, mirror(bright, auto=False, exposure=3.0), "manual between auto calls")
    ctx.write_image(dark)
    ctx.tonemap(adapt=0.5)
    compare(ctx, mirror(dark, adapt=0.5), "adapt 0.5 after a manual call")
    ctx.close()


def test_flip_and_the_device_pointer(rt):
    import torch
    h, w = 5, 7
    img = ti.hdr(h, w)
    ctx = rt.host.Context(w, h)
    assert ctx.device_display_ptr() == 0
    ctx.write_image(img)
    ctx.tonemap()
    want = tm.tonemap(img)["display"]
    assert (ctx.read_display() == want).all() and (ctx.read_display(flip=True) == want[::-1]).all()
    assert (ctx.read_display(flip=False) == want).all()                # the flip is the read-out's, the buffer keeps the image's order
    ptr = ctx.device_display_ptr()
    assert ptr
    ctx.synchronize()
    t = torch.as_tensor(_DeviceArray(ptr, (h, w, 4), "|u1"), device="cuda:0")
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == want).all()
    ctx.tonemap(op=0)                                                  # the next call writes the same buffer
    assert ctx.device_display_ptr() == ptr
    ctx.close()


def test_denoised_and_temporal_sources_after_their_calls_on_a_rendered_frame(rt):
    sc, H_ = rt.scenes, rt.host
    w, h = 96, 64
    ctx = H_.Context(w, h)
    ctx.set_aov(H_.AOV_ALBEDO | H_.AOV_NORMAL | H_.AOV_POSITION)
    ctx.upload_scene(sc.scene_mesh(10, 5, env_size=16))
    for p in gc.frame_sequence(sc, sc.params_c2(), 2):
        ctx.render(p)
    for source in (1, 2):                                              # the buffer does not exist yet
        with pytest.raises(H_.RtglError, match=r"\(-4\)"):
            ctx.tonemap(source=source)
    with pytest.raises(H_.RtglError, match=r"\(-4\)"):
        ctx.read_display()
    ctx.denoise_guided()
    ctx.temporal_accumulate()
    image, denoised, history = ctx.read_image(), ctx.read_denoised(), ctx.read_temporal()
    planes = [ctx.read_aov(k) for k in (H_.AOV_ALBEDO, H_.AOV_NORMAL, H_.AOV_POSITION)]
    assert not same(image, denoised)
    for source, buf in ((0, image), (1, denoised), (2, history)):
        for params in (dict(), dict(op=2), dict(op=0, auto=False, exposure=0.7)):
            ctx.tonemap(source=source, **params)
            compare(ctx, tm.tonemap(buf, **params), f"source {source} {params}")
    assert same(ctx.read_image(), image) and same(ctx.read_denoised(), denoised) and same(ctx.read_temporal(), history)
    assert all(same(ctx.read_aov(k), a) for k, a in zip((H_.AOV_ALBEDO, H_.AOV_NORMAL, H_.AOV_POSITION), planes))
    ctx.close()


def test_state_and_argument_errors_on_a_live_context(rt):
    H_ = rt.host
    lib = H_.load_library()
    ctx = H_.Context(16, 16)
    e, hist, ign = C.c_float(), (C.c_uint32 * 256)(), C.c_uint32()
    assert lib.rtgl_read_tonemap_exposure(ctx.h, C.byref(e)) == ERR_STATE
    assert lib.rtgl_read_tonemap_histogram(ctx.h, hist, C.byref(ign)) == ERR_STATE
    assert lib.rtgl_tonemap(ctx.h, None) == 0                          # NULL: the defaults
    assert lib.rtgl_read_display_u8(ctx.h, None, 0) == ERR_INVALID
    assert lib.rtgl_read_tonemap_exposure(ctx.h, None) == ERR_INVALID
    assert lib.rtgl_read_tonemap_histogram(ctx.h, None, None) == ERR_INVALID
    assert lib.rtgl_read_tonemap_histogram(ctx.h, hist, None) == 0     # `ignored` may be NULL
    p = H_.CTonemapParams()
    lib.rtgl_tonemap_defaults(C.byref(p))
    for field, value in (("source", 3), ("op", 3), ("flags", 2), ("adapt", 1.5), ("key", float("nan")), ("high_permille", 900)):
        q = H_.CTonemapParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert lib.rtgl_tonemap(ctx.h, C.byref(q)) == ERR_INVALID, field
    ctx.close()
    tiled = H_.Context(32, 32, rank=0, world=2, strip_rows=8)
    assert lib.rtgl_tonemap(tiled.h, None) == ERR_STATE
    assert b"tiled" in lib.rtgl_last_error(tiled.h)
    tiled.close()
