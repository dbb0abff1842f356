"""Adaptive sampling on the device (include/rtgl_amd.h, "adaptive sampling").

The references are a second context's ordinary frames and the numpy restatement, tests/adaptive_mirror.py, pinned by
tests/test_adaptive_mirror.py.  Every comparison is of bits: a masked frame gives an active pixel the sample the ordinary frame with the
same uniforms gives it, and the merge and the update are defined operation by operation."""
import ctypes as C

import numpy as np
import pytest

import adaptive_mirror as am

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


def scenes(rt):
    sc = rt.scenes
    return {"c1": (sc.scene_c1(False), sc.params_c1()), "mesh": (sc.scene_mesh(10, 5, env_size=16), sc.params_c2())}


@pytest.fixture(scope="module")
def randoms(rt):
    g = rt.scenes.GlibcRand(0)
    return [g.rand() for _ in range(16)]


def context(rt, name, w, h, options=(), **kw):
    ctx = rt.host.Context(w, h, **kw)
    ctx.upload_scene(scenes(rt)[name][0])
    for key, value in options:
        ctx.set_option(key, value)
    return ctx


_samples = {}


def samples(rt, name, w, h, randoms):
    """the one-frame image of every random word (frames = 0, reset_flag = 1) from an ordinary context: computed once, never changed"""
    key = (name, w, h)
    if key not in _samples:
        ctx, base = context(rt, name, w, h), scenes(rt)[name][1]
        out = []
        for r in randoms[:8]:
            ctx.render(base.replace(frames=0, reset_flag=1, random=r))
            img = ctx.read_image()
            img.setflags(write=False)
            out.append(img)
        ctx.close()
        _samples[key] = out
    return _samples[key]


def records_counts(ctx):
    return ctx.read_adaptive_tiles()["samples"]


# ---------------------------------------------------------------------------------------------- 1. a full mask is the ordinary accumulation

@pytest.mark.parametrize("size", [(8, 8), (16, 16), (24, 40), (70, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", [("mesh", 1), ("mesh", 2), ("mesh", 4), ("c1", None)], ids=lambda c: f"{c[0]}-kernel{c[1]}")
def test_full_mask_frames_equal_ordinary_frames(rt, randoms, case, size):
    name, kernel = case
    w, h = size
    options = [("kernel", kernel)] if kernel is not None else []
    base = scenes(rt)[name][1]
    a, b = context(rt, name, w, h, options), context(rt, name, w, h, options)
    a.adaptive_begin()
    b.clear_image()
    for k in range(5):
        a.adaptive_frame(base.replace(frames=77, reset_flag=k % 2, random=randoms[k]))      # (frames and reset_flag are ignored)
        b.render(base.replace(frames=k, reset_flag=0, random=randoms[k]))
        assert same(a.read_image(), b.read_image()), f"frame {k}"
    assert a.get_option("kernel_in_use") == (kernel if kernel is not None else rt.host.KERNEL_WAVEFRONT)
    assert b.get_option("kernel_in_use") == (kernel if kernel is not None else rt.host.KERNEL_MEGA)
    s = a.adaptive_update()
    assert (records_counts(a)[am.tile_pixels(h, w) > 0] == 5).all() and s["samples_total"] == 5 * (w // 8 * 8) * (h // 8 * 8)
    assert a.last_frame_ms() > 0
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 2. explicit masks

def run_masks(rt, randoms, name, w, h, masks, options=()):
    """a session whose frame k runs under masks[k]: after every frame the image equals the mirror fed with the ordinary context's full
    samples; after the first, the active pixels are the ordinary reset frame's and the others are still zero"""
    base, smp = scenes(rt)[name][1], samples(rt, name, w, h, randoms)
    ctx, sess = context(rt, name, w, h, options), am.Session(h, w)
    ctx.adaptive_begin()
    for k, mask in enumerate(masks):
        ctx.adaptive_set_mask(mask)
        sess.set_mask(mask)
        assert (ctx.adaptive_get_mask() == sess.mask).all()
        ctx.adaptive_frame(base.replace(random=randoms[k]))
        sess.frame(smp[k])
        img = ctx.read_image()
        if k == 0:
            on = am.active_pixels(h, w, sess.mask)
            assert same(img[on][:, :3], smp[0][on][:, :3]) and (img[on][:, 3] == 1).all() and (bits(img[~on]) == 0).all()
        assert same(img, sess.image), f"frame {k}"
    ctx.adaptive_update()
    sess.update()
    assert (records_counts(ctx) == sess.n).all()
    ctx.close()


def tiles_mask(h, w, on):
    s = am.shape(h, w)
    m = np.zeros((s["ty"], s["tx"]), np.uint8)
    for ty, tx in on:
        m[ty, tx] = 1
    return m


def test_explicit_masks_on_the_mesh_scene(rt, randoms):
    w, h = 40, 56                                            # 3 x 4 tiles; column 2 holds 8 footprint columns, row 3 holds 8 footprint rows
    checker = (np.add.outer(np.arange(4), np.arange(3)) % 2).astype(np.uint8)
    single, edge, empty = tiles_mask(h, w, [(1, 1)]), tiles_mask(h, w, [(3, 2)]), tiles_mask(h, w, [])
    run_masks(rt, randoms, "mesh", w, h, [single, edge, checker, 1 - checker])
    run_masks(rt, randoms, "mesh", w, h, [edge, empty, checker, single])
    run_masks(rt, randoms, "mesh", w, h, [checker, checker, 1 - checker, np.ones((4, 3), np.uint8)])
    run_masks(rt, randoms, "c1", w, h, [checker, single, edge, 1 - checker])


def test_two_halves_of_equal_size_under_one_camera(rt, randoms):
    """left half, then right half: the same n0 and the same camera, other tiles -- what the key of the camera's kept bits cannot see"""
    w, h = 64, 32
    left = np.array([[1, 1, 0, 0]] * 2, np.uint8)
    run_masks(rt, randoms, "mesh", w, h, [left, 1 - left, left, 1 - left])


def test_a_half_mask_through_binned_and_culled_queues(rt, randoms):
    w, h = 128, 128
    half = np.zeros((8, 8), np.uint8)
    half[:, :4] = 1
    run_masks(rt, randoms, "mesh", w, h, [half, 1 - half], options=[("sort_min_rays", 0), ("cull", 3)])


# ---------------------------------------------------------------------------------------------- 3. the camera's kept bits

def test_a_session_leaves_the_kept_camera_bits_as_they_were(rt, randoms):
    """two ordinary frames, a session of masked frames, ordinary frames again: the same images, and as many lean camera bounces, as a
    context that cleared its image instead"""
    w, h = 64, 32
    base = scenes(rt)["mesh"][1]
    a, b = context(rt, "mesh", w, h), context(rt, "mesh", w, h)
    for ctx in (a, b):
        for k in range(2):
            ctx.render(base.replace(frames=k + 1, random=randoms[k]))
    lean = a.get_option("camera_lean_frames")
    assert lean == b.get_option("camera_lean_frames")
    left = np.array([[1, 1, 0, 0]] * 2, np.uint8)
    a.adaptive_begin()
    for k, mask in enumerate((left, 1 - left, left)):
        a.adaptive_set_mask(mask)
        a.adaptive_frame(base.replace(random=randoms[8 + k]))
    assert a.get_option("camera_lean_frames") == lean          # a masked frame never takes the lean camera bounce
    b.clear_image()
    for k in range(4):
        for ctx in (a, b):
            ctx.render(base.replace(frames=k, reset_flag=int(k == 0), random=randoms[2 + k]))
        assert same(a.read_image(), b.read_image()), f"frame {k} after the session"
    assert a.get_option("camera_lean_frames") == b.get_option("camera_lean_frames") > lean
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 4. the update

def inject(ctx, image):
    """copy `image` over the accumulation image through rtgl_device_image (which leaves the session open) and read it back"""
    import torch
    ptr = ctx.device_image_ptr()
    assert ptr
    image = np.ascontiguousarray(image, np.float32)
    torch.as_tensor(_DeviceArray(ptr, image.shape, "<f4"), device="cuda:0").copy_(torch.from_numpy(image))
    torch.cuda.synchronize()
    assert same(ctx.read_image(), image)


def special_image(rng, h, w):
    img = rng.random((h, w, 4), np.float32) * np.float32(2.0)
    flat = img.reshape(-1, 4)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -1.5, 0.0, -0.0, 3.0e38, -3.0e38, 1.0e-40, 2.0e19, 1.0e30)):
        flat[rng.integers(0, len(flat), 1 + len(flat) // 97), k % 3] = v
    return img


def check_update(ctx, sess, label):
    got, want = ctx.adaptive_update(), sess.update()
    rec = ctx.read_adaptive_tiles()
    assert rec.tobytes() == np.ascontiguousarray(sess.records).tobytes(), f"{label}: device {rec.ravel()}, mirror {sess.records.ravel()}"
    assert am.same_summary(got, want) == [], f"{label}: device {got}, mirror {want}"
    assert (ctx.adaptive_get_mask() == sess.mask).all(), label
    assert not np.isnan(rec["sum"]).any() and not np.isnan(rec["mse"]).any()


@pytest.mark.parametrize("size", [(8, 8), (24, 40), (70, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_update_on_injected_images_equals_the_mirror(rt, randoms, size):
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    params = dict(threshold=0.3, floor=0.01, min_samples=2, max_samples=6)
    ctx, sess = context(rt, "c1", w, h), am.Session(h, w, **params)
    base = scenes(rt)["c1"][1].replace(max_bounce=1)
    ctx.adaptive_begin(**params)
    check_update(ctx, sess, "no frame yet")
    nt = sess.mask.size
    for step in range(8):
        if step in (2, 5):                                   # tiles that sit a round out keep record and snapshot
            tiles = ((np.arange(nt) + step) % 2).reshape(sess.mask.shape)
            ctx.adaptive_set_mask(tiles)
            sess.set_mask(tiles)
        ctx.adaptive_frame(base.replace(random=randoms[step]))
        image = special_image(rng, h, w) if step % 3 == 2 else rng.random((h, w, 4), np.float32)
        if step == 6:
            image[..., :3] = np.where(am.active_pixels(h, w, sess.mask)[..., None], sess.image[..., :3], image[..., :3])     # nothing moved: mse 0, converged
        inject(ctx, image)
        sess.frame(image)                                    # (the counts move; the image is replaced)
        sess.image = image.copy()
        check_update(ctx, sess, f"step {step}")
        assert same(ctx.read_image(), image), "the update changed the image"
    ctx.close()


@pytest.mark.parametrize("extra", [False, True], ids=["on", "one-ulp-above"])
def test_a_tile_on_the_threshold(rt, randoms, extra):
    """8 x 8, n = 2 m, den = 1: mse = 2^-12 = threshold^2 exactly is converged, one ulp above is not (tests/test_adaptive_mirror.py)"""
    params = dict(threshold=1.0 / 64, floor=0.5, min_samples=1, max_samples=100)
    ctx, sess = context(rt, "c1", 8, 8), am.Session(8, 8, **params)
    base = scenes(rt)["c1"][1].replace(max_bounce=1)
    ctx.adaptive_begin(**params)
    first = np.full((8, 8, 4), 0.5, np.float32)
    first[0, 0, :3] = 0.375
    if extra:
        first[3, 5, :3] = np.float32(0.5) - np.float32(0.75 * 2.0 ** -14)
    for k, image in enumerate((first, np.full((8, 8, 4), 0.5, np.float32))):
        ctx.adaptive_frame(base.replace(random=randoms[k]))
        inject(ctx, image)
        sess.frame(image)
        sess.image = image.copy()
        check_update(ctx, sess, f"update {k}")
    r = ctx.read_adaptive_tiles()[0, 0]
    want = np.float32(2.0 ** -12) if not extra else np.nextafter(np.float32(2.0 ** -12), np.float32(1.0))
    assert bits(r["mse"]) == bits(want) and r["converged"] == int(not extra) and r["count"] == 64
    ctx.close()


def test_render_adaptive_on_the_sphere_scene(rt):
    sc = rt.scenes
    r = rt.host.HeadlessRenderer(64, 64)
    r.set_scene(sc.scene_c1(False))
    r.params = sc.params_c1()
    frames, s = r.render_adaptive(0.05, 512)
    rec = r.ctx.read_adaptive_tiles()
    print(f"render_adaptive: {frames} frames, per-tile samples {s['samples_min']} .. {s['samples_max']}, {s['samples_total']} samples")
    assert s["converged"] == 1 and frames > 0 and not r.ctx.adaptive_get_mask().any()
    assert (am.done(rec) | (rec["samples"] >= 512)).all() and s["tiles_converged"] + s["tiles_capped"] == 16
    assert s["samples_min"] < s["samples_max"] == frames
    r.ctx.close()


# ---------------------------------------------------------------------------------------------- 5. session rules and errors

def test_every_ending_event_and_every_refusal(rt, randoms):
    import torch
    w, h = 24, 40
    ctx = context(rt, "mesh", w, h)
    lib, base = ctx.lib, scenes(rt)["mesh"][1]
    s, mask = rt.host.CAdaptiveSummary(), np.ones((3, 2), np.uint8)
    own = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")

    def no_session(label):
        assert lib.rtgl_adaptive_frame(ctx.h) == ERR_STATE, label
        assert lib.rtgl_adaptive_update(ctx.h, C.byref(s)) == ERR_STATE, label
        assert lib.rtgl_adaptive_set_mask(ctx.h, mask.ctypes.data_as(C.c_void_p)) == ERR_STATE, label
        assert lib.rtgl_adaptive_get_mask(ctx.h, mask.ctypes.data_as(C.c_void_p)) == ERR_STATE, label

    no_session("before the first begin")
    assert not ctx.device_adaptive_tiles_ptr()
    ctx.adaptive_begin()
    assert lib.rtgl_adaptive_frame(ctx.h) == ERR_STATE          # no frame parameters yet
    ctx.set_params(base.replace(random=randoms[0]))
    events = [("rtgl_render_frame", lambda: ctx.render(base.replace(frames=1, random=randoms[1]))), ("rtgl_clear_image", ctx.clear_image),
              ("rtgl_write_image_f32", lambda: ctx.write_image(np.zeros((h, w, 4), np.float32))),
              ("rtgl_bind_device_image", lambda: ctx.bind_device_image(own.data_ptr())), ("rtgl_bind_device_image(NULL)", lambda: ctx.bind_device_image(0))]
    for name, event in events:
        ctx.adaptive_begin()
        ctx.adaptive_frame(base.replace(random=randoms[0]))
        event()
        no_session(name)
    assert ctx.device_adaptive_tiles_ptr() and ctx.read_adaptive_tiles().shape == (3, 2)      # the records stay readable
    # refusals inside a session
    ctx.adaptive_begin()
    for key in ("aov", "rng_state"):
        ctx.set_option(key, 1)
        assert lib.rtgl_adaptive_frame(ctx.h) == ERR_STATE, key
        ctx.set_option(key, 0)
    ctx.set_params(base.replace(samples=2))
    assert lib.rtgl_adaptive_frame(ctx.h) == ERR_INVALID
    ctx.set_params(base.replace(max_bounce=0))
    assert lib.rtgl_adaptive_frame(ctx.h) == ERR_INVALID
    assert lib.rtgl_adaptive_update(ctx.h, None) == ERR_INVALID and lib.rtgl_adaptive_set_mask(ctx.h, None) == ERR_INVALID
    assert lib.rtgl_adaptive_get_mask(ctx.h, None) == ERR_INVALID and lib.rtgl_read_adaptive_tiles(ctx.h, None, None, None) == ERR_INVALID
    p = rt.host.CAdaptiveParams()
    lib.rtgl_adaptive_defaults(C.byref(p))
    p.max_samples = 8
    assert lib.rtgl_adaptive_begin(ctx.h, C.byref(p)) == ERR_INVALID and lib.rtgl_adaptive_begin(ctx.h, None) == ERR_INVALID
    ctx.adaptive_frame(base.replace(random=randoms[0]))          # a refused begin leaves the session as it was
    ctx.close()


def test_tiled_and_multi_device_contexts_are_refused(rt):
    for kw in (dict(rank=0, world=2, strip_rows=8), dict(devices=[0, 0], strip_rows=8)):
        ctx = rt.host.Context(32, 32, **kw)
        p = rt.host.CAdaptiveParams()
        ctx.lib.rtgl_adaptive_defaults(C.byref(p))
        assert ctx.lib.rtgl_adaptive_begin(ctx.h, C.byref(p)) == ERR_STATE, kw
        assert ctx.lib.rtgl_adaptive_frame(ctx.h) == ERR_STATE, kw
        ctx.close()


def test_frames_held_by_a_batching_context_are_submitted_first(rt, randoms):
    w, h = 24, 40
    base = scenes(rt)["mesh"][1]
    a, b = context(rt, "mesh", w, h, [("frame_batch", 8)]), context(rt, "mesh", w, h)
    for ctx in (a, b):
        for k in range(3):                                   # (held by `a`)
            ctx.render(base.replace(frames=k, random=randoms[k]), sync=False)
        ctx.adaptive_begin()                                 # submits them, then clears the image
        for k in range(3):
            ctx.adaptive_frame(base.replace(random=randoms[4 + k]), sync=False)
    assert same(a.read_image(), b.read_image())
    smp, sess = samples(rt, "mesh", w, h, randoms), am.Session(h, w)
    for k in range(3):
        sess.frame(smp[4 + k])
    assert same(a.read_image(), sess.image)
    for ctx in (a, b):                                       # an ordinary frame ends the session even while it is only held
        ctx.render(base.replace(frames=3, random=randoms[3]), sync=False)
        assert ctx.lib.rtgl_adaptive_frame(ctx.h) == ERR_STATE
    assert same(a.read_image(), b.read_image())
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 6. other buffers

def test_a_session_leaves_every_other_buffer_alone(rt, randoms):
    w, h = 32, 32
    H_ = rt.host
    base = scenes(rt)["mesh"][1]
    ctx = context(rt, "mesh", w, h, [("aov", H_.AOV_ALL), ("rng_state", 1)])
    for k in range(3):
        ctx.render(base.replace(frames=k + 1, random=randoms[k]))
        if k:
            ctx.error_estimate()
    ctx.denoise()
    ctx.temporal_accumulate()
    ctx.tonemap()

    def others():
        return dict(denoised=ctx.read_denoised(), temporal=ctx.read_temporal(), display=ctx.read_display(), rng=ctx.read_rng_state(),
                    error_tiles=ctx.read_error_tiles(), error_summary=repr(ctx.read_error_summary()))
    planes = lambda: [ctx.read_aov(p) for p in (H_.AOV_ALBEDO, H_.AOV_NORMAL, H_.AOV_POSITION, H_.AOV_IDS)]
    before, planes_before = others(), planes()
    ctx.adaptive_begin()
    assert ctx.lib.rtgl_adaptive_frame(ctx.h) == ERR_STATE       # the planes are on
    ctx.adaptive_update()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(planes(), planes_before))
    ctx.set_option("aov", 0)
    ctx.set_option("rng_state", 0)
    ctx.adaptive_begin(min_samples=1, max_samples=4)
    for k in range(3):
        ctx.adaptive_frame(base.replace(random=randoms[4 + k]))
        ctx.adaptive_update()
    ctx.set_option("rng_state", 1)
    after = others()
    for key in before:
        a, b = before[key], after[key]
        assert (a == b) if isinstance(a, str) else (a.tobytes() == b.tobytes()), key
    ctx.close()


def test_device_memory_grows_only_when_a_session_begins(rt, randoms):
    w, h = 70, 53
    base = scenes(rt)["mesh"][1]
    a, b = context(rt, "mesh", w, h), context(rt, "mesh", w, h)
    steps = {id(a): [], id(b): []}
    for ctx in (a, b):
        steps[id(ctx)].append(ctx.get_option("device_mbytes"))
        for k in range(2):
            ctx.render(base.replace(frames=k + 1, random=randoms[k]))
            steps[id(ctx)].append(ctx.get_option("device_mbytes"))
    assert steps[id(a)] == steps[id(b)]
    b.adaptive_begin()
    s = am.shape(h, w)
    tiles, blocks = s["ty"] * s["tx"], s["blocks_x"] * s["blocks_y"]
    added = w * h * (16 + 4) + tiles * (32 + 8) + (blocks + tiles) * 4
    grown = b.get_option("device_mbytes") - steps[id(b)][-1]
    assert 0 <= grown <= (added + (1 << 20) - 1) >> 20
    assert a.get_option("device_mbytes") == steps[id(a)][-1]
    a.close()
    b.close()
