"""Robust accumulation on the device (include/rtgl_amd.h, "robust accumulation").

The references are the numpy restatement, tests/robust_mirror.py, pinned by tests/test_robust_mirror.py, and a second context's ordinary
accumulation.  Every comparison is exact: the fold and the resolve are defined operation by operation, so every word the device writes
equals the mirror's, and where the mirror has a NaN the device has one (no budget of differing NaNs).  The one thing the contract leaves
open is a NaN's sign and payload, which differ between processors: `words` maps every NaN to one word before comparing."""
import ctypes as C

import numpy as np
import pytest

import robust_inputs as ri
import robust_mirror as rm

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


def words(a):
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same(a, b):
    return a.shape == b.shape and bool((words(a) == words(b)).all())


def check_session(ctx, sess, gains, label, last):
    """all bucket planes, both destinations and the G plane of a device session against the mirror's; `last`: the image as the last
    write left it, which a resolve into the buffer must not touch"""
    assert ctx.robust_frames() == (sess.N, sess.K), label
    for j in range(sess.K):
        assert same(ctx.read_robust_bucket(j), sess.planes[j]), f"{label}: bucket {j}"
    for gain in gains:
        ctx.robust_resolve(gain=gain)
        want = sess.resolve(gain, rm.DEST_BUFFER)
        got = ctx.read_robust()
        assert same(got[..., 3], want[..., 3]), f"{label} gain {gain}: the G plane"
        assert same(got, want), f"{label} gain {gain}: the output plane"
        assert same(ctx.read_image(), last), f"{label} gain {gain}: a resolve into the buffer changed the image"
        ctx.robust_resolve(gain=gain, dest=rm.DEST_IMAGE)
        assert same(ctx.read_image(), sess.resolve(gain, rm.DEST_IMAGE)), f"{label} gain {gain}: the image"
        assert same(ctx.read_robust(), want), f"{label} gain {gain}: a resolve into the image changed the output plane"
        ctx.write_image(last)


def run_injected(ctx, samples, K, gains, label):
    h, w = samples[0].shape[:2]
    sess = rm.Session(h, w, K)
    ctx.robust_begin(buckets=K)
    for s in samples:
        ctx.write_image(s)
        ctx.robust_accumulate()
        sess.accumulate(s)
    check_session(ctx, sess, gains, label, samples[-1])


# ---------------------------------------------------------------------------------------------- 1. injected samples

@pytest.mark.parametrize("K", ri.BUCKETS)
@pytest.mark.parametrize("size", ri.GPU_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_injected_families_equal_the_mirror(rt, size, K):
    """every family of tests/robust_inputs.py: write_image, then robust_accumulate, per sample; one context, a session per family"""
    w, h = size
    ctx = rt.host.Context(w, h)
    for family in ri.FAMILIES:
        case = ri.make(family, h, w, K)
        run_injected(ctx, case["samples"], K, case["gains"], f"{family} {w} x {h} K = {K}")
    ctx.robust_end()
    ctx.close()


def test_a_full_hd_session(rt):
    """1920 x 1080, K = 8, N = 9: more than one wave of blocks, the last block partly filled (2,073,600 = 8100 x 256), bucket 0 twice"""
    w, h, K = 1920, 1080, 8
    samples = ri.noisy(np.random.default_rng(1080), h, w, 9)
    ctx = rt.host.Context(w, h)
    run_injected(ctx, samples, K, [1.0], "1920 x 1080")
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. rendered frames

@pytest.fixture(scope="module")
def randoms(rt):
    g = rt.scenes.GlibcRand(0)
    return [g.rand() for _ in range(24)]


def rendering_context(rt, w, h, options=(), **kw):
    ctx = rt.host.Context(w, h, **kw)
    ctx.upload_scene(rt.scenes.scene_c1(True))
    for key, value in options:
        ctx.set_option(key, value)
    return ctx


@pytest.fixture(scope="module")
def rendered(rt, randoms):
    """scene_c1(True), 64 x 64, K = 8, N = 20: (the context with its open session, the one-frame images it folded, the mirror's session);
    rendered once, shared; the tests only read the buckets"""
    base, K, N = rt.scenes.params_c1(), 8, 20
    ctx, sess, ones = rendering_context(rt, 64, 64), rm.Session(64, 64, K), []
    ctx.robust_begin(buckets=K)
    for k in range(N):
        ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)
        ctx.robust_accumulate()
        one = ctx.read_image()
        one.setflags(write=False)
        ones.append(one)
        sess.accumulate(one)
    yield ctx, ones, sess
    ctx.close()


def test_a_bucket_is_the_ordinary_accumulation_of_its_frames(rt, randoms, rendered):
    ctx, ones, sess = rendered
    base = rt.scenes.params_c1()
    other = rendering_context(rt, 64, 64)
    for j in range(sess.K):
        for i, k in enumerate(range(j, sess.N, sess.K)):
            other.render(base.replace(frames=i, reset_flag=int(i == 0), random=randoms[k]))
        assert same(ctx.read_robust_bucket(j), other.read_image()), f"bucket {j}"
    other.close()


def test_the_rendered_resolve_equals_the_mirror(rt, randoms, rendered):
    ctx, ones, sess = rendered
    assert (ones[0][..., 3] == 1).all() and any(not same(ones[0], o) for o in ones[1:])
    check_session(ctx, sess, [1.0, 0.0, 2.5], "rendered", ones[-1])
    ctx.robust_resolve()
    trimmed = rm.resolve(sess.planes, sess.N, 1.0)[2] > 0
    assert 0 < trimmed.sum() < trimmed.size                        # the lit scene has fireflies, and not everywhere


def test_render_robust_of_the_headless_renderer(rt):
    sc = rt.scenes
    a, b = rt.host.HeadlessRenderer(64, 64), rt.host.HeadlessRenderer(64, 64)
    sess = rm.Session(64, 64, 4)
    for r in (a, b):
        r.set_scene(sc.scene_c1(True))
        r.params = sc.params_c1()
    g = sc.GlibcRand(0)
    stream = [g.rand() for _ in range(20)]
    for k in range(9):
        b.ctx.render(b.params.replace(frames=0, reset_flag=1, random=stream[k]))
        sess.accumulate(b.ctx.read_image())
    got = a.render_robust(9, buckets=4, gain=2.0)
    assert same(got, sess.resolve(2.0)) and a.ctx.robust_frames() == (9, 4)
    assert same(a.ctx.read_image(), b.ctx.read_image())            # the image still holds the last frame
    # the session drew nine words and left the loop's counters alone, as renderer.h's robust_frame() does
    assert (a.m_frames, a.m_reset) == (0, False) and a._rand.rand() == stream[9]
    a.reset_buffer()
    sess2 = rm.Session(64, 64, 4)
    for k in range(10, 19):
        b.ctx.render(b.params.replace(frames=0, reset_flag=1, random=stream[k]))
        sess2.accumulate(b.ctx.read_image())
    got = a.render_robust(9, buckets=4, gain=2.0, to_image=True)
    assert same(got, sess2.resolve(2.0, rm.DEST_IMAGE)) and same(a.ctx.read_image(), got)
    assert not same(sess2.resolve(2.0), sess.resolve(2.0))         # (other words, another picture)
    assert (a.m_frames, a.m_reset) == (0, True)                     # the pending reset is still pending ...
    p = a.render_frame()
    assert (p.frames, p.reset_flag, p.random) == (1, 1, stream[19]) and (a.m_frames, a.m_reset) == (0, False)      # ... for the next ordinary frame
    b.ctx.render(b.params.replace(frames=1, reset_flag=1, random=stream[19]))
    assert same(a.ctx.read_image(), b.ctx.read_image())
    with pytest.raises(ValueError):
        a.render_robust(0)
    a.ctx.close()
    b.ctx.close()


# ---------------------------------------------------------------------------------------------- 3. dest = IMAGE

def test_a_resolve_into_the_image_is_a_write_of_the_image(rt, randoms):
    """read_image is the buffer resolve's rgb with w = 1; denoise and tonemap take the picture as they take one that write_image put"""
    H_ = rt.host
    base = rt.scenes.params_c1()
    a, b = (rendering_context(rt, 64, 64, [("aov", H_.AOV_ALL)]) for _ in range(2))
    a.robust_begin(buckets=8)
    for k in range(12):
        for ctx in (a, b):
            ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)
        a.robust_accumulate()
    a.robust_resolve()
    out = a.read_robust()
    a.robust_resolve(dest=rm.DEST_IMAGE)
    img = a.read_image()
    assert same(img[..., :3], out[..., :3]) and (words(img[..., 3]) == words(f32(1))).all()
    b.write_image(img)
    for ctx in (a, b):
        ctx.denoise()
        ctx.tonemap()
    assert same(a.read_denoised(), b.read_denoised()) and (a.read_display() == b.read_display()).all()
    assert a.read_display()[..., :3].any()
    a.close()
    b.close()


def test_a_resolve_into_the_image_ends_an_adaptive_session(rt, randoms):
    base = rt.scenes.params_c1()
    ctx = rendering_context(rt, 64, 64)
    ctx.adaptive_begin()
    ctx.adaptive_frame(base.replace(random=randoms[0]))
    ctx.robust_begin()
    ctx.robust_accumulate()
    ctx.robust_resolve()
    ctx.adaptive_frame(base.replace(random=randoms[1]))            # begin, accumulate and a resolve into the buffer leave the session open
    ctx.robust_accumulate()
    ctx.robust_resolve(dest=rm.DEST_IMAGE)
    assert ctx.lib.rtgl_adaptive_frame(ctx.h) == ERR_STATE
    ctx.close()


@pytest.mark.parametrize("event", ["buffer", "image", "write_image"])
def test_the_error_estimate_sees_a_new_epoch_after_a_resolve_into_the_image(rt, randoms, event):
    """a snapshot after frame 1, an estimate after frame 2; then the event and frame 3: the estimate is valid again after a session that
    resolved into the buffer, and a first call again (not valid) after a resolve into the image, as after rtgl_write_image_f32"""
    base = rt.scenes.params_c1()
    ctx = rendering_context(rt, 64, 64)
    for k in (1, 2):
        ctx.render(base.replace(frames=k, random=randoms[k]))
        ctx.error_estimate()
    assert ctx.read_error_summary()["valid"] == 1
    image = ctx.read_image()
    ctx.robust_begin(buckets=4)
    ctx.robust_accumulate()
    if event == "write_image":
        ctx.write_image(image)
    else:
        ctx.robust_resolve(gain=0.0, dest=rm.DEST_IMAGE if event == "image" else rm.DEST_BUFFER)
    assert same(ctx.read_image(), image)                           # (one frame in one bucket, gain 0: the image itself, w = 1)
    ctx.render(base.replace(frames=3, random=randoms[3]))
    ctx.error_estimate()
    assert ctx.read_error_summary()["valid"] == (1 if event == "buffer" else 0)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 4. other contexts and states

def test_a_tiled_context_works_on_its_strips(rt, randoms, rendered):
    """rank 1 of world 2 at 64 x 64: the rows rtgl_local_row_to_global names, equal to the untiled result"""
    ctx, ones, sess = rendered
    base = rt.scenes.params_c1()
    tiled = rendering_context(rt, 64, 64, rank=1, world=2, strip_rows=8)
    rows = tiled.global_rows()
    assert len(rows) == 32 and rows[0] == 8 and (rows != np.arange(32)).any()
    tiled.robust_begin(buckets=sess.K)
    for k in range(sess.N):
        tiled.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)
        tiled.robust_accumulate()
    for j in range(sess.K):
        assert same(tiled.read_robust_bucket(j), sess.planes[j][rows]), f"bucket {j}"
    tiled.robust_resolve()
    ctx.robust_resolve()
    assert same(tiled.read_robust(), ctx.read_robust()[rows]) and same(tiled.read_robust(), sess.resolve()[rows])
    tiled.robust_resolve(dest=rm.DEST_IMAGE)
    assert same(tiled.read_image(), sess.resolve(dest=rm.DEST_IMAGE)[rows])
    # injected: rows of special values
    case = ri.make("specials", 64, 64, 16)
    local = [np.ascontiguousarray(s[rows]) for s in case["samples"]]
    run_injected(tiled, local, 16, case["gains"], "tiled specials")
    tiled.close()


def test_a_multi_device_context_is_refused(rt):
    ctx = rt.host.Context(32, 32, devices=[0, 0], strip_rows=8)
    p = rt.host.CRobustParams()
    ctx.lib.rtgl_robust_defaults(C.byref(p), None)
    assert ctx.lib.rtgl_robust_begin(ctx.h, C.byref(p)) == ERR_STATE
    assert b"multi-device" in ctx.lib.rtgl_last_error(ctx.h)
    assert ctx.lib.rtgl_robust_accumulate(ctx.h) == ERR_STATE
    ctx.close()


def test_frames_held_by_a_batching_context_are_submitted_first(rt, randoms):
    base = rt.scenes.params_c1()
    a, b = rendering_context(rt, 24, 40, [("frame_batch", 8)]), rendering_context(rt, 24, 40)
    for ctx in (a, b):
        ctx.robust_begin(buckets=4)
        for k in range(3):                                   # (held by `a`)
            ctx.render(base.replace(frames=k, reset_flag=int(k == 0), random=randoms[k]), sync=False)
        ctx.robust_accumulate()                              # submits them, then folds the image of three frames
    assert same(a.read_robust_bucket(0), b.read_robust_bucket(0)) and same(a.read_robust_bucket(0), b.read_image())
    assert a.read_robust_bucket(0)[:40, :24, :3].any()
    a.close()
    b.close()


def test_two_contexts_take_turns(rt):
    sizes, Ks = [(17, 17), (70, 53)], [16, 4]
    ctxs = [rt.host.Context(w, h) for w, h in sizes]
    cases = [ri.make("ragged", h, w, K) for (w, h), K in zip(sizes, Ks)]
    sessions = [rm.Session(h, w, K) for (w, h), K in zip(sizes, Ks)]
    for ctx, K in zip(ctxs, Ks):
        ctx.robust_begin(buckets=K)
    for k in range(max(len(c["samples"]) for c in cases)):
        for ctx, case, sess in zip(ctxs, cases, sessions):
            if k < len(case["samples"]):
                ctx.write_image(case["samples"][k])
                ctx.robust_accumulate()
                sess.accumulate(case["samples"][k])
    for ctx, case, sess in zip(ctxs, cases, sessions):
        check_session(ctx, sess, case["gains"], "turns", case["samples"][-1])
        ctx.close()


def test_states_and_refusals_on_a_live_context(rt):
    H_ = rt.host
    w, h = 17, 17
    ctx = H_.Context(w, h)
    lib = ctx.lib
    p, r = H_.CRobustParams(), H_.CRobustResolveParams()
    lib.rtgl_robust_defaults(C.byref(p), C.byref(r))
    n, k = C.c_uint32(), C.c_uint32()
    px = np.zeros((h, w, 4), f32)
    out = px.ctypes.data_as(C.c_void_p)

    def no_session(label):
        assert lib.rtgl_robust_accumulate(ctx.h) == ERR_STATE, label
        assert lib.rtgl_robust_resolve(ctx.h, C.byref(r)) == ERR_STATE, label
        assert lib.rtgl_robust_end(ctx.h) == ERR_STATE, label
        assert lib.rtgl_robust_frames(ctx.h, C.byref(n), C.byref(k)) == ERR_STATE, label
        assert lib.rtgl_read_robust_f32(ctx.h, out) == ERR_STATE, label
        assert lib.rtgl_read_robust_bucket_f32(ctx.h, 0, out) == ERR_STATE, label
        assert b"no session" in lib.rtgl_last_error(ctx.h), label

    no_session("before the first begin")
    ctx.robust_begin()
    assert ctx.robust_frames() == (0, 8)
    assert lib.rtgl_robust_resolve(ctx.h, C.byref(r)) == ERR_STATE          # N = 0
    assert lib.rtgl_read_robust_f32(ctx.h, out) == ERR_STATE                # no resolve yet
    assert not ctx.read_robust_bucket(7).any()                              # zeroed
    # invalid arguments; a refused call leaves the session as it was
    assert lib.rtgl_robust_begin(ctx.h, None) == ERR_INVALID and lib.rtgl_robust_resolve(ctx.h, None) == ERR_INVALID
    for buckets in (0, 1, 2, 3, 5, 12, 17, 32):
        bad = H_.CRobustParams(buckets=buckets)
        assert lib.rtgl_robust_begin(ctx.h, C.byref(bad)) == ERR_INVALID, buckets
    for kw in (dict(flags=1), dict(reserved=(0, 0, 0, 0, 0, 1))):
        assert lib.rtgl_robust_begin(ctx.h, C.byref(H_.CRobustParams(buckets=8, **kw))) == ERR_INVALID, kw
    ctx.write_image(np.full((h, w, 4), 0.5, f32))
    ctx.robust_accumulate()
    for kw in (dict(gain=float("nan")), dict(gain=float("inf")), dict(gain=-1.0), dict(gain=1.0, dest=2), dict(gain=1.0, flags=1), dict(gain=1.0, reserved=(0, 0, 0, 0, 1))):
        assert lib.rtgl_robust_resolve(ctx.h, C.byref(H_.CRobustResolveParams(**kw))) == ERR_INVALID, kw
    assert lib.rtgl_read_robust_f32(ctx.h, out) == ERR_STATE                # none of them resolved
    assert lib.rtgl_robust_frames(ctx.h, None, None) == ERR_INVALID
    assert lib.rtgl_robust_frames(ctx.h, C.byref(n), None) == 0 and lib.rtgl_robust_frames(ctx.h, None, C.byref(k)) == 0 and (n.value, k.value) == (1, 8)
    assert lib.rtgl_read_robust_bucket_f32(ctx.h, 8, out) == ERR_INVALID and lib.rtgl_read_robust_bucket_f32(ctx.h, 0xFFFFFFFF, out) == ERR_INVALID
    assert lib.rtgl_read_robust_bucket_f32(ctx.h, 0, None) == ERR_INVALID and lib.rtgl_read_robust_f32(ctx.h, None) == ERR_INVALID
    ctx.robust_resolve()
    assert (ctx.read_robust() == np.array([0.5, 0.5, 0.5, 0.875], f32)).all()      # (G is of all 8 keys, seven of them 0: 3.5 / (8 x 0.5))
    # a second begin restarts: N = 0 and zeroed planes, with the same K and with another
    for K in (8, 16, 4):
        ctx.robust_begin(buckets=K)
        assert ctx.robust_frames() == (0, K) and not any(ctx.read_robust_bucket(j).any() for j in range(K))
        assert lib.rtgl_read_robust_f32(ctx.h, out) == ERR_STATE and lib.rtgl_read_robust_bucket_f32(ctx.h, K, out) == ERR_INVALID
        ctx.robust_accumulate()
    ctx.robust_end()
    no_session("after end")
    ctx.robust_begin()
    ctx.robust_end()
    ctx.close()


# ---------------------------------------------------------------------------------------------- 5. other buffers and memory

def test_a_session_leaves_every_other_buffer_alone(rt, randoms):
    H_ = rt.host
    base = rt.scenes.params_c1()
    ctx = rendering_context(rt, 32, 32, [("aov", H_.AOV_ALL), ("rng_state", 1)])
    for k in range(3):
        ctx.render(base.replace(frames=k + 1, random=randoms[k]))
        if k:
            ctx.error_estimate()
    ctx.denoise()
    ctx.temporal_accumulate()
    ctx.tonemap()

    def others():
        return dict(image=ctx.read_image(), denoised=ctx.read_denoised(), temporal=ctx.read_temporal(), display=ctx.read_display(), rng=ctx.read_rng_state(),
                    error_tiles=ctx.read_error_tiles(), error_summary=repr(ctx.read_error_summary()),
                    planes=b"".join(ctx.read_aov(p).tobytes() for p in (H_.AOV_ALBEDO, H_.AOV_NORMAL, H_.AOV_POSITION, H_.AOV_IDS)))
    before = others()
    ctx.robust_begin(buckets=4)
    for _ in range(6):
        ctx.robust_accumulate()
    ctx.robust_resolve()
    sess = rm.Session(32, 32, 4)
    for _ in range(6):
        sess.accumulate(before["image"])
    assert same(ctx.read_robust(), sess.resolve())
    ctx.robust_end()
    after = others()
    for key in before:
        a, b = before[key], after[key]
        assert (a == b) if isinstance(a, (str, bytes)) else (a.tobytes() == b.tobytes()), key
    ctx.render(base.replace(frames=4, random=randoms[3]))          # and the accumulation and its estimate go on
    ctx.error_estimate()
    assert ctx.read_error_summary()["valid"] == 1
    ctx.close()


def test_device_memory_is_held_between_begin_and_end_only(rt, randoms):
    """256 x 256: a plane is 1 MiB, so a session of K buckets adds K + 1 MiB exactly"""
    base = rt.scenes.params_c1()
    a, b = rendering_context(rt, 256, 256), rendering_context(rt, 256, 256)
    for ctx in (a, b):
        ctx.render(base.replace(frames=1, random=randoms[0]))
    m0 = b.get_option("device_mbytes")
    assert a.get_option("device_mbytes") == m0
    for K in (8, 8, 16, 4):                                  # (the second begin with the same K allocates nothing)
        b.robust_begin(buckets=K)
        assert b.get_option("device_mbytes") == m0 + K + 1, K
    b.robust_accumulate()
    b.robust_resolve()
    b.robust_resolve(dest=rm.DEST_IMAGE)
    assert b.get_option("device_mbytes") == m0 + 5
    b.robust_end()
    assert b.get_option("device_mbytes") == m0 == a.get_option("device_mbytes")
    for ctx in (a, b):
        ctx.render(base.replace(frames=2, random=randoms[1]))
    assert b.get_option("device_mbytes") == a.get_option("device_mbytes")
    a.close()
    b.close()
