"""A robust adaptive session on the device (include/rtgl_amd.h, "robust adaptive sampling").

The references are the numpy restatement, tests/robust_adaptive_mirror.py, pinned by tests/test_robust_adaptive_mirror.py, a plain robust
session on the same context, and adaptive sampling's own mirror.  Every comparison is exact: a NaN where the mirror has one, nothing else
may differ.  The named cases are those of tests/robust_adaptive_inputs.py: the ones the seeded defects of the CPU module are caught by."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_mirror as am
import robust_adaptive_inputs as rai
import robust_adaptive_mirror as ram
from test_facade_post import build_program

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


class _DeviceArray:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def same_records(got, want):
    return all(same(got[k], want[k]) for k in ("sum", "mse")) and all((got[k] == want[k]).all() for k in ("count", "converged", "samples", "samples_snapshot", "reserved"))


@pytest.fixture(scope="module")
def randoms(rt):
    g = rt.scenes.GlibcRand(0)
    return [g.rand() for _ in range(48)]


def scenes(rt):
    sc = rt.scenes
    return {"c1": (sc.scene_c1(False), sc.params_c1()), "lit": (sc.scene_c1(True), sc.params_c1()), "mesh": (sc.scene_mesh(10, 5, env_size=16), sc.params_c2())}


def context(rt, name, w, h, options=(), **kw):
    ctx = rt.host.Context(w, h, **kw)
    if name:
        ctx.upload_scene(scenes(rt)[name][0])
    for key, value in options:
        ctx.set_option(key, value)
    return ctx


def last_error(ctx):
    return ctx.lib.rtgl_last_error(ctx.h).decode()


class DeviceSession:
    """the context behind the interface of robust_adaptive_mirror.Session, for robust_adaptive_inputs.run"""

    def __init__(self, ctx, K):
        self.ctx, self.K = ctx, K

    def set_mask(self, tiles):
        self.ctx.robust_adaptive_set_mask(tiles)

    def fold(self, image):
        self.ctx.write_image(image)
        self.ctx.robust_adaptive_accumulate()

    def update(self):
        return self.ctx.robust_adaptive_update()

    def resolve(self, gain, dest):
        self.ctx.robust_adaptive_resolve(gain=gain, dest=dest)
        return self.ctx.read_image() if dest == ram.DEST_IMAGE else self.ctx.read_robust_adaptive()

    def tamper(self):
        import torch
        ptr = self.ctx.device_robust_adaptive_tiles_ptr()
        assert ptr
        rec = np.zeros(self.ctx._tiles_shape(), ram.TILE_DTYPE)
        for key, value in zip(("sum", "mse", "count", "converged", "samples", "samples_snapshot"), rai.SENTINEL):
            rec[key] = value
        words = np.frombuffer(np.ascontiguousarray(rec).tobytes(), np.int32).copy()
        torch.cuda.synchronize()
        torch.as_tensor(_DeviceArray(ptr, words.shape, "<i4"), device="cuda:0").copy_(torch.from_numpy(words))
        torch.cuda.synchronize()

    def buckets(self, which=None):
        return {j: self.ctx.read_robust_adaptive_bucket(j) for j in (range(self.K) if which is None else which)}


def run_case(rt, name, w, h, K):
    """the device and the mirror through one case in lockstep, everything observable compared after every step"""
    case = rai.make(name, h, w, K)
    ctx = context(rt, None, w, h)
    ctx.robust_adaptive_begin(**case["params"])
    dev, sess = DeviceSession(ctx, K), ram.Session(h, w, **case["params"])
    assert (ctx.robust_adaptive_get_mask() == sess.mask).all()
    for index, step in enumerate(case["steps"]):
        label = f"{name} {w}x{h} K={K} step {index} {step[0]}"
        if step[0] == "mask":
            dev.set_mask(step[1])
            sess.set_mask(step[1])
            assert (ctx.robust_adaptive_get_mask() == sess.mask).all(), label
        elif step[0] == "fold":
            written = sorted({int(n) % K for n in sess.n[sess.mask != 0]})
            dev.fold(step[1])
            sess.fold(step[1])
            for j, plane in dev.buckets(written).items():
                assert same(plane, sess.planes[j]), f"{label}: bucket {j}"
            assert same(ctx.read_image(), step[1]), f"{label}: the fold changed the image"
        elif step[0] == "update":
            got, want = dev.update(), sess.update()
            rec = ctx.read_robust_adaptive_tiles()
            assert same_records(rec, sess.records), f"{label}: device {rec.ravel()}, mirror {sess.records.ravel()}"
            assert am.same_summary(got, want) == [], f"{label}: device {got}, mirror {want}"
            assert (ctx.robust_adaptive_get_mask() == sess.mask).all(), label
            assert np.isfinite(rec["sum"]).all() and np.isfinite(rec["mse"]).all(), label
        elif step[0] == "tamper":
            dev.tamper()
            rai.tamper(sess)
            assert same_records(ctx.read_robust_adaptive_tiles(), sess.records), label
        else:
            for gain in case["gains"]:
                for dest in (ram.DEST_BUFFER, ram.DEST_IMAGE):
                    got, want = dev.resolve(gain, dest), sess.resolve(gain, dest)
                    assert same(got, want), f"{label}: gain {gain} dest {dest}"
                    assert np.isfinite(got[~case["injected"]]).all(), f"{label}: a non-finite output outside the injected pixels"
    for j, plane in dev.buckets().items():
        assert same(plane, sess.planes[j]), f"{name} {w}x{h} K={K}: bucket {j} at the end"
    ctx.robust_adaptive_end()
    ctx.close()


# ---------------------------------------------------------------------------------------------- 1. injected folds under masks, every size

@pytest.mark.parametrize("K", rai.BUCKETS)
@pytest.mark.parametrize("name", rai.NAMES)
def test_named_cases_equal_the_mirror(rt, name, K):
    for w, h in rai.SIZES:
        run_case(rt, name, w, h, K)


def test_pictures_without_a_footprint_are_zeros_and_no_ops(rt):
    for w, h in ((1, 1), (7, 7)):
        ctx = context(rt, "c1", w, h)
        ctx.robust_adaptive_begin(buckets=4, min_samples=4, max_samples=8)
        assert not ctx.robust_adaptive_get_mask().any()
        image = np.full((h, w, 4), 0.5, f32)
        ctx.write_image(image)
        ctx.robust_adaptive_accumulate()
        ctx.robust_adaptive_frame(scenes(rt)["c1"][1])
        s = ctx.robust_adaptive_update()
        assert s["converged"] == 1 and s["tiles_total"] == 0 and s["samples_total"] == 0 and s["blocks_active"] == 0
        assert ctx.read_robust_adaptive_tiles().tobytes() == bytes(32)
        for j in range(4):
            assert (bits(ctx.read_robust_adaptive_bucket(j)) == 0).all()
        ctx.robust_adaptive_resolve()
        assert (bits(ctx.read_robust_adaptive()) == 0).all() and same(ctx.read_image(), image)
        ctx.robust_adaptive_resolve(dest=ram.DEST_IMAGE)
        assert (bits(ctx.read_image()) == 0).all()
        ctx.close()


# ---------------------------------------------------------------------------------------------- 2. rendered frames

@pytest.mark.parametrize("K", rai.BUCKETS)
@pytest.mark.parametrize("case", [("mesh", 24, 40), ("lit", 70, 53)], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_a_rendered_session_equals_a_plain_robust_session_on_the_same_context(rt, randoms, case, K):
    name, w, h = case
    base = scenes(rt)[name][1]
    s = am.shape(h, w)
    inside = np.zeros((h, w), bool)
    inside[:s["fh"], :s["fw"]] = True
    params = dict(buckets=K, threshold=0.2, floor=0.02, gain=2.0, min_samples=K, max_samples=4 * K)
    ctx = context(rt, name, w, h)
    ctx.robust_begin(buckets=K)
    ctx.robust_adaptive_begin(**params)
    N = 2 * K + 3
    for k in range(N):
        ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)
        ctx.robust_accumulate()
        ctx.robust_adaptive_frame(base.replace(frames=9, reset_flag=0, random=randoms[k]), sync=False)      # (frames and reset_flag are ignored)
    assert ctx.last_frame_ms() > 0
    for j in range(K):
        got, want = ctx.read_robust_adaptive_bucket(j), ctx.read_robust_bucket(j)
        assert same(got[inside], want[inside]) and (bits(got[~inside]) == 0).all(), f"bucket {j}"
    for gain in (0.0, 2.0):
        ctx.robust_resolve(gain=gain)
        ctx.robust_adaptive_resolve(gain=gain)
        got, want = ctx.read_robust_adaptive(), ctx.read_robust()
        assert same(got[inside], want[inside]) and (bits(got[~inside]) == 0).all(), f"gain {gain}"
    summary = ctx.robust_adaptive_update()
    ctx.robust_error_estimate(threshold=params["threshold"], floor=params["floor"], gain=params["gain"])
    got, want = ctx.read_robust_adaptive_tiles(), ctx.read_robust_error_tiles()
    for key in ("sum", "mse"):
        assert same(got[key], want[key]), key
    for key in ("count", "converged"):
        assert (got[key] == want[key]).all(), key
    has = am.tile_pixels(h, w) > 0
    assert (got["samples"][has] == N).all() and (got["samples_snapshot"][has] == N).all() and summary["samples_total"] == N * s["fh"] * s["fw"]
    assert got["count"].any()
    ctx.close()


def test_masked_frames_fold_the_samples_of_ordinary_frames(rt, randoms):
    """under a checkerboard and its inverse: the buckets are the mirror's fed with a second context's ordinary one-frame images"""
    w, h, K = 40, 56, 4
    base = scenes(rt)["mesh"][1]
    a, b = context(rt, "mesh", w, h), context(rt, "mesh", w, h)
    params = dict(buckets=K, min_samples=K, max_samples=64)
    a.robust_adaptive_begin(**params)
    sess = ram.Session(h, w, **params)
    masks = rai.named_masks(h, w)
    for k, which in enumerate(("checker", "inverse", "checker", "all", "one", "checker", "none", "all")):
        a.robust_adaptive_set_mask(masks[which])
        sess.set_mask(masks[which])
        a.robust_adaptive_frame(base.replace(random=randoms[k]))
        b.render(base.replace(frames=0, reset_flag=1, random=randoms[k]))
        sess.fold(b.read_image())
        for j in range(K):
            assert same(a.read_robust_adaptive_bucket(j), sess.planes[j]), f"frame {k} bucket {j}"
    got, want = a.robust_adaptive_update(), sess.update()
    assert am.same_summary(got, want) == [] and same_records(a.read_robust_adaptive_tiles(), sess.records)
    a.close()
    b.close()


def test_render_robust_adaptive_follows_the_mirror_driven_loop(rt):
    """scene_c1(True), 64 x 64: at every update the device's masks, counts and summary are those of the mirror's loop fed with the device's
    own buckets; the loop stops before max_samples; HeadlessRenderer.render_robust_adaptive is that loop and returns its resolve"""
    sc = rt.scenes
    w = h = 64
    K, check_every = 8, 8
    params = dict(buckets=K, threshold=0.12, floor=0.01, gain=1.0, min_samples=16, max_samples=512)
    r = rt.host.HeadlessRenderer(w, h)
    r.set_scene(sc.scene_c1(True))
    r.params = sc.params_c1()
    ctx = r.ctx
    ctx.robust_adaptive_begin(**params)
    sess = ram.Session(h, w, **params)
    done = 0
    got, want = ctx.robust_adaptive_update(), sess.update()
    history = []
    while True:
        assert am.same_summary(got, want) == [], f"after {done} frames: device {got}, mirror {want}"
        assert (ctx.robust_adaptive_get_mask() == sess.mask).all() and same_records(ctx.read_robust_adaptive_tiles(), sess.records)
        history.append((done, got["tiles_active"], got["samples_total"]))
        if got["converged"]:
            break
        for _ in range(check_every):
            ctx.robust_adaptive_frame(r.session_frame(), sync=False)
            done += 1
        sess.n = sess.n + np.uint32(check_every) * sess.mask.astype(np.uint32)
        sess.planes = np.stack([ctx.read_robust_adaptive_bucket(j) for j in range(K)])
        got, want = ctx.robust_adaptive_update(), sess.update()
    print(f"render_robust_adaptive: (frames, active tiles, samples) {history}")
    assert 0 < done and got["samples_max"] < params["max_samples"] and got["tiles_capped"] == 0 and got["tiles_converged"] == 16
    assert got["samples_min"] < got["samples_max"] == done       # the tiles stopped at different counts: the masks differed between rounds
    ctx.robust_adaptive_resolve(gain=1.0)
    picture = ctx.read_robust_adaptive()
    assert same(picture, sess.resolve(1.0, ram.DEST_BUFFER))
    ctx.close()
    r2 = rt.host.HeadlessRenderer(w, h)
    r2.set_scene(sc.scene_c1(True))
    r2.params = sc.params_c1()
    frames, summary, out = r2.render_robust_adaptive(params["threshold"], params["max_samples"], min_samples=16, check_every=check_every, buckets=K)
    assert frames == done and am.same_summary(summary, got) == [] and same(out, picture)
    frames, summary, out = r2.render_robust_adaptive(params["threshold"], params["max_samples"], min_samples=16, check_every=check_every, buckets=K, to_image=True)
    assert same(out, r2.ctx.read_image()) and summary["converged"] == 1 and (out[..., 3] == 1).all()
    r2.ctx.close()


# ---------------------------------------------------------------------------------------------- 3. the state around the session

def test_the_session_leaves_every_other_buffer_alone(rt, randoms):
    w, h, K = 32, 32, 4
    H_ = rt.host
    base = scenes(rt)["mesh"][1]
    ctx, ordinary = context(rt, "mesh", w, h, [("aov", H_.AOV_ALL)]), context(rt, "mesh", w, h)
    for k in range(3):
        ctx.render(base.replace(frames=k + 1, random=randoms[k]))
        if k:
            ctx.error_estimate()
    ctx.denoise_guided()
    ctx.set_option("aov", 0)
    # an adaptive session with one frame, and a plain robust session with its error records
    ctx.adaptive_begin(min_samples=1, max_samples=8)
    mirror = am.Session(h, w, min_samples=1, max_samples=8)
    ctx.adaptive_frame(base.replace(random=randoms[4]))
    ordinary.render(base.replace(frames=0, reset_flag=1, random=randoms[4]))
    mirror.frame(ordinary.read_image())
    ctx.adaptive_update()
    mirror.update()
    ctx.robust_begin(buckets=4)
    for _ in range(5):
        ctx.robust_accumulate()
    ctx.robust_error_estimate()
    ctx.robust_resolve()

    def others():
        return dict(image=ctx.read_image(), denoised=ctx.read_denoised(), variance=ctx.read_denoise_variance(), error_tiles=ctx.read_error_tiles(),
                    error_summary=repr(ctx.read_error_summary()), adaptive_tiles=ctx.read_adaptive_tiles(), adaptive_mask=ctx.adaptive_get_mask(),
                    robust=ctx.read_robust(), robust_error_tiles=ctx.read_robust_error_tiles(), robust_error_summary=repr(ctx.read_robust_error_summary()),
                    robust_frames=repr(ctx.robust_frames()), buckets=np.stack([ctx.read_robust_bucket(j) for j in range(4)]))

    def unchanged(label):
        after = others()
        for key in before:
            a, b = before[key], after[key]
            assert (a == b) if isinstance(a, str) else (a.tobytes() == b.tobytes()), f"{label}: {key}"
    before = others()
    ctx.robust_adaptive_begin(buckets=K, min_samples=K, max_samples=16)
    unchanged("begin")
    for k in range(K + 1):
        ctx.robust_adaptive_frame(base.replace(random=randoms[8 + k]))
    unchanged("frames")
    ctx.robust_adaptive_accumulate()
    ctx.robust_adaptive_update()
    ctx.robust_adaptive_set_mask(rai.named_masks(h, w)["checker"])
    ctx.robust_adaptive_frame(base.replace(random=randoms[20]))
    ctx.robust_adaptive_update()
    ctx.robust_adaptive_resolve()
    ctx.read_robust_adaptive()
    ctx.read_robust_adaptive_tiles()
    ctx.read_robust_adaptive_bucket(K - 1)
    unchanged("update, masks, resolve into the buffer, read-outs")
    # the adaptive session is still its mirror's under a mask of its own, and its mask, frame and update move nothing of the open robust
    # adaptive session: the two kinds share their host code, not their state
    def session():
        return dict(mask=ctx.robust_adaptive_get_mask(), tiles=ctx.read_robust_adaptive_tiles(),
                    buckets=np.stack([ctx.read_robust_adaptive_bucket(j) for j in range(K)]))
    held = session()
    masks = rai.named_masks(h, w)
    own = next(m for m in (masks["one"], masks["checker"]) if m.tobytes() != held["mask"].tobytes())
    ctx.adaptive_set_mask(own)
    mirror.set_mask(own)
    assert ctx.adaptive_get_mask().tobytes() == own.tobytes()
    ctx.adaptive_frame(base.replace(random=randoms[5]))
    ordinary.render(base.replace(frames=0, reset_flag=1, random=randoms[5]))
    mirror.frame(ordinary.read_image())
    assert same(ctx.read_image(), mirror.image)
    got, want = ctx.adaptive_update(), mirror.update()
    assert am.same_summary(got, want) == [] and ctx.read_adaptive_tiles().tobytes() == np.ascontiguousarray(mirror.records).tobytes()
    for key, value in session().items():
        assert value.tobytes() == held[key].tobytes(), f"adaptive set_mask, frame and update: {key}"
    # the resolve into the image: the picture is an image like any other, the adaptive session ends, the snapshot is dropped
    before = others()
    ctx.robust_adaptive_resolve(gain=1.0)
    want = ctx.read_robust_adaptive()
    ctx.robust_adaptive_resolve(gain=1.0, dest=ram.DEST_IMAGE)
    img = ctx.read_image()
    assert same(img[..., :3], want[..., :3]) and img[..., :3].any()
    assert ctx.lib.rtgl_adaptive_frame(ctx.h) == ERR_STATE
    for key in ("image", "adaptive_mask"):
        before.pop(key)
    after = dict(denoised=ctx.read_denoised(), variance=ctx.read_denoise_variance(), robust=ctx.read_robust(), robust_error_tiles=ctx.read_robust_error_tiles(),
                 buckets=np.stack([ctx.read_robust_bucket(j) for j in range(4)]), adaptive_tiles=ctx.read_adaptive_tiles())
    for key, value in after.items():
        assert value.tobytes() == before[key].tobytes(), f"resolve into the image: {key}"
    ordinary.write_image(img)
    for c in (ctx, ordinary):
        c.denoise_guided(sigma_normal=0.0, sigma_position=0.0, demodulate=False)
        c.tonemap()
    assert same(ctx.read_denoised(), ordinary.read_denoised()) and (ctx.read_display() == ordinary.read_display()).all()
    ctx.robust_adaptive_frame(base.replace(random=randoms[21]))  # the session goes on
    ctx.close()
    ordinary.close()


def test_the_error_snapshot_survives_the_session(rt, randoms):
    """frames, a snapshot, a whole robust adaptive session short of a resolve into the image, another frame: the estimate is the one of a
    context that ran no session -- no call of the session writes the image or drops the snapshot"""
    w, h, K = 40, 24, 4
    base = scenes(rt)["mesh"][1]
    a, b = context(rt, "mesh", w, h), context(rt, "mesh", w, h)
    for ctx in (a, b):
        for k in range(2):
            ctx.render(base.replace(frames=k + 1, random=randoms[k]))
        ctx.error_estimate()
    a.robust_adaptive_begin(buckets=K, min_samples=K, max_samples=16)
    for k in range(K + 1):
        a.robust_adaptive_frame(base.replace(random=randoms[8 + k]))
    a.robust_adaptive_accumulate()
    a.robust_adaptive_update()
    a.robust_adaptive_resolve()
    assert same(a.read_image(), b.read_image())
    for ctx in (a, b):
        ctx.render(base.replace(frames=3, random=randoms[2]))
        ctx.error_estimate()
    sa, sb = a.read_error_summary(), b.read_error_summary()
    assert repr(sa) == repr(sb) and sa["valid"] == 1 and (sa["frames_now"], sa["frames_snapshot"]) == (3, 2)
    assert a.read_error_tiles().tobytes() == b.read_error_tiles().tobytes() and same(a.read_image(), b.read_image())
    a.robust_adaptive_resolve(dest=ram.DEST_IMAGE)           # this one is a write of the image: the snapshot goes
    a.render(base.replace(frames=4, random=randoms[3]))
    a.error_estimate()
    assert a.read_error_summary()["valid"] == 0
    a.close()
    b.close()


def test_held_frames_are_submitted_first_and_a_torch_stream_carries_the_session(rt, randoms):
    import torch
    w, h, K = 24, 40, 4
    base = scenes(rt)["mesh"][1]
    params = dict(buckets=K, min_samples=K, max_samples=32)
    a, b = context(rt, "mesh", w, h, [("frame_batch", 3)]), context(rt, "mesh", w, h)
    for ctx in (a, b):
        ctx.robust_adaptive_begin(**params)
        for k in range(2):                                   # (held by `a`)
            ctx.render(base.replace(frames=k, reset_flag=int(k == 0), random=randoms[k]), sync=False)
        ctx.robust_adaptive_accumulate()                     # submits them, then folds the image of two frames
        ctx.robust_adaptive_frame(base.replace(random=randoms[2]), sync=False)
    for j in range(K):
        assert same(a.read_robust_adaptive_bucket(j), b.read_robust_adaptive_bucket(j))
    assert same(a.read_robust_adaptive_bucket(0), b.read_image()) and b.read_image()[..., :3].any()
    a.close()

    def finish(ctx):
        for k in range(3, 3 + K):
            ctx.robust_adaptive_frame(base.replace(random=randoms[k]), sync=False)
        summary = ctx.robust_adaptive_update()
        ctx.robust_adaptive_resolve()
        return summary, ctx.read_robust_adaptive_tiles(), ctx.read_robust_adaptive(), [ctx.read_robust_adaptive_bucket(j) for j in range(K)]
    want = finish(b)
    b.close()                                                # (one stream per device at a time: rtgl_set_stream)
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    c = rt.host.Context(w, h)
    with torch.cuda.stream(side):
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.upload_scene(scenes(rt)["mesh"][0])
        c.robust_adaptive_begin(**params)
        for k in range(2):
            c.render(base.replace(frames=k, reset_flag=int(k == 0), random=randoms[k]), sync=False)
        c.robust_adaptive_accumulate()
        c.robust_adaptive_frame(base.replace(random=randoms[2]), sync=False)
        got = finish(c)
        side.synchronize()
    assert am.same_summary(got[0], want[0]) == [] and same_records(got[1], want[1]) and same(got[2], want[2]) and want[2][..., :3].any()
    for j in range(K):
        assert same(got[3][j], want[3][j])
    c.close()


def test_a_second_begin_restarts_and_end_frees(rt, randoms):
    w, h = 70, 53
    ctx = context(rt, "c1", w, h)
    base = scenes(rt)["c1"][1]
    ctx.robust_adaptive_begin(buckets=16, min_samples=16, max_samples=64)
    ctx.robust_adaptive_frame(base.replace(random=randoms[1]))   # (the frame's own queues stay with the context)
    ctx.robust_adaptive_end()
    start = ctx.get_option("device_mbytes")
    image = np.random.default_rng(3).random((h, w, 4), f32)
    for K in (4, 4, 16, 8):
        ctx.robust_adaptive_begin(buckets=K, min_samples=K, max_samples=64)
        assert ctx.read_robust_adaptive_tiles().tobytes() == bytes(32 * 20)
        for j in range(K):
            assert (bits(ctx.read_robust_adaptive_bucket(j)) == 0).all()
        ctx.write_image(image)
        for _ in range(K):
            ctx.robust_adaptive_accumulate()
        ctx.robust_adaptive_frame(base.replace(random=randoms[0]))
        ctx.robust_adaptive_update()
        assert ctx.read_robust_adaptive_tiles()["samples"][0, 0] == K + 1
        assert same(ctx.read_image(), image)                 # begin and the frame leave the image alone
    ctx.robust_adaptive_end()
    assert ctx.get_option("device_mbytes") <= start and not ctx.device_robust_adaptive_tiles_ptr()
    assert ctx.lib.rtgl_robust_adaptive_end(ctx.h) == ERR_STATE
    ctx.close()


# ---------------------------------------------------------------------------------------------- 4. refusals

def test_every_refusal_names_its_call(rt, randoms):
    w, h = 24, 40
    H_ = rt.host
    ctx = context(rt, "mesh", w, h)
    lib, base = ctx.lib, scenes(rt)["mesh"][1]
    s, mask, px = H_.CAdaptiveSummary(), np.ones((3, 2), np.uint8), np.zeros((h, w, 4), f32)
    tiles, r = np.zeros((3, 2), ram.TILE_DTYPE), H_.CRobustResolveParams()
    lib.rtgl_robust_defaults(None, C.byref(r))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    calls = {"rtgl_robust_adaptive_frame": lambda: lib.rtgl_robust_adaptive_frame(ctx.h),
             "rtgl_robust_adaptive_accumulate": lambda: lib.rtgl_robust_adaptive_accumulate(ctx.h),
             "rtgl_robust_adaptive_update": lambda: lib.rtgl_robust_adaptive_update(ctx.h, C.byref(s)),
             "rtgl_robust_adaptive_set_mask": lambda: lib.rtgl_robust_adaptive_set_mask(ctx.h, vp(mask)),
             "rtgl_robust_adaptive_get_mask": lambda: lib.rtgl_robust_adaptive_get_mask(ctx.h, vp(mask)),
             "rtgl_robust_adaptive_resolve": lambda: lib.rtgl_robust_adaptive_resolve(ctx.h, C.byref(r)),
             "rtgl_robust_adaptive_end": lambda: lib.rtgl_robust_adaptive_end(ctx.h),
             "rtgl_read_robust_adaptive_f32": lambda: lib.rtgl_read_robust_adaptive_f32(ctx.h, vp(px)),
             "rtgl_read_robust_adaptive_bucket_f32": lambda: lib.rtgl_read_robust_adaptive_bucket_f32(ctx.h, 0, vp(px)),
             "rtgl_read_robust_adaptive_tiles": lambda: lib.rtgl_read_robust_adaptive_tiles(ctx.h, vp(tiles), None, None)}

    def refused(name, call, code):
        assert call() == code, name
        assert last_error(ctx).startswith(name + ":"), (name, last_error(ctx))

    def no_session(label):
        for name, call in calls.items():
            refused(name, call, ERR_STATE)
            assert "no session" in last_error(ctx), (label, name)
        assert not ctx.device_robust_adaptive_tiles_ptr() and last_error(ctx).startswith("rtgl_device_robust_adaptive_tiles:")
    no_session("before the first begin")
    # the events that end an adaptive session do not end this one
    ctx.robust_adaptive_begin()
    refused("rtgl_robust_adaptive_frame", calls["rtgl_robust_adaptive_frame"], ERR_STATE)      # no frame parameters yet
    ctx.render(base.replace(frames=1, random=randoms[1]))
    ctx.clear_image()
    ctx.write_image(px)
    ctx.robust_adaptive_frame(base.replace(random=randoms[0]))
    refused("rtgl_read_robust_adaptive_f32", calls["rtgl_read_robust_adaptive_f32"], ERR_STATE)      # no resolve into the buffer yet
    ctx.robust_adaptive_resolve(dest=ram.DEST_IMAGE)
    refused("rtgl_read_robust_adaptive_f32", calls["rtgl_read_robust_adaptive_f32"], ERR_STATE)
    ctx.robust_adaptive_resolve()
    assert calls["rtgl_read_robust_adaptive_f32"]() == 0
    # refusals inside a session
    for key in ("aov", "rng_state"):
        ctx.set_option(key, 1)
        refused("rtgl_robust_adaptive_frame", calls["rtgl_robust_adaptive_frame"], ERR_STATE)
        ctx.set_option(key, 0)
    ctx.set_params(base.replace(samples=2))
    refused("rtgl_robust_adaptive_frame", calls["rtgl_robust_adaptive_frame"], ERR_INVALID)
    ctx.set_params(base.replace(max_bounce=0))
    refused("rtgl_robust_adaptive_frame", calls["rtgl_robust_adaptive_frame"], ERR_INVALID)
    ctx.set_params(base)
    refused("rtgl_robust_adaptive_update", lambda: lib.rtgl_robust_adaptive_update(ctx.h, None), ERR_INVALID)
    refused("rtgl_robust_adaptive_set_mask", lambda: lib.rtgl_robust_adaptive_set_mask(ctx.h, None), ERR_INVALID)
    refused("rtgl_robust_adaptive_get_mask", lambda: lib.rtgl_robust_adaptive_get_mask(ctx.h, None), ERR_INVALID)
    refused("rtgl_robust_adaptive_resolve", lambda: lib.rtgl_robust_adaptive_resolve(ctx.h, None), ERR_INVALID)
    refused("rtgl_read_robust_adaptive_f32", lambda: lib.rtgl_read_robust_adaptive_f32(ctx.h, None), ERR_INVALID)
    refused("rtgl_read_robust_adaptive_bucket_f32", lambda: lib.rtgl_read_robust_adaptive_bucket_f32(ctx.h, 0, None), ERR_INVALID)
    refused("rtgl_read_robust_adaptive_bucket_f32", lambda: lib.rtgl_read_robust_adaptive_bucket_f32(ctx.h, 8, vp(px)), ERR_INVALID)
    refused("rtgl_read_robust_adaptive_tiles", lambda: lib.rtgl_read_robust_adaptive_tiles(ctx.h, None, None, None), ERR_INVALID)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(gain=nan), dict(gain=inf), dict(gain=-1.0), dict(dest=2), dict(flags=1), dict(reserved=(0, 0, 0, 0, 1))):
        q = H_.CRobustResolveParams()
        lib.rtgl_robust_defaults(None, C.byref(q))
        for k, v in bad.items():
            setattr(q, k, v)
        refused("rtgl_robust_adaptive_resolve", lambda: lib.rtgl_robust_adaptive_resolve(ctx.h, C.byref(q)), ERR_INVALID)
    refused("rtgl_robust_adaptive_begin", lambda: lib.rtgl_robust_adaptive_begin(ctx.h, None), ERR_INVALID)
    for bad in rai.invalid_params():
        p = H_.CRobustAdaptiveParams()
        lib.rtgl_robust_adaptive_defaults(C.byref(p))
        for k, v in bad.items():
            setattr(p, k, v)
        refused("rtgl_robust_adaptive_begin", lambda: lib.rtgl_robust_adaptive_begin(ctx.h, C.byref(p)), ERR_INVALID)
    ctx.robust_adaptive_frame(base.replace(random=randoms[0]))  # a refused begin leaves the session as it was
    ctx.robust_adaptive_end()
    no_session("after end")
    ctx.close()


def test_tiled_and_multi_device_contexts_are_refused(rt):
    for kw in (dict(rank=0, world=2, strip_rows=8), dict(devices=[0, 0], strip_rows=8)):
        ctx = rt.host.Context(32, 32, **kw)
        p = rt.host.CRobustAdaptiveParams()
        ctx.lib.rtgl_robust_adaptive_defaults(C.byref(p))
        assert ctx.lib.rtgl_robust_adaptive_begin(ctx.h, C.byref(p)) == ERR_STATE, kw
        assert last_error(ctx).startswith("rtgl_robust_adaptive_begin:"), kw
        assert ctx.lib.rtgl_robust_adaptive_frame(ctx.h) == ERR_STATE and ctx.lib.rtgl_robust_adaptive_accumulate(ctx.h) == ERR_STATE, kw
        ctx.close()


# ---------------------------------------------------------------------------------------------- 5. the C++ twin

class Logging:
    """mixed into host.HeadlessRenderer: the uniforms of every frame of any kind"""

    def next_frame(self):
        self.log.append(super().next_frame())
        return self.log[-1]

    def session_frame(self, reset_flag=0):
        self.log.append(super().session_frame(reset_flag))
        return self.log[-1]


def summary_of(raw64):
    s = C.cast(C.create_string_buffer(raw64, 64), C.POINTER(C.c_uint32))
    names = ("tiles_total", "tiles_active", "tiles_converged", "tiles_capped", "blocks_active", "samples_min", "samples_max", "converged")
    out = {k: int(s[i]) for i, k in enumerate(names)}
    out["samples_total"] = int(np.frombuffer(raw64, np.uint64)[4])
    out["max_tile_mse"] = np.frombuffer(raw64, f32)[10]
    return out


def test_the_facade_and_the_headless_renderer_are_twins(rt, tmp_path):
    """tests/cpp/facade_robust_adaptive.cpp in a child process: its log of uniforms, frame counts, summaries, records and pictures against
    host.HeadlessRenderer through the same calls, and its first picture and records against the mirror fed with its own buckets"""
    w, h = 70, 53
    exe = build_program(rt, tmp_path, "facade_robust_adaptive")
    d = str(tmp_path)
    try:
        run = subprocess.run([exe, d, str(w), str(h)], cwd=d, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("facade_robust_adaptive did not end within its time limit")
    assert run.returncode == 0, f"facade_robust_adaptive ended with {run.returncode}:\n{run.stderr[-2000:]}"
    H_, sc = rt.host, rt.scenes
    raw = lambda name, dtype: np.fromfile(os.path.join(d, name + ".raw"), dtype)
    blob = open(os.path.join(d, "params.raw"), "rb").read()
    n = C.sizeof(H_.CFrameParams)
    used = [H_.CFrameParams.from_buffer_copy(blob[i:i + n]) for i in range(0, len(blob), n)]
    a, b, logged = (int(v) for v in raw("returns", np.int64))
    assert logged == len(used) == 1 + a + 1 + b + 2
    summaries = [summary_of(raw("summaries", np.uint8)[i * 64:(i + 1) * 64].tobytes()) for i in range(3)]
    scene = sc.Scene(spheres=raw("spheres", f32).reshape(-1, 8), materials=raw("materials", f32).reshape(-1, 8), nodes=raw("nodes", f32).reshape(-1, 12))
    fields = {name: getattr(used[0], name) for name, _ in H_.CFrameParams._fields_}
    fields = {k: (tuple(v) if hasattr(v, "__len__") else v) for k, v in fields.items()}
    fields.update(frames=0, reset_flag=0, random=0)
    r = type("LoggingRenderer", (Logging, H_.HeadlessRenderer), {})(w, h)
    r.log = []
    r.set_scene(scene)
    r.params = sc.FrameParams(**fields)
    r.render_frame()
    r.reset_buffer()
    done, first, picture = r.render_robust_adaptive(0.35, 48, min_samples=8, check_every=6, buckets=4)
    assert done == a and 8 <= a and am.same_summary(first, summaries[0]) == [] and first["converged"] == 1, f"{done}, {first}; facade {a}, {summaries[0]}"
    assert same(picture, raw("picture_first", f32).reshape(h, w, 4))
    tiles = r.ctx.read_robust_adaptive_tiles()
    assert tiles.tobytes() == raw("tiles_first", np.uint8).tobytes()
    # the mirror over the program's own buckets and counts
    planes = np.stack([raw(f"bucket{j}", f32).reshape(h, w, 4) for j in range(4)])
    assert same(picture, ram.resolve(planes, tiles["samples"], 1.0, ram.DEST_BUFFER))
    m, records = ram.update(planes, tiles["samples"], np.zeros_like(tiles["samples"]), np.zeros(tiles.shape, ram.TILE_DTYPE), threshold=0.35, floor=0.01, gain=1.0)
    assert same_records(records, tiles)
    mask = np.zeros(tiles.shape, np.uint8)
    mask[0, 0] = 1
    r.ctx.robust_adaptive_set_mask(mask)
    r.ctx.robust_adaptive_frame(r.session_frame())
    hand = r.ctx.robust_adaptive_update()
    assert am.same_summary(hand, summaries[1]) == [] and r.ctx.read_robust_adaptive_tiles().tobytes() == raw("tiles_hand", np.uint8).tobytes()
    assert hand["samples_max"] == tiles["samples"][0, 0] + 1
    done, second, picture = r.render_robust_adaptive(1e-6, 11, min_samples=8, check_every=4, buckets=8, gain=0.5, to_image=True)
    assert done == b == 12 and am.same_summary(second, summaries[2]) == [] and 0 < second["tiles_capped"] and second["tiles_capped"] + second["tiles_converged"] == second["tiles_total"] == 12      # (a tile of plain background has no spread)
    assert same(picture, raw("picture_second", f32).reshape(h, w, 4))
    r.run(2)
    assert [(p.frames, p.reset_flag, p.random) for p in r.log] == [(p.frames, p.reset_flag, p.random) for p in used]
    assert same(r.ctx.read_image(), raw("final_image", f32).reshape(h, w, 4))
    r.ctx.close()
