"""rtgl_robust_error_estimate on the device (include/rtgl_amd.h, "robust error estimate").

The reference is the numpy restatement, tests/robust_error_mirror.py, pinned by tests/test_robust_error_mirror.py.  Every comparison is
exact: the estimate is defined operation by operation and the sums are taken in one order, so every word of the tile records and of the
summary equals the mirror's.  The bucket planes are injected through the path tests/test_gpu_robust.py uses (write_image, then
robust_accumulate, per sample), which that module holds to tests/robust_mirror.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import error_mirror as em
import robust_error_inputs as rei
import robust_error_mirror as rem
import robust_inputs as ri
import robust_mirror as rm
from test_facade_post import build_program

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


def device_result(ctx):
    out = ctx.read_robust_error_summary()
    out["tiles"] = ctx.read_robust_error_tiles()
    return out


def inject(ctx, samples, K):
    """a session of the device and the mirror's, fed with the same samples"""
    h, w = samples[0].shape[:2]
    sess = rm.Session(h, w, K)
    ctx.robust_begin(buckets=K)
    for s in samples:
        ctx.write_image(s)
        ctx.robust_accumulate()
        sess.accumulate(s)
    return sess


def check_estimates(ctx, sess, params_list, label):
    for params in params_list:
        ctx.robust_error_estimate(**params)
        want = rem.estimate(sess.planes, sess.N, **params)
        assert em.same_result(device_result(ctx), want) == [], f"{label} {params}"


# ---------------------------------------------------------------------------------------------- 1. injected buckets

@pytest.mark.parametrize("K", rei.BUCKETS)
@pytest.mark.parametrize("size", rei.GPU_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_injected_families_equal_the_mirror(rt, size, K):
    """every family of tests/robust_error_inputs.py; one context, a session per family"""
    w, h = size
    ctx = rt.host.Context(w, h)
    for family in rei.FAMILIES:
        case = rei.make(family, h, w, K)
        sess = inject(ctx, case["samples"], K)
        check_estimates(ctx, sess, case["params"], f"{family} {w} x {h} K = {K}")
        for j in range(K):                                         # the estimate only read the buckets
            assert same(ctx.read_robust_bucket(j), sess.planes[j]), f"{family}: bucket {j}"
    ctx.robust_end()
    ctx.close()


def test_a_full_hd_session(rt):
    """1920 x 1080, K = 8, N = 9: 120 x 68 tiles, the last tile row half outside the picture, the solve's lanes over 32 rounds of records"""
    w, h, K = 1920, 1080, 8
    samples = ri.noisy(np.random.default_rng(1080), h, w, 9)
    ctx = rt.host.Context(w, h)
    sess = inject(ctx, samples, K)
    check_estimates(ctx, sess, [dict(), dict(gain=0.0, threshold=0.5)], "1920 x 1080")
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. rendered frames

@pytest.fixture(scope="module")
def randoms(rt):
    g = rt.scenes.GlibcRand(0)
    return [g.rand() for _ in range(64)]


def rendering_context(rt, w, h, options=(), **kw):
    ctx = rt.host.Context(w, h, **kw)
    ctx.upload_scene(rt.scenes.scene_c1(True))
    for key, value in options:
        ctx.set_option(key, value)
    return ctx


def test_a_rendered_session_equals_the_mirror_fed_with_its_buckets(rt, randoms):
    base, K, N = rt.scenes.params_c1(), 8, 20
    ctx = rendering_context(rt, 64, 64)
    ctx.robust_begin(buckets=K)
    for k in range(N):
        ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)
        ctx.robust_accumulate()
    planes = np.stack([ctx.read_robust_bucket(j) for j in range(K)])
    for params in (dict(), dict(gain=0.0), dict(gain=2.5, threshold=0.2, quantile_permille=600)):
        ctx.robust_error_estimate(**params)
        got = device_result(ctx)
        assert em.same_result(got, rem.estimate(planes, N, **params)) == [], params
        assert got["frames_now"] == N and got["tiles_valid"] == 16 and 0 < float(got["mse"]) < np.inf
    assert int(ctx.device_robust_error_tiles_ptr()) != 0
    ctx.close()


# ---------------------------------------------------------------------------------------------- 3. other buffers, memory

def test_an_estimate_leaves_every_other_buffer_alone(rt, randoms):
    """two contexts through the same calls, one with robust error estimates in between: every buffer, the records and the summary of
    rtgl_error_estimate, and what rtgl_error_estimate says next (so: its snapshot) are the same bits"""
    H_ = rt.host
    base = rt.scenes.params_c1()
    a, b = (rendering_context(rt, 32, 32, [("aov", H_.AOV_ALL), ("rng_state", 1)]) for _ in range(2))

    def others(ctx):
        return dict(image=ctx.read_image(), denoised=ctx.read_denoised(), temporal=ctx.read_temporal(), display=ctx.read_display(), rng=ctx.read_rng_state(),
                    error_tiles=ctx.read_error_tiles(), error_summary=repr(ctx.read_error_summary()), robust=ctx.read_robust(),
                    buckets=b"".join(ctx.read_robust_bucket(j).tobytes() for j in range(4)),
                    planes=b"".join(ctx.read_aov(p).tobytes() for p in (H_.AOV_ALBEDO, H_.AOV_NORMAL, H_.AOV_POSITION, H_.AOV_IDS)))

    for ctx in (a, b):
        for k in range(3):
            ctx.render(base.replace(frames=k + 1, reset_flag=int(k == 0), random=randoms[k]))
            if k:
                ctx.error_estimate()
        ctx.denoise()
        ctx.temporal_accumulate()
        ctx.tonemap()
        ctx.robust_begin(buckets=4)
        for _ in range(6):
            ctx.robust_accumulate()
        ctx.robust_resolve()
    before = others(a)
    for params in (dict(), dict(gain=0.0, threshold=0.3)):
        a.robust_error_estimate(**params)
        a.read_robust_error_summary()
    after, twin = others(a), others(b)
    for key in before:
        for x, y in ((before[key], after[key]), (before[key], twin[key])):
            assert (x == y) if isinstance(x, (str, bytes)) else (x.tobytes() == y.tobytes()), key
    for ctx in (a, b):                                             # the accumulation and its estimate go on, alike
        ctx.render(base.replace(frames=4, random=randoms[3]))
        ctx.error_estimate()
    sa, sb = a.read_error_summary(), b.read_error_summary()
    assert sa["valid"] == 1 and repr(sa) == repr(sb) and a.read_error_tiles().tobytes() == b.read_error_tiles().tobytes()
    assert a.read_image().tobytes() == b.read_image().tobytes()
    a.close()
    b.close()
    a, b = (rendering_context(rt, 32, 32) for _ in range(2))       # an open adaptive session stays open and as it was
    for ctx in (a, b):
        ctx.adaptive_begin(min_samples=1, max_samples=4)
        ctx.adaptive_frame(base.replace(random=randoms[10]))
        ctx.adaptive_update()
        ctx.robust_begin(buckets=4)
        for _ in range(4):
            ctx.robust_accumulate()
    a.robust_error_estimate()
    assert a.read_robust_error_summary()["valid"] == 1
    for ctx in (a, b):
        ctx.adaptive_frame(base.replace(random=randoms[11]))
    assert repr(a.adaptive_update()) == repr(b.adaptive_update()) and a.read_image().tobytes() == b.read_image().tobytes()
    assert (a.adaptive_get_mask() == b.adaptive_get_mask()).all() and a.read_adaptive_tiles().tobytes() == b.read_adaptive_tiles().tobytes()
    a.close()
    b.close()


def test_device_memory_is_back_to_its_start_after_end(rt, randoms):
    """256 x 256: a session of K buckets is K + 1 MiB, the records of the estimate 4 KiB + 64 bytes; all of it goes with rtgl_robust_end"""
    base = rt.scenes.params_c1()
    a, b = rendering_context(rt, 256, 256), rendering_context(rt, 256, 256)
    for ctx in (a, b):
        ctx.render(base.replace(frames=1, random=randoms[0]))
    m0 = a.get_option("device_mbytes")
    assert b.get_option("device_mbytes") == m0
    b.robust_begin(buckets=4)
    assert b.get_option("device_mbytes") == m0 + 5                 # (begin's own memory is what it was)
    for _ in range(4):
        b.robust_accumulate()
    b.robust_error_estimate()
    assert b.read_robust_error_summary()["valid"] == 1
    assert m0 + 5 <= b.get_option("device_mbytes") <= m0 + 6
    b.robust_begin(buckets=8)                                      # a second begin keeps the records' memory; the read-outs wait for an estimate
    assert b.lib.rtgl_read_robust_error_summary(b.h, C.byref(rt.host.CErrorSummary())) == ERR_STATE
    assert m0 + 9 <= b.get_option("device_mbytes") <= m0 + 10
    b.robust_end()
    assert b.get_option("device_mbytes") == m0 == a.get_option("device_mbytes")
    for ctx in (a, b):
        ctx.render(base.replace(frames=2, random=randoms[1]))
    assert b.get_option("device_mbytes") == a.get_option("device_mbytes")
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 4. states and refusals

def test_states_and_refusals_on_a_live_context(rt):
    H_ = rt.host
    w, h = 17, 17
    ctx = H_.Context(w, h)
    lib = ctx.lib
    p, s = H_.CRobustErrorParams(), H_.CErrorSummary()
    assert lib.rtgl_robust_error_defaults(C.byref(p)) == 0
    tiles = np.zeros((2, 2), H_.ERROR_TILE_DTYPE)
    tp = tiles.ctypes.data_as(C.c_void_p)

    def unreadable(label):
        assert lib.rtgl_read_robust_error_summary(ctx.h, C.byref(s)) == ERR_STATE, label
        assert lib.rtgl_read_robust_error_tiles(ctx.h, tp, None, None) == ERR_STATE, label
        assert not lib.rtgl_device_robust_error_tiles(ctx.h), label
        assert b"rtgl_robust_error_estimate" in lib.rtgl_last_error(ctx.h), label

    assert lib.rtgl_robust_error_estimate(ctx.h, C.byref(p)) == ERR_STATE and b"no session" in lib.rtgl_last_error(ctx.h)
    unreadable("before the first begin")
    image = np.full((h, w, 4), 0.5, f32)
    ctx.write_image(image)
    for K in (8, 4, 16):                                           # N < K: refused; N = K: taken; a second begin, with another K, starts over
        ctx.robust_begin(buckets=K)
        unreadable(f"after begin, K = {K}")
        for n in range(K):
            assert lib.rtgl_robust_error_estimate(ctx.h, None) == ERR_STATE and b"fewer frames than buckets" in lib.rtgl_last_error(ctx.h), (K, n)
            ctx.robust_accumulate()
        unreadable(f"before the first estimate, K = {K}")
        assert lib.rtgl_robust_error_estimate(ctx.h, None) == 0    # NULL: the defaults
        got = device_result(ctx)
        want = rem.estimate(np.broadcast_to(image, (K, h, w, 4)), K)
        assert em.same_result(got, want) == [] and got["converged"] == 1 and got["frames_now"] == K
        # invalid arguments: refused, and the results of the last estimate stay as they are
        nan, inf = float("nan"), float("inf")
        for kw in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=nan), dict(threshold=inf), dict(floor=0.0), dict(floor=nan), dict(floor=-inf),
                   dict(gain=nan), dict(gain=inf), dict(gain=-1.0), dict(gain=-1e-30), dict(quantile_permille=0), dict(quantile_permille=1001),
                   dict(flags=1), dict(reserved=(0, 0, 1)), dict(reserved=(1, 0, 0))):
            bad = H_.CRobustErrorParams()
            lib.rtgl_robust_error_defaults(C.byref(bad))
            for k, v in kw.items():
                setattr(bad, k, v)
            assert lib.rtgl_robust_error_estimate(ctx.h, C.byref(bad)) == ERR_INVALID, kw
            assert not rem.valid_params(bad.threshold, bad.floor, bad.gain, bad.quantile_permille, bad.flags, tuple(bad.reserved)), kw
        assert lib.rtgl_read_robust_error_summary(ctx.h, None) == ERR_INVALID and lib.rtgl_read_robust_error_tiles(ctx.h, None, None, None) == ERR_INVALID
        assert em.same_result(device_result(ctx), want) == []
        nx, ny = C.c_uint32(), C.c_uint32()
        assert lib.rtgl_read_robust_error_tiles(ctx.h, tp, C.byref(nx), None) == 0 and lib.rtgl_read_robust_error_tiles(ctx.h, tp, None, C.byref(ny)) == 0
        assert (nx.value, ny.value) == (2, 2) and tiles.tobytes() == want["tiles"].tobytes()
    ctx.robust_end()
    assert lib.rtgl_robust_error_estimate(ctx.h, None) == ERR_STATE and b"no session" in lib.rtgl_last_error(ctx.h)
    unreadable("after end")
    ctx.close()
    assert lib.rtgl_robust_error_estimate(None, None) == ERR_INVALID and lib.rtgl_read_robust_error_summary(None, C.byref(s)) == ERR_INVALID
    assert lib.rtgl_read_robust_error_tiles(None, tp, None, None) == ERR_INVALID and not lib.rtgl_device_robust_error_tiles(None)


def test_tiled_and_multi_device_contexts_are_refused(rt):
    """a strip is not the picture: rank 1 of world 2 may hold a session, but not estimate it; a multi-device context holds no session"""
    tiled = rt.host.Context(64, 64, rank=1, world=2, strip_rows=8)
    tiled.robust_begin(buckets=4)
    for _ in range(4):
        tiled.robust_accumulate()
    assert tiled.lib.rtgl_robust_error_estimate(tiled.h, None) == ERR_STATE and b"strips" in tiled.lib.rtgl_last_error(tiled.h)
    assert tiled.lib.rtgl_read_robust_error_summary(tiled.h, C.byref(rt.host.CErrorSummary())) == ERR_STATE
    tiled.robust_resolve()                                         # the session is as it was
    tiled.close()
    multi = rt.host.Context(32, 32, devices=[0, 0], strip_rows=8)
    assert multi.lib.rtgl_robust_error_estimate(multi.h, None) == ERR_STATE and b"multi-device" in multi.lib.rtgl_last_error(multi.h)
    assert not multi.lib.rtgl_device_robust_error_tiles(multi.h)
    multi.close()


# ---------------------------------------------------------------------------------------------- 5. several contexts, held frames

def test_two_contexts_take_turns(rt):
    sizes, Ks = [(17, 17), (70, 53)], [16, 4]
    ctxs = [rt.host.Context(w, h) for w, h in sizes]
    cases = [rei.make("ragged", h, w, K) for (w, h), K in zip(sizes, Ks)]
    sessions = [rm.Session(h, w, K) for (w, h), K in zip(sizes, Ks)]
    for ctx, K in zip(ctxs, Ks):
        ctx.robust_begin(buckets=K)
    checked = 0
    for k in range(max(len(c["samples"]) for c in cases)):
        for ctx, case, sess in zip(ctxs, cases, sessions):
            if k < len(case["samples"]):
                ctx.write_image(case["samples"][k])
                ctx.robust_accumulate()
                sess.accumulate(case["samples"][k])
                if sess.N >= sess.K:
                    ctx.robust_error_estimate(gain=0.25)           # (enqueued; read after the other context's turn)
        for ctx, sess in zip(ctxs, sessions):
            if sess.N >= sess.K and k < 2 * sess.K + 3:
                assert em.same_result(device_result(ctx), rem.estimate(sess.planes, sess.N, gain=0.25)) == [], (k, sess.K)
                checked += 1
    assert checked > 20
    for ctx in ctxs:
        ctx.close()


def test_frames_held_by_a_batching_context_are_submitted_first(rt, randoms):
    base = rt.scenes.params_c1()
    a, b = rendering_context(rt, 24, 40, [("frame_batch", 8)]), rendering_context(rt, 24, 40)
    for ctx in (a, b):
        ctx.robust_begin(buckets=4)
        for k in range(4):
            ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)
            ctx.robust_accumulate()
        for k in range(3):                                         # (held by `a`: the estimate submits them, and reads the buckets, not the image)
            ctx.render(base.replace(frames=k, reset_flag=int(k == 0), random=randoms[4 + k]), sync=False)
        ctx.robust_error_estimate()
    planes = np.stack([b.read_robust_bucket(j) for j in range(4)])
    want = rem.estimate(planes, 4)
    assert em.same_result(device_result(a), want) == [] and em.same_result(device_result(b), want) == []
    assert same(a.read_image(), b.read_image()) and a.read_image()[..., :3].any()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 6. render_robust_until and the C++ twin

class Logging:
    """mixed into host.HeadlessRenderer: the uniforms of every frame of any kind"""

    def next_frame(self):
        self.log.append(super().next_frame())
        return self.log[-1]

    def session_frame(self, reset_flag=0):
        self.log.append(super().session_frame(reset_flag))
        return self.log[-1]


def logging_renderer(rt, w, h, scene, params):
    cls = type("LoggingRenderer", (Logging, rt.host.HeadlessRenderer), {})
    r = cls(w, h)
    r.log = []
    r.set_scene(scene)
    r.params = params
    return r


key = lambda entries: [(p.frames, p.reset_flag, p.random) for p in entries]


def test_render_robust_until_is_the_loop_written_out(rt):
    """scene_c1(True) at 64 x 64, K = 8, threshold 0.1, an estimate every 8 frames: the stop of DESIGN.md 5.13 (40 frames); then a run that
    max_frames ends, with check_every and K that do not divide it, into the image"""
    sc = rt.scenes
    scene, params = sc.scene_c1(True), sc.params_c1()
    r = logging_renderer(rt, 64, 64, scene, params)
    other = rendering_context(rt, 64, 64)
    g = sc.GlibcRand(0)
    stream = [g.rand() for _ in range(96)]
    drawn = [0]

    def frame(k):
        other.render(params.replace(frames=0, reset_flag=1, random=stream[drawn[0] + k]))
        return other.read_image()

    r.render_frame()                                               # one ordinary frame and a pending reset: the session leaves both alone
    r.reset_buffer()
    drawn[0] = 1
    done, summary, picture = r.render_robust_until(0.1, 64, check_every=8)
    want_done, want_summary, sess = rem.render_until(frame, 8, 0.1, 64, check_every=8)
    assert done == want_done == 40 and summary["converged"] == 1 and r.ctx.robust_frames() == (40, 8)
    assert em.same_result(dict(summary, tiles=r.ctx.read_robust_error_tiles()), want_summary) == []
    assert same(picture, sess.resolve(1.0)) and same(r.ctx.read_robust(), picture)
    assert key(r.log) == [(1, 0, stream[0])] + [(0, 1, stream[1 + k]) for k in range(40)]
    assert (r.m_frames, r.m_reset) == (1, True)
    drawn[0] = 41
    done, summary, picture = r.render_robust_until(1e-6, 13, check_every=5, buckets=4, gain=0.5, to_image=True, quantile_permille=1000, floor=0.02)
    want_done, want_summary, sess = rem.render_until(frame, 4, 1e-6, 13, check_every=5, gain=0.5, quantile_permille=1000, floor=0.02)
    assert done == want_done == 13 and summary["converged"] == 0 and summary["frames_now"] == 13
    assert em.same_result(dict(summary, tiles=r.ctx.read_robust_error_tiles()), want_summary) == []
    assert same(picture, sess.resolve(0.5, rm.DEST_IMAGE)) and same(r.ctx.read_image(), picture)
    done, summary, picture = r.render_robust_until(0.1, 3, buckets=4)      # fewer frames than buckets: no estimate, the picture all the same
    assert done == 3 and summary is None and picture.shape == (64, 64, 4) and r.ctx.robust_frames() == (3, 4)
    p = r.render_frame()                                           # the pending reset is still pending, for the next ordinary frame
    assert (p.frames, p.reset_flag, p.random) == (2, 1, stream[57]) and (r.m_frames, r.m_reset) == (0, False)
    for bad in (dict(max_frames=0), dict(max_frames=8, check_every=0)):
        with pytest.raises(ValueError):
            r.render_robust_until(0.1, **bad)
    r.ctx.close()
    other.close()


def test_the_facade_and_the_headless_renderer_are_twins(rt, tmp_path):
    """tests/cpp/facade_robust_until.cpp in a child process: its log of uniforms, stop frames, summaries and pictures against
    host.HeadlessRenderer through the same calls, and its hand-made estimate against the mirror fed with its own buckets"""
    w, h = 70, 53
    exe = build_program(rt, tmp_path, "facade_robust_until")
    d = str(tmp_path)
    try:
        run = subprocess.run([exe, d, str(w), str(h)], cwd=d, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("facade_robust_until did not end within its time limit")
    assert run.returncode == 0, f"facade_robust_until ended with {run.returncode}:\n{run.stderr[-2000:]}"
    H_, sc = rt.host, rt.scenes
    raw = lambda name, dtype: np.fromfile(os.path.join(d, name + ".raw"), dtype)
    blob = open(os.path.join(d, "params.raw"), "rb").read()
    n = C.sizeof(H_.CFrameParams)
    used = [H_.CFrameParams.from_buffer_copy(blob[i:i + n]) for i in range(0, len(blob), n)]
    a, frames_a, b, frames_b, logged = (int(v) for v in raw("returns", np.int64))
    assert logged == len(used) == 1 + 1 + a + b + 2
    summaries = [H_.Context._summary_dict(H_.CErrorSummary.from_buffer_copy(raw("summaries", np.uint8)[i * 64:(i + 1) * 64].tobytes())) for i in range(3)]
    scene = sc.Scene(spheres=raw("spheres", f32).reshape(-1, 8), materials=raw("materials", f32).reshape(-1, 8), nodes=raw("nodes", f32).reshape(-1, 12))
    fields = {name: getattr(used[0], name) for name, _ in H_.CFrameParams._fields_}
    fields = {k: (tuple(v) if hasattr(v, "__len__") else v) for k, v in fields.items()}
    fields.update(frames=0, reset_flag=0, random=0)
    r = logging_renderer(rt, w, h, scene, sc.FrameParams(**fields))
    r.ctx.robust_begin()
    r.ctx.render(r.session_frame(reset_flag=1), sync=False)
    r.ctx.robust_accumulate()
    r.render_frame()
    r.reset_buffer()
    done, first, picture = r.render_robust_until(0.35, 40, check_every=6, buckets=4)
    assert done == a == frames_a and 4 <= a <= 40 and repr(first) == repr(summaries[0])
    assert same(picture, raw("picture_first", f32).reshape(h, w, 4))
    planes = np.stack([raw(f"bucket{j}", f32).reshape(h, w, 4) for j in range(4)])
    hand = dict(gain=0.0, quantile_permille=500, threshold=0.2)
    r.ctx.robust_error_estimate(**hand)
    want = rem.estimate(planes, a, **hand)
    assert em.same_result(dict(summaries[1], tiles=want["tiles"]), want) == [] and em.same_result(device_result(r.ctx), want) == []
    done, second, picture = r.render_robust_until(1e-6, 21, check_every=8, buckets=8, gain=0.5, to_image=True, quantile_permille=500)
    assert done == b == frames_b == 21 and repr(second) == repr(summaries[2]) and second["converged"] == 0
    assert same(picture, raw("picture_second", f32).reshape(h, w, 4))
    r.run(2)
    assert key(r.log) == key(used)
    assert same(r.ctx.read_image(), raw("final_image", f32).reshape(h, w, 4))
    r.ctx.close()
