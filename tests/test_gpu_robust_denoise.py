"""rtgl_robust_denoise on the device (include/rtgl_amd.h, "robust denoise").

The reference is the numpy restatement, tests/robust_denoise_mirror.py, pinned by tests/test_robust_denoise_mirror.py.  The comparison
rule is that of tests/test_gpu_denoise_inputs.py (`check`): where the mirror's component is not a NaN the device's has the same bits, no
tolerance; where it is a NaN the device's is a NaN.  The bucket planes are injected through write_image and robust_accumulate, the first-hit
planes through tensors over rtgl_device_aov."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_guided_mirror as gm
import robust_denoise_inputs as rdi
import robust_denoise_mirror as rdm
import robust_mirror as rm
import tonemap_mirror as tmm
from test_facade_post import build_program
from test_gpu_denoise import ALBEDO, GUIDES, NORMAL, POSITION, same
from test_gpu_denoise_inputs import check, plane_tensor, prepared

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
f32 = np.float32
PLANES = (ALBEDO, NORMAL, POSITION)


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


def fold(ctx, samples, K):
    """a session of the device and the mirror's, fed with the same samples"""
    h, w = samples[0].shape[:2]
    sess = rm.Session(h, w, K)
    ctx.robust_begin(buckets=K)
    for s in samples:
        ctx.write_image(s)
        ctx.robust_accumulate()
        sess.accumulate(s)
    return sess


def put_planes(ctx, albedo, normal, position):
    """the first-hit planes that are enabled take the arrays (copies, not a kernel's stores); read back, so that no case runs on other data"""
    import torch
    ctx.synchronize()
    enabled = ctx.get_option("aov")
    for plane, a in zip(PLANES, (albedo, normal, position)):
        if enabled & plane:
            plane_tensor(ctx, plane).copy_(torch.from_numpy(np.ascontiguousarray(a, f32)))
    torch.cuda.synchronize()
    for plane, a in zip(PLANES, (albedo, normal, position)):
        assert not enabled & plane or same(ctx.read_aov(plane), a)


def mirror_args(ctx, albedo, normal, position):
    enabled = ctx.get_option("aov")
    return [a if enabled & plane else None for plane, a in zip(PLANES, (albedo, normal, position))]


def check_calls(ctx, sess, guides, params_list, passes_list, label):
    for params in params_list:
        budget = rdi.nan_budget(sess.planes, guides[0] if dict(rdm.DEFAULTS, **params)["demodulate"] else None)
        want = rdm.robust_denoise_each(sess.planes, sess.N, *guides, passes_list=tuple(passes_list), **dict(rdm.DEFAULTS, **params))
        for k in passes_list:
            ctx.robust_denoise(passes=k, **params)
            tag = f"{label} {params} passes {k}"
            check(ctx.read_denoised(), want[k][0], budget, tag + ": denoised")
            check(ctx.read_denoise_variance(), want[k][1], budget, tag + ": variance")
            if k == 0 and not dict(rdm.DEFAULTS, **params)["demodulate"]:
                check(ctx.read_denoised(), rm.image_plane(sess.planes, sess.N, params.get("gain", 1.0)), budget, tag + ": not the resolve")


# ---------------------------------------------------------------------------------------------- 1. injected inputs

CASES = rdi.listed_cases()


@pytest.mark.parametrize("K", rdi.BUCKETS)
@pytest.mark.parametrize("size", rdi.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_injected_inputs_equal_the_mirror(rt, size, K):
    """the listed cases of this size and K on one context: passes 0, 1 and 5 of every parameter set"""
    w, h = size
    ctx = prepared(rt, w, h)
    mine = [c for c in CASES if c[2] == size and c[3] == K]
    assert mine
    for family, guides, _, _, sets in mine:
        case = rdi.make(family, guides, h, w, K, sets)
        sess = fold(ctx, case["samples"], K)
        arrays = (case["albedo"], case["normal"], case["position"])
        put_planes(ctx, *arrays)
        check_calls(ctx, sess, arrays, case["params"], rdi.PASSES, f"{family} / {guides} {w} x {h} K = {K}")
    ctx.close()


def test_eight_passes(rt):
    """step 128 at one size: the wide segments of the pass kernel"""
    w, h, K = 130, 9, 8
    ctx = prepared(rt, w, h)
    case = rdi.make("long", "benign", h, w, K, (0, 1))
    sess = fold(ctx, case["samples"], K)
    arrays = (case["albedo"], case["normal"], case["position"])
    put_planes(ctx, *arrays)
    check_calls(ctx, sess, arrays, case["params"], (8,), "eight passes")
    ctx.close()


@pytest.mark.parametrize("mask, params", [(ALBEDO | POSITION, dict(sigma_normal=0.0)), (ALBEDO | NORMAL, dict(sigma_position=0.0)),
                                          (NORMAL, dict(sigma_position=0.0, demodulate=False)), (0, dict(sigma_normal=0.0, sigma_position=0.0, demodulate=False))],
                         ids=["no_normal", "no_position", "normal_alone", "no_plane"])
def test_a_term_that_is_off_needs_no_plane(rt, mask, params):
    w, h, K = 70, 53, 8
    sc = rt.scenes
    ctx = rt.host.Context(w, h)
    ctx.upload_scene(sc.scene_c1(True))
    ctx.set_aov(mask)
    ctx.render(sc.params_c1().replace(frames=0, reset_flag=1))
    case = rdi.make("ragged", "edges", h, w, K, (0,))
    sess = fold(ctx, case["samples"], K)
    arrays = (case["albedo"], case["normal"], case["position"])
    put_planes(ctx, *arrays)
    check_calls(ctx, sess, mirror_args(ctx, *arrays), [dict(params, gain=g) for g in (0.0, 1.0, 4.0)], rdi.PASSES, f"planes {mask}")
    ctx.close()


# ---------------------------------------------------------------------------------------------- 2. rendered frames

@pytest.fixture(scope="module")
def randoms(rt):
    g = rt.scenes.GlibcRand(0)
    return [g.rand() for _ in range(32)]


def rendered_session(rt, randoms, w=70, h=53, K=8, N=16, options=(), sync=False):
    sc = rt.scenes
    ctx = rt.host.Context(w, h)
    ctx.upload_scene(sc.scene_c1(True))
    ctx.set_aov(GUIDES)
    for key, value in options:
        ctx.set_option(key, value)
    ctx.robust_begin(buckets=K)
    base = sc.params_c1()
    for k in range(N):
        ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=sync)
        ctx.robust_accumulate()
    return ctx


def mirror_of_session(ctx, K, N, passes_list=(5,), **params):
    planes = np.stack([ctx.read_robust_bucket(j) for j in range(K)])
    guides = [ctx.read_aov(p) for p in PLANES]
    return rdm.robust_denoise_each(planes, N, *guides, passes_list=tuple(passes_list), **dict(rdm.DEFAULTS, **params))


def test_a_rendered_session_equals_the_mirror_fed_with_its_buckets(rt, randoms):
    K, N = 8, 16
    ctx = rendered_session(rt, randoms, K=K, N=N)
    for params in (dict(), dict(demodulate=False, gain=0.0), dict(gain=4.0, sigma_lum=2.0)):
        want = mirror_of_session(ctx, K, N, (0, 2, 5), **params)
        for k in (0, 2, 5):
            ctx.robust_denoise(passes=k, **params)
            check(ctx.read_denoised(), want[k][0], 0.0, f"{params} passes {k}: denoised")
            check(ctx.read_denoise_variance(), want[k][1], 0.0, f"{params} passes {k}: variance")
    got = ctx.read_denoise_variance()
    assert (got[..., 3] >= 2).all() and (got[..., 3] <= K).all() and np.isfinite(got).all() and (got[..., 1] > 0).any()
    ctx.close()


def test_frames_held_by_a_batching_context_are_submitted_first(rt, randoms):
    """frame_batch = 3 and two frames rendered behind the last fold.  A context holds frames back only while "aov" is 0 and the scene has
    triangles, so the call is one that needs no plane; the image is bound to a tensor, which shows without a library call that the two
    frames were still held in front of rtgl_robust_denoise and are in the image behind it."""
    import torch
    sc = rt.scenes
    w, h, K = 70, 53, 4
    base = sc.params_c2()
    no_planes = dict(sigma_normal=0.0, sigma_position=0.0, demodulate=False)
    tensor = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    out = []
    for batch in (3, 1):
        ctx = rt.host.Context(w, h)
        ctx.upload_scene(sc.scene_mesh(10, 5, env_size=16))
        ctx.set_option("frame_batch", batch)
        if batch > 1:
            ctx.bind_device_image(tensor.data_ptr())
        ctx.robust_begin(buckets=K)
        for k in range(K + 1):
            ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)
            ctx.robust_accumulate()
        if batch > 1:
            ctx.synchronize()
            folded = tensor.cpu().numpy()                          # the image as the last fold saw it
        for k in range(2):
            ctx.render(base.replace(frames=k, reset_flag=int(k == 0), random=randoms[K + 1 + k]), sync=False)
        if batch > 1:
            torch.cuda.synchronize()
            assert same(tensor.cpu().numpy(), folded), "the two frames were not held: this case shows nothing"
        ctx.robust_denoise(**no_planes)
        if batch > 1:
            torch.cuda.synchronize()
            assert not same(tensor.cpu().numpy(), folded), "the call did not submit the held frames"
        planes = np.stack([ctx.read_robust_bucket(j) for j in range(K)])
        want = rdm.robust_denoise(planes, K + 1, **dict(rdm.DEFAULTS, **no_planes))
        check(ctx.read_denoised(), want[0], 0.0, f"frame_batch {batch}: denoised")
        check(ctx.read_denoise_variance(), want[1], 0.0, f"frame_batch {batch}: variance")
        out.append((ctx.read_denoised(), ctx.read_denoise_variance(), ctx.read_image()))
        if batch > 1:
            ctx.bind_device_image(0)                               # detached before the tensor goes away
        ctx.close()
    assert all(same(a, b) for a, b in zip(*out)) and out[0][2][..., :3].any()


def test_frames_behind_the_last_fold_give_the_guides(rt, randoms):
    """with the planes on every frame is submitted at once, frame_batch or not: the call takes the planes of the LATEST frame, rendered
    behind the last fold, and the buckets as the folds left them"""
    K, N = 8, 16
    base = rt.scenes.params_c1()
    out = []
    for options in ([("frame_batch", 3)], []):
        ctx = rendered_session(rt, randoms, K=K, N=N, options=options)
        before = [ctx.read_aov(p) for p in PLANES]
        for k in range(3):
            ctx.render(base.replace(frames=k, reset_flag=int(k == 0), random=randoms[N + k]), sync=False)
        ctx.robust_denoise()
        got = ctx.read_denoised(), ctx.read_denoise_variance()
        assert not all(same(a, ctx.read_aov(p)) for a, p in zip(before, PLANES))      # (the planes moved on)
        want = mirror_of_session(ctx, K, N)[5]
        check(got[0], want[0], 0.0, f"{options}: denoised")
        check(got[1], want[1], 0.0, f"{options}: variance")
        out.append(got + (ctx.read_image(),))
        ctx.close()
    assert all(same(a, b) for a, b in zip(*out))


def test_a_torch_stream_gives_the_same_bits(rt, randoms):
    import torch
    K, N = 8, 16
    plain = rendered_session(rt, randoms, K=K, N=N)
    plain.robust_denoise()
    want = plain.read_denoised(), plain.read_denoise_variance()
    plain.close()
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    ctx = rt.host.Context(70, 53)
    with torch.cuda.stream(side):
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        sc = rt.scenes
        ctx.upload_scene(sc.scene_c1(True))
        ctx.set_aov(GUIDES)
        ctx.robust_begin(buckets=K)
        for k in range(N):
            ctx.render(sc.params_c1().replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)
            ctx.robust_accumulate()
        ctx.robust_denoise()
        denoised = torch.as_tensor(_device(ctx.device_denoised_ptr(), 53, 70), device="cuda:0").clone()
        side.synchronize()
    assert same(denoised.cpu().numpy(), want[0]) and same(ctx.read_denoise_variance(), want[1])
    ctx.set_stream(0)
    ctx.close()


def _device(ptr, h, w):
    from test_gpu_denoise import _DeviceArray
    assert ptr
    return _DeviceArray(ptr, (h, w, 4), "<f4")


# ---------------------------------------------------------------------------------------------- 3. refusals

def call(rt, ctx, **fields):
    p = rt.host.CRobustDenoiseParams()
    assert ctx.lib.rtgl_robust_denoise_defaults(C.byref(p)) == 0
    for k, v in fields.items():
        setattr(p, k, v)
    return ctx.lib.rtgl_robust_denoise(ctx.h, C.byref(p)), ctx.lib.rtgl_last_error(ctx.h)


def test_state_refusals(rt):
    w, h, K = 16, 8, 4
    ctx = prepared(rt, w, h)
    image = np.full((h, w, 4), 0.5, f32)
    rc, why = call(rt, ctx)
    assert rc == ERR_STATE and b"rtgl_robust_denoise" in why and b"no session" in why
    assert ctx.lib.rtgl_robust_denoise(ctx.h, None) == ERR_STATE
    ctx.robust_begin(buckets=K)
    for n in range(K):
        rc, why = call(rt, ctx)
        assert rc == ERR_STATE and b"fewer frames than buckets" in why, n
        ctx.write_image(image)
        ctx.robust_accumulate()
    assert call(rt, ctx)[0] == 0 and ctx.lib.rtgl_robust_denoise(ctx.h, None) == 0
    # invalid records on a live context
    nan, inf = float("nan"), float("inf")
    for bad in (dict(passes=9), dict(sigma_lum=nan), dict(sigma_lum=0.0), dict(sigma_lum=-1.0), dict(sigma_normal=inf), dict(sigma_position=nan), dict(gain=nan),
                dict(gain=-1.0), dict(gain=inf), dict(flags=2), dict(flags=0x80000001), dict(reserved=(0, 1)), dict(reserved=(1, 0))):
        rc, why = call(rt, ctx, **bad)
        assert rc == ERR_INVALID and why, bad
    # planes restarted: enabled again, no frame since
    ctx.set_aov(GUIDES)
    rc, why = call(rt, ctx)
    assert rc == ERR_STATE and b"restarted" in why
    assert call(rt, ctx, sigma_normal=0.0, sigma_position=0.0, flags=0)[0] == 0      # (no plane needed: nothing to wait for)
    # a missing plane
    ctx.set_aov(ALBEDO | NORMAL)
    rc, why = call(rt, ctx)
    assert rc == ERR_STATE and b"not enabled" in why
    ctx.set_aov(0)
    rc, why = call(rt, ctx, sigma_normal=0.0, sigma_position=0.0)
    assert rc == ERR_STATE and b"not enabled" in why
    ctx.robust_end()
    rc, why = call(rt, ctx, sigma_normal=0.0, sigma_position=0.0, flags=0)
    assert rc == ERR_STATE and b"no session" in why
    ctx.close()


def test_a_tiled_context_is_refused(rt):
    tiled = rt.host.Context(64, 64, rank=1, world=2, strip_rows=8)
    tiled.robust_begin(buckets=4)
    for _ in range(4):
        tiled.robust_accumulate()
    rc, why = call(rt, tiled, sigma_normal=0.0, sigma_position=0.0, flags=0)
    assert rc == ERR_STATE and b"strips" in why
    tiled.robust_resolve()                                         # the session is as it was
    tiled.close()


# ---------------------------------------------------------------------------------------------- 4. nothing else touched, downstream

def test_the_call_writes_its_own_buffers_only(rt, randoms):
    K, N = 8, 16
    ctx = rendered_session(rt, randoms, K=K, N=N, sync=True)
    ctx.robust_resolve(dest=0)
    ctx.robust_error_estimate()
    # an accumulating picture with a snapshot in progress (the session's image is whatever the last frame left)
    ctx.error_estimate(first_frames=0)                             # (a session frame is sent with frames = 0)

    def state():
        return ([ctx.read_robust_bucket(j) for j in range(K)] + [ctx.read_robust(), ctx.read_image()] + [ctx.read_aov(p) for p in PLANES]
                + [ctx.read_robust_error_tiles().view(np.uint32), ctx.read_error_tiles().view(np.uint32)])
    before = state()
    summary = ctx.read_robust_error_summary(), ctx.read_error_summary()
    for params in (dict(), dict(passes=0, demodulate=False), dict(passes=1, gain=0.0)):
        ctx.robust_denoise(**params)
    after = state()
    assert all(a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all() for a, b in zip(before, after))
    assert repr(summary) == repr((ctx.read_robust_error_summary(), ctx.read_error_summary()))
    assert ctx.robust_frames() == (N, K)
    # a following rtgl_denoise_guided still gives its own mirror's bits
    image, guides = ctx.read_image(), [ctx.read_aov(p) for p in PLANES]
    ctx.denoise_guided()
    want = gm.denoise_guided(image, *guides, **gm.DEFAULTS)
    check(ctx.read_denoised(), want[0], 0.0, "denoise_guided after robust_denoise: denoised")
    check(ctx.read_denoise_variance(), want[1], 0.0, "denoise_guided after robust_denoise: variance")
    # ... and the other way round
    ctx.robust_denoise()
    want = mirror_of_session(ctx, K, N)[5]
    check(ctx.read_denoised(), want[0], 0.0, "robust_denoise after denoise_guided")
    ctx.close()


def test_tonemap_takes_the_denoised_buffer(rt, randoms):
    K, N = 8, 16
    ctx = rendered_session(rt, randoms, K=K, N=N)
    ctx.robust_denoise()
    want = mirror_of_session(ctx, K, N)[5][0]
    for params in (dict(source=1), dict(source=1, auto=False, exposure=0.5, op=2)):
        ctx.tonemap_reset()
        ctx.tonemap(**params)
        out = tmm.tonemap(want, None, **params)
        assert (ctx.read_display() == out["display"]).all(), params
    ctx.close()


# ---------------------------------------------------------------------------------------------- 5. the facade

def test_the_facade_the_headless_renderer_and_the_mirror_agree(rt, tmp_path):
    """tests/cpp/facade_robust_denoise.cpp in a child process: the buffers it dumps against the mirror fed with its own buckets and planes,
    and against host.HeadlessRenderer through the same calls"""
    from test_gpu_robust_error import logging_renderer
    w, h, K, N = 70, 53, 8, 16
    exe = build_program(rt, tmp_path, "facade_robust_denoise")
    d = str(tmp_path)
    try:
        run = subprocess.run([exe, d, str(w), str(h)], cwd=d, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("facade_robust_denoise did not end within its time limit")
    assert run.returncode == 0, f"facade_robust_denoise ended with {run.returncode}:\n{run.stderr[-2000:]}"
    H_, sc = rt.host, rt.scenes
    raw = lambda name, dtype=f32: np.fromfile(os.path.join(d, name + ".raw"), dtype)
    pic = lambda name: raw(name).reshape(h, w, 4)
    planes = np.stack([pic(f"bucket{j}") for j in range(K)])
    guides = [pic(n) for n in ("albedo", "normal", "position")]
    hand = dict(passes=2, demodulate=False, gain=0.5, sigma_lum=2.0)
    want_default = rdm.robust_denoise(planes, N, *guides, **rdm.DEFAULTS)
    want_hand = rdm.robust_denoise(planes, N, *guides, **dict(rdm.DEFAULTS, **hand))
    check(pic("denoised_default"), want_default[0], 0.0, "facade, defaults: denoised")
    check(pic("variance_default"), want_default[1], 0.0, "facade, defaults: variance")
    check(pic("denoised_hand"), want_hand[0], 0.0, "facade, by hand: denoised")
    check(pic("variance_hand"), want_hand[1], 0.0, "facade, by hand: variance")
    blob = open(os.path.join(d, "params.raw"), "rb").read()
    n = C.sizeof(H_.CFrameParams)
    used = [H_.CFrameParams.from_buffer_copy(blob[i:i + n]) for i in range(0, len(blob), n)]
    assert len(used) == N
    scene = sc.Scene(spheres=raw("spheres").reshape(-1, 8), materials=raw("materials").reshape(-1, 8), nodes=raw("nodes").reshape(-1, 12))
    fields = {name: getattr(used[0], name) for name, _ in H_.CFrameParams._fields_}
    fields = {k: (tuple(v) if hasattr(v, "__len__") else v) for k, v in fields.items()}
    fields.update(frames=0, reset_flag=0, random=0)
    r = logging_renderer(rt, w, h, scene, sc.FrameParams(**fields))
    r.set_aov(GUIDES)
    r.render_robust(N, buckets=K)
    assert [(p.frames, p.reset_flag, p.random) for p in r.log] == [(p.frames, p.reset_flag, p.random) for p in used]
    r.robust_denoise()
    assert same(r.read_denoised(), pic("denoised_default")) and same(r.read_denoise_variance(), pic("variance_default"))
    r.robust_denoise(**hand)
    assert same(r.read_denoised(), pic("denoised_hand")) and same(r.read_denoise_variance(), pic("variance_hand"))
    r.ctx.close()
