"""rtgl_guides_frame (include/rtgl_amd.h, "guide pass") on the device: the first-hit planes without a frame.

The reference is the frame path itself on a twin context: a guide pass after a restart must leave the four planes bit for bit as a frame
of the same parameters leaves them, a sequence of frames and passes must equal tests/guides_mirror.py's fold of the entries' own planes,
and nothing else of a context may move -- image, RNG states, counters, denoised and display buffers, the error snapshot, the sessions, and
every later frame.  No new arithmetic: everything is compared bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_guided_mirror as dgm
import denoise_mirror as dm
import golden_cases as gc
import guides_mirror as gm
import raytracer_glsl_amd
import robust_denoise_mirror as rdm

pytestmark = pytest.mark.gpu

H_ = raytracer_glsl_amd.host
ALBEDO, NORMAL, POSITION, IDS, ALL = H_.AOV_ALBEDO, H_.AOV_NORMAL, H_.AOV_POSITION, H_.AOV_IDS, H_.AOV_ALL
PLANES = (ALBEDO, NORMAL, POSITION, IDS)
GUIDES = ALBEDO | NORMAL | POSITION
ERR_INVALID, ERR_STATE = -1, -4
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_aov.py does)"""
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def randoms(rt):
    g = rt.scenes.GlibcRand(0)
    return [g.rand() for _ in range(40)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and (bits(a) == bits(b)).all()


def named(rt, name):
    """(scene, the parameters of the case's first frame)"""
    case = gc.build_cases(rt.scenes)[name]
    return case["scene"](), case["frames"][0]


def context(rt, scene, w, h, aov=ALL, options=(), **kw):
    ctx = rt.host.Context(w, h, **kw)
    for key, value in options:
        ctx.set_option(key, value)
    ctx.upload_scene(scene)
    if aov:
        ctx.set_aov(aov)
    return ctx


def planes_of(ctx, mask=None):
    mask = ctx.get_option("aov") if mask is None else mask
    return {p: ctx.read_aov(p) for p in PLANES if mask & p}


def assert_planes(got, want, label):
    assert sorted(got) == sorted(want), label
    for p in want:
        neq = (bits(got[p]) != bits(want[p])).any(axis=2)
        assert not neq.any(), f"{label}: plane {p}: {int(neq.sum())} of {neq.size} pixels differ, first at (row, column) {list(zip(*np.nonzero(neq)))[:6]}"


def frame_planes(rt, scene, w, h, p, aov=ALL, options=()):
    """the planes a frame of `p` writes on a fresh context: the reference of a pass, and an entry of the mirror's fold"""
    ctx = context(rt, scene, w, h, aov, options)
    ctx.render(p)
    out = planes_of(ctx)
    ctx.close()
    for a in out.values():
        a.setflags(write=False)
    return out


def as_frame(p):
    """P': the frame whose planes a pass of P must write"""
    return p.replace(max_bounce=max(p.max_bounce, 1), samples=1)


# ---------------------------------------------------------------------------------------------- 1. twin equality

SPHERE_SCENES = ["c1_256", "spheres_deep_chain", "env_incomplete_cube"]
MESH_SCENES = ["mesh_env_dof", "mesh_two_meshes_overlap", "mesh_stacked_duplicates", "mesh_backfacing"]


def check_twin(rt, scene, p, w, h, aov=ALL, options=(), label=""):
    want = frame_planes(rt, scene, w, h, as_frame(p), aov, options)
    ctx = context(rt, scene, w, h, aov, options)
    ctx.guides_frame(p)
    assert_planes(planes_of(ctx), want, f"{label}: pass")
    fh, fw = gm.footprint(h, w)
    for k, a in planes_of(ctx).items():
        assert not a[fh:].any() and not a[:, fw:].any(), f"{label}: plane {k} written outside the dispatch footprint"
    if fh and fw:
        assert ctx.last_frame_ms() > 0
    # what a pass ignores: max_bounce = 0 (the ray is traced all the same), samples, reset_flag, frames
    ctx.clear_image()
    ctx.guides_frame(p.replace(max_bounce=0, samples=3, reset_flag=1, frames=41))
    assert_planes(planes_of(ctx), want, f"{label}: pass with max_bounce 0, samples 3, reset_flag 1")
    ctx.close()
    return want


@pytest.mark.parametrize("name", SPHERE_SCENES)
def test_a_pass_equals_a_frame_on_scenes_without_triangles(rt, name):
    scene, p = named(rt, name)
    for options in ((), (("kernel", 0),), (("kernel", 1),), (("kernel", 2),), (("kernel", 4),)):
        want = check_twin(rt, scene, p, 64, 64, options=options, label=f"{name} {options}")
    kinds = want[IDS][..., 0]
    assert (kinds == 0).any() if name == "env_incomplete_cube" else (kinds == 1).any()


@pytest.mark.parametrize("kernel", [0, 1, 2, 4])
@pytest.mark.parametrize("name", MESH_SCENES)
def test_a_pass_equals_a_frame_on_scenes_with_triangles(rt, name, kernel):
    scene, p = named(rt, name)
    want = check_twin(rt, scene, p, 64, 64, options=(("kernel", kernel),), label=f"{name} kernel {kernel}")
    assert (want[IDS][..., 0] == 2).any() == (name != "mesh_backfacing")      # (a triangle seen from behind is no hit: the scan finds nothing)
    # the result does not depend on option "kernel": kernel 4's frame is the reference of all
    if kernel != 4:
        assert_planes(want, frame_planes(rt, scene, 64, 64, as_frame(p), options=(("kernel", 4),)), f"{name}: frames of kernels {kernel} and 4")


def test_depth_of_field_on_and_off(rt):
    scene, p = named(rt, "mesh_env_dof")
    assert p.use_dof
    a = check_twin(rt, scene, p, 64, 64, label="dof on")
    b = check_twin(rt, scene, p.replace(use_dof=0), 64, 64, label="dof off")
    assert not same(a[POSITION], b[POSITION])


@pytest.mark.parametrize("size", [(70, 53), (8, 8), (72, 24), (7, 9), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes(rt, size):
    w, h = size
    for name in ("mesh_env_dof", "c1_256"):
        scene, p = named(rt, name)
        want = check_twin(rt, scene, p, w, h, label=f"{name} {w} x {h}")
        if min(w, h) < 8:                                  # an empty footprint: the call is OK and nothing is written
            assert not any(a.any() for a in want.values())


@pytest.mark.parametrize("mask", [ALBEDO, NORMAL, POSITION, IDS, ALL])
def test_plane_masks(rt, mask):
    scene, p = named(rt, "mesh_two_meshes_overlap")
    want = check_twin(rt, scene, p, 40, 24, aov=mask, label=f"mask {mask}")
    assert sorted(want) == [b for b in PLANES if mask & b]
    full = frame_planes(rt, scene, 40, 24, as_frame(p))
    assert_planes(want, {k: full[k] for k in want}, f"mask {mask} against all planes")


# ---------------------------------------------------------------------------------------------- 2. accumulation

def sequence_params(p, randoms):
    return [p.replace(frames=k + 1, reset_flag=0, random=randoms[k]) for k in range(4)]


@pytest.mark.parametrize("name, options", [("mesh_env_dof", ()), ("mesh_env_dof", (("kernel", 2),)), ("c1_256", ())], ids=["mesh-kernel4", "mesh-kernel2", "spheres"])
def test_frames_and_passes_fold_into_one_mean(rt, randoms, name, options):
    scene, base = named(rt, name)
    w, h = 70, 53
    ps = sequence_params(base, randoms)
    singles = [frame_planes(rt, scene, w, h, as_frame(p), options=options) for p in ps]
    assert not same(singles[0][POSITION], singles[1][POSITION])      # (the jitter moves the hits)
    ctx = context(rt, scene, w, h, options=options)
    ctx.render(ps[0]); ctx.guides_frame(ps[1]); ctx.guides_frame(ps[2]); ctx.render(ps[3])
    assert_planes(planes_of(ctx), gm.fold(singles, h, w).planes, "frame, pass, pass, frame")
    # restarts: rtgl_clear_image, setting "aov", rtgl_adaptive_begin -- the next pass is entry 1; a reset frame is entry 1 itself
    ctx.clear_image(); ctx.guides_frame(ps[1])
    assert_planes(planes_of(ctx), gm.fold(singles[1:2], h, w).planes, "after rtgl_clear_image")
    ctx.guides_frame(ps[2])
    assert_planes(planes_of(ctx), gm.fold(singles[1:3], h, w).planes, "after rtgl_clear_image, second pass")
    ctx.set_aov(ALL); ctx.guides_frame(ps[3]); ctx.guides_frame(ps[0])
    assert_planes(planes_of(ctx), gm.fold([singles[3], singles[0]], h, w).planes, "after setting aov")
    ctx.adaptive_begin(); ctx.guides_frame(ps[2])
    assert_planes(planes_of(ctx), gm.fold(singles[2:3], h, w).planes, "after rtgl_adaptive_begin")
    ctx.render(ps[0].replace(reset_flag=1)); ctx.guides_frame(ps[1]); ctx.guides_frame(ps[3])
    assert_planes(planes_of(ctx), gm.fold([singles[0], singles[1], singles[3]], h, w).planes, "after a reset frame")
    ctx.close()


# ---------------------------------------------------------------------------------------------- 3. nothing else moves

def test_a_pass_writes_the_planes_only(rt, randoms):
    scene, base = named(rt, "mesh_env_dof")
    w, h = 64, 64
    ctx = context(rt, scene, w, h, options=(("rng_state", 1), ("counters", 1)))
    ps = sequence_params(base, randoms)
    ctx.render(ps[0]); ctx.render(ps[1])
    ctx.denoise(); ctx.denoise_guided(); ctx.tonemap()

    def others():
        return [ctx.read_image(), ctx.read_rng_state(), ctx.read_denoised(), ctx.read_denoise_variance(), ctx.read_display()]
    before, counted = others(), ctx.counters()
    assert counted["paths"] == w * h
    seen = planes_of(ctx)
    ctx.guides_frame(ps[2])
    assert not same(planes_of(ctx)[POSITION], seen[POSITION])
    for name, a, b in zip(("image", "RNG states", "denoised", "variance", "display"), before, others()):
        assert same(a, b), name
    assert ctx.counters() == counted
    ctx.close()


def rest_params(base, randoms):
    """frames of a camera at rest: the kept camera bits are in use from the second on"""
    return [base.replace(frames=k + 1, reset_flag=0, random=randoms[k]) for k in range(4)]


@pytest.mark.parametrize("lean", [0, 1])
@pytest.mark.parametrize("planes_off_for_frames", [False, True], ids=["planes-on", "planes-off-for-frames"])
def test_later_frames_are_those_of_a_context_without_the_pass(rt, randoms, lean, planes_off_for_frames):
    """F1, F2, pass, F3 against F1, F2, F3 (kernel 4, a mesh, the camera at rest): image and RNG states.  With the planes on the lean
    camera bounce is never taken; the second form switches them on for the pass alone, so that F3 is a lean frame on kept bits."""
    scene, base = named(rt, "mesh_env_dof")
    w, h = 72, 40
    ps = rest_params(base, randoms)
    options = (("kernel", 4), ("rng_state", 1), ("camera_lean", lean))
    aov = 0 if planes_off_for_frames else ALL
    a, b = context(rt, scene, w, h, aov, options), context(rt, scene, w, h, aov, options)
    for p in ps[:2]:
        a.render(p); b.render(p)
    if planes_off_for_frames:
        a.set_aov(ALL)
    a.guides_frame(ps[3])
    if planes_off_for_frames:
        a.set_aov(0)
    a.render(ps[2]); b.render(ps[2])
    assert same(a.read_image(), b.read_image()) and same(a.read_rng_state(), b.read_rng_state())
    a.render(ps[3]); b.render(ps[3])
    assert same(a.read_image(), b.read_image()) and same(a.read_rng_state(), b.read_rng_state())
    if planes_off_for_frames:
        assert a.get_option("camera_lean_frames") == b.get_option("camera_lean_frames")
        if lean:                                             # the kept bits were in use: frames behind the first took the lean camera bounce on them
            assert a.get_option("camera_lean_frames") >= 1
    a.close(); b.close()


def test_the_error_estimate_does_not_see_a_pass(rt, randoms):
    scene, base = named(rt, "mesh_env_dof")
    w, h = 64, 48
    ps = [base.replace(frames=k + 1, reset_flag=0, random=randoms[k]) for k in range(4)]
    out = []
    for with_pass in (False, True):
        ctx = context(rt, scene, w, h)
        ctx.render(ps[0]); ctx.render(ps[1])
        ctx.error_estimate()
        if with_pass:
            ctx.guides_frame(ps[3])
        ctx.render(ps[2])
        if with_pass:
            ctx.guides_frame(ps[0])
        ctx.render(ps[3])
        ctx.error_estimate()
        out.append((ctx.read_error_summary(), ctx.read_error_tiles()))
        ctx.close()
    assert out[0][0] == out[1][0] and out[0][0]["valid"] == 1 and (out[0][0]["frames_now"], out[0][0]["frames_snapshot"]) == (4, 2)
    assert out[0][1].tobytes() == out[1][1].tobytes()


# ---------------------------------------------------------------------------------------------- 4. sessions

def guide_arrays(ctx):
    return [ctx.read_aov(p) for p in (ALBEDO, NORMAL, POSITION)]


def check_pair(got, want, label):
    for name, g, w_ in zip(("denoised", "variance"), got, want):
        nan = np.isnan(w_)
        bad = np.where(nan, ~np.isnan(g), bits(g) != bits(w_))
        assert not bad.any(), f"{label}: {name}: {int(bad.sum())} of {bad.size} components differ"


def test_an_adaptive_session_can_be_denoised(rt, randoms):
    scene, base = named(rt, "mesh_env_dof")
    w, h = 64, 64
    a, b = context(rt, scene, w, h, aov=0), context(rt, scene, w, h, aov=0)
    for ctx in (a, b):
        ctx.adaptive_begin(min_samples=4, max_samples=64)
        for k in range(8):
            ctx.adaptive_frame(base.replace(random=randoms[k]))
    image = a.read_image()
    assert same(image, b.read_image())
    a.set_aov(GUIDES)
    assert a.lib.rtgl_denoise_guided(a.h, None) == ERR_STATE      # zeroed planes: no frame since they restarted
    singles = []
    for k in range(4):
        p = base.replace(random=randoms[8 + k])
        a.guides_frame(p)
        singles.append(frame_planes(rt, scene, w, h, as_frame(p), aov=GUIDES))
    assert_planes(planes_of(a), gm.fold(singles, h, w, GUIDES).planes, "four passes in an adaptive session")
    a.denoise_guided()
    check_pair((a.read_denoised(), a.read_denoise_variance()), dgm.denoise_guided(a.read_image(), *guide_arrays(a), **dgm.DEFAULTS), "adaptive session")
    assert same(a.read_image(), image)
    sa, sb = a.adaptive_update(), b.adaptive_update()       # the session is open, and its records are the twin's
    assert sa == sb and sa["samples_max"] == 8
    assert a.read_adaptive_tiles().tobytes() == b.read_adaptive_tiles().tobytes()
    a.close(); b.close()


def test_a_robust_adaptive_session_can_be_denoised(rt, randoms):
    scene, base = named(rt, "mesh_env_dof")
    w, h = 64, 64
    a, b = context(rt, scene, w, h, aov=0), context(rt, scene, w, h, aov=0)
    for ctx in (a, b):
        ctx.robust_adaptive_begin(buckets=4, min_samples=4, max_samples=64)
        for k in range(8):
            ctx.robust_adaptive_frame(base.replace(random=randoms[k]))
    a.set_aov(GUIDES)
    for k in range(4):
        a.guides_frame(base.replace(random=randoms[8 + k]))
    sa, sb = a.robust_adaptive_update(), b.robust_adaptive_update()
    assert sa == sb and a.read_robust_adaptive_tiles().tobytes() == b.read_robust_adaptive_tiles().tobytes()
    for ctx in (a, b):
        ctx.robust_adaptive_resolve(dest=H_.ROBUST_DEST_IMAGE)
    image = a.read_image()
    assert same(image, b.read_image()) and image[..., :3].any()
    a.denoise()
    got, want = a.read_denoised(), dm.denoise(image, *guide_arrays(a), **dm.DEFAULTS)
    nan = np.isnan(want)
    assert not np.where(nan, ~np.isnan(got), bits(got) != bits(want)).any()
    assert same(a.read_image(), image)
    a.close(); b.close()


def test_a_robust_session_takes_passes_between_its_folds(rt, randoms):
    sc = rt.scenes
    scene, base = sc.scene_c1(True), sc.params_c1()
    w, h, K, N = 64, 48, 4, 8
    a, b = context(rt, scene, w, h, aov=GUIDES), context(rt, scene, w, h, aov=GUIDES)
    for ctx in (a, b):
        ctx.robust_begin(buckets=K)
        for k in range(N):
            ctx.render(base.replace(frames=0, reset_flag=1, random=randoms[k]), sync=False)
            if ctx is a and k % 3 == 0:                      # (behind frames 0, 3 and 6: the last frame, 7, restarts the planes alone)
                ctx.guides_frame(base.replace(random=randoms[20 + k]), sync=False)
            ctx.robust_accumulate()
    last = planes_of(b)                                      # the session's guides of before: the last frame's hit
    singles = [{p: last[p] for p in last}]
    for k in range(4):
        p = base.replace(random=randoms[30 + k])
        a.guides_frame(p)
        singles.append(frame_planes(rt, scene, w, h, as_frame(p), aov=GUIDES))
    assert a.robust_frames() == b.robust_frames() == (N, K)
    buckets = np.stack([a.read_robust_bucket(j) for j in range(K)])
    assert same(buckets, np.stack([b.read_robust_bucket(j) for j in range(K)]))
    assert_planes(planes_of(a), gm.fold(singles, h, w, GUIDES).planes, "the last frame and four passes")
    a.robust_denoise()
    want = rdm.robust_denoise(buckets, N, *guide_arrays(a), **rdm.DEFAULTS)
    check_pair((a.read_denoised(), a.read_denoise_variance()), want, "robust session")
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 5. refusals

def test_refusals_move_nothing(rt, randoms):
    scene, base = named(rt, "mesh_env_dof")
    w, h = 40, 24
    lib = rt.host.load_library()
    assert lib.rtgl_guides_frame(None) == ERR_INVALID
    ctx = context(rt, scene, w, h)                           # the planes on, zeroed, a restart pending; no frame parameters
    zero = planes_of(ctx)
    assert lib.rtgl_guides_frame(ctx.h) == ERR_STATE
    assert b"rtgl_set_frame_params" in lib.rtgl_last_error(ctx.h)
    assert_planes(planes_of(ctx), zero, "refused without frame parameters")
    ps = sequence_params(base, randoms)
    singles = [frame_planes(rt, scene, w, h, as_frame(p)) for p in ps[:2]]
    ctx.guides_frame(ps[0])
    held = planes_of(ctx)
    ctx.set_aov(0)
    assert lib.rtgl_guides_frame(ctx.h) == ERR_STATE
    assert b"aov" in lib.rtgl_last_error(ctx.h) and len(lib.rtgl_last_error(ctx.h)) > 10
    with pytest.raises(rt.host.RtglError):
        ctx.guides_frame(ps[1])
    ctx.close()
    # the count: a refused call neither consumes a pending restart nor counts as an entry
    ctx = context(rt, scene, w, h)
    assert lib.rtgl_guides_frame(ctx.h) == ERR_STATE
    ctx.guides_frame(ps[0])
    assert_planes(planes_of(ctx), held, "the first pass behind a refused call")
    ctx.guides_frame(ps[1])
    assert_planes(planes_of(ctx), gm.fold(singles, h, w).planes, "two passes behind a refused call")
    ctx.close()


def test_a_multi_device_handle_is_refused(rt):
    scene, base = named(rt, "c1_256")
    ctx = context(rt, scene, 32, 32, devices=[0, 0], strip_rows=8)
    ctx.set_params(base)
    assert ctx.lib.rtgl_guides_frame(ctx.h) == ERR_STATE and b"multi-device" in ctx.lib.rtgl_last_error(ctx.h)
    ctx.close()


# ---------------------------------------------------------------------------------------------- 6. tiled

@pytest.mark.parametrize("name", ["mesh_env_dof", "c1_256"])
def test_tiled_contexts_work_on_their_strips(rt, randoms, name):
    scene, base = named(rt, name)
    w, h = 70, 53
    ps = sequence_params(base, randoms)[:2]
    whole = context(rt, scene, w, h)
    for p in ps:
        whole.guides_frame(p)
    want = planes_of(whole)
    whole.close()
    union = {p: np.zeros_like(a) for p, a in want.items()}
    rows_seen = []
    for rank in range(2):
        ctx = context(rt, scene, w, h, rank=rank, world=2, strip_rows=8)
        for p in ps:
            ctx.guides_frame(p)
        rows = ctx.global_rows()
        rows_seen += list(rows)
        for p, a in planes_of(ctx).items():
            union[p][rows] = a
        ctx.close()
    assert sorted(rows_seen) == list(range(h))
    assert_planes(union, want, "the union of two ranks")


# ---------------------------------------------------------------------------------------------- 7. facade

def test_the_facade_makes_the_same_passes(rt, tmp_path):
    from test_facade_post import build_program
    w, h = 70, 53
    exe = build_program(rt, tmp_path, "facade_guides")
    d = str(tmp_path)
    try:
        run = subprocess.run([exe, d, str(w), str(h)], cwd=d, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("facade_guides did not end within its time limit")
    assert run.returncode == 0, f"facade_guides ended with {run.returncode}:\n{run.stderr[-2000:]}"
    sc = rt.scenes
    raw = lambda name, dtype=f32: np.fromfile(os.path.join(d, name + ".raw"), dtype)
    blob = open(os.path.join(d, "params.raw"), "rb").read()
    n = C.sizeof(H_.CFrameParams)
    used = [H_.CFrameParams.from_buffer_copy(blob[i:i + n]) for i in range(0, len(blob), n)]
    assert len(used) == 3 and len({p.random for p in used}) == 3 and all(p.frames == 0 and p.reset_flag == 0 for p in used)
    scene = sc.Scene(spheres=raw("spheres").reshape(-1, 8), materials=raw("materials").reshape(-1, 8), nodes=raw("nodes").reshape(-1, 12))
    ctx = context(rt, scene, w, h)
    for p in used:                                           # the C ABI with the facade's own parameter records
        assert ctx.lib.rtgl_set_frame_params(ctx.h, C.byref(p)) == 0 and ctx.lib.rtgl_guides_frame(ctx.h) == 0
    got = planes_of(ctx)
    for plane, name in ((ALBEDO, "albedo"), (NORMAL, "normal"), (POSITION, "position")):
        assert same(got[plane], raw(name).reshape(h, w, 4)), name
    assert same(got[IDS], raw("ids", np.int32).reshape(h, w, 4).astype(got[IDS].dtype)), "ids"
    assert not raw("image").any()                            # the facade's passes left its image as created
    ctx.close()
    # host.HeadlessRenderer, the Python twin: one rand() per pass, the parameters returned
    r = rt.host.HeadlessRenderer(w, h, aov=ALL)
    r.set_scene(scene)
    fields = {name: getattr(used[0], name) for name, _ in H_.CFrameParams._fields_}
    fields = {k: (tuple(v) if hasattr(v, "__len__") else v) for k, v in fields.items()}
    fields.update(frames=0, reset_flag=0, random=0)
    r.params = sc.FrameParams(**fields)
    for _ in range(2):                                       # the program's two refused calls drew a word each: the facade marshals first
        r._rand.rand()
    mine = r.render_guides(3)
    assert [(p.frames, p.reset_flag, p.random) for p in mine] == [(p.frames, p.reset_flag, p.random) for p in used]
    assert_planes(planes_of(r.ctx), got, "HeadlessRenderer.render_guides")
    assert r.m_frames == 0
    r.ctx.close()
