"""The post-process methods of the C++ facade (include/rtgl/renderer.h) executed on the device.

tests/cpp/facade_post.cpp drives them on facade_demo's scene, once per size, in a child process; the tests only read what it dumped.
Nothing expected comes from the facade: traced images are the program's own log of uniforms replayed through the CPU oracle (the
ordinary frames of planes_denoise and until) or through host.Context, which test_gpu_parity / test_gpu_aov / test_gpu_adaptive /
test_gpu_robust hold to the oracle; every post-process output is the numpy mirror's, fed with the program's own dumped inputs.  Every
comparison is of bits (a NaN counts as one word, the suite's convention); there is no tolerance anywhere.  The last test drives
host.HeadlessRenderer, the Python twin, through the adaptive and robust call sequences and wants the program's uniforms and pictures."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import adaptive_mirror as am
import denoise_guided_mirror as dgm
import denoise_mirror as dm
import error_mirror as em
import robust_mirror as rm
import temporal_clip_mirror as tcm
import temporal_mirror as tm
import temporal_moments_mirror as mm
import tonemap_mirror as tmm
from test_facade import OCTAHEDRON, write_png
from test_facade_post import build_program

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (70, 53)]            # (70, 53): tests/test_gpu_adaptive.py's size that is a multiple of neither 16 nor 8 either way
IDS = [f"{w}x{h}" for w, h in SIZES]
BOUNCES = 4                             # set_bounces() of the driver
CAMERA = ("camera_position", "camera_fov", "camera_aperture", "camera_focal_length", "camera_forward", "camera_up", "camera_right")
SESSION_FIELDS = ("samples", "max_bounce", "time", "background", "use_envmap", "use_dof") + CAMERA
ADAPTIVE = dict(threshold=0.2, min_samples=2, max_samples=6)      # render_adaptive(0.2f, 6, 2, 2) and the hand-driven session
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """torch's HIP runtime is brought up before the library's in this process (as tests/test_gpu_denoise.py does)"""
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def dumps(rt, tmp_path_factory):
    """{(w, h): directory}: the driver built once and run once per size, one child at a time, each under a time limit.  A child that
    ends on a signal, the limit or a failed check fails the fixture, and with it every test of the module before it touches the device."""
    root = tmp_path_factory.mktemp("facade_post")
    exe = build_program(rt, root, "facade_post")
    env = rt.scenes.sky_cubemap(16)
    out = {}
    for w, h in SIZES:
        d = str(root / f"{w}x{h}")
        os.mkdir(d)
        with open(os.path.join(d, "mesh.obj"), "w") as f:
            f.write(OCTAHEDRON)
        for name, face in zip(("right", "left", "top", "bottom", "front", "back"), env):
            write_png(os.path.join(d, name + ".png"), face)
        try:
            run = subprocess.run([exe, d, str(w), str(h)], cwd=d, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            pytest.fail(f"facade_post {w} x {h} did not end within its time limit")
        if run.returncode != 0:
            pytest.fail(f"facade_post {w} x {h} ended with {run.returncode}:\n{run.stderr[-2000:]}")
        out[(w, h)] = d
    return out


@pytest.fixture(params=SIZES, ids=IDS)
def case(request, dumps):
    return request.param + (dumps[request.param],)


# ---------------------------------------------------------------------------------------------- helpers

def words(a):
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool((words(a) == words(b)).all()) if a.dtype == f32 else a.tobytes() == b.tobytes()


def load(d, scenario, name, h, w, dtype=f32):
    a = np.fromfile(os.path.join(d, scenario, name + ".raw"), dtype)
    assert a.size == h * w * 4, f"{scenario}/{name}: {a.size} values for {w} x {h}"      # local rows x width x 4, the facade's size
    a = a.reshape(h, w, 4)
    a.setflags(write=False)
    return a


def raw(d, scenario, name, dtype):
    return np.fromfile(os.path.join(d, scenario, name + ".raw"), dtype)


def log_of(rt, d, scenario):
    blob = open(os.path.join(d, scenario, "params.raw"), "rb").read()
    n = ctypes.sizeof(rt.host.CFrameParams)
    assert len(blob) % n == 0
    return [rt.host.CFrameParams.from_buffer_copy(blob[i:i + n]) for i in range(0, len(blob), n)]


def params_of(rt, u, **over):
    """the FrameParams of a logged record, every field"""
    kw = {name: getattr(u, name) for name, _ in rt.host.CFrameParams._fields_}
    kw = {k: (tuple(v) if hasattr(v, "__len__") else v) for k, v in kw.items()}
    kw.update(over)
    return rt.scenes.FrameParams(**kw)


def field(u, name):
    v = getattr(u, name)
    return tuple(v) if hasattr(v, "__len__") else v


def scene_of(rt, d):
    sc = rt.scenes
    verts = np.fromfile(os.path.join(d, "vertices.raw"), f32).reshape(-1, 4)
    mats = np.fromfile(os.path.join(d, "materials.raw"), f32).reshape(-1, 8)
    assert mats.tobytes() == sc.demo_materials().tobytes() and verts.shape[0] == 30
    env = np.fromfile(os.path.join(d, "envmap.raw"), np.uint8).reshape(6, 16, 16, 4)
    assert env.tobytes() == sc.sky_cubemap(16).tobytes()
    return sc.Scene(spheres=np.fromfile(os.path.join(d, "spheres.raw"), f32).reshape(-1, 8), materials=mats,
                    meshes=sc.make_meshes([(0, verts.shape[0] // 3, 6)]), vertices=verts,
                    nodes=np.fromfile(os.path.join(d, "nodes.raw"), f32).reshape(-1, 12), env=env)


def context(rt, d, w, h, aov=0):
    ctx = rt.host.Context(w, h)
    ctx.upload_scene(scene_of(rt, d))
    if aov:
        ctx.set_aov(aov)
    return ctx


def one_frame_images(rt, d, w, h, entries):
    """the one-frame image (frames = 0, reset_flag = 1) of every logged record, from an ordinary context"""
    ctx, out = context(rt, d, w, h), []
    for u in entries:
        ctx.render(params_of(rt, u, frames=0, reset_flag=1))
        img = ctx.read_image()
        img.setflags(write=False)
        out.append(img)
    ctx.close()
    return out


def stream(rt, n):
    g = rt.scenes.GlibcRand(0)
    return [g.rand() for _ in range(n)]


def check_log(rt, used, sequence, label, refused_before=0):
    """(frames, reset_flag) of every record, and u_random: the program draws from rand() nowhere else between srand(0) and the last frame
    of a scenario, so the words are glibc's stream after srand(0), one per frame of any kind; refused_before: the session frames the
    library refused before the first record (each has drawn its word and is not logged)"""
    assert [(u.frames, u.reset_flag) for u in used] == list(sequence), label
    assert [u.random for u in used] == stream(rt, refused_before + len(used))[refused_before:], label
    for u in used:
        assert (u.samples, u.max_bounce, u.use_dof, u.use_envmap) == (1, BOUNCES, 1, 1), label


def summary_dict(rt, blob, cls, names):
    s = cls.from_buffer_copy(blob)
    return s, {k: getattr(s, k) for k in names}


def pfm_of(path, img):
    h, w = img.shape[:2]
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    blob = open(path, "rb").read()
    return blob[:len(head)] == head and blob[len(head):] == np.ascontiguousarray(img[:, :, :3]).tobytes()


def decode_png(path):
    """8-bit RGBA, not interlaced; the filter types 0 (the only one include/rtgl/png_io.h writes), 1 and 2"""
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, head = 8, b"", None
    while at < len(blob):
        n, kind = struct.unpack(">I4s", blob[at:at + 8])
        data = blob[at + 8:at + 8 + n]
        assert struct.unpack(">I", blob[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif kind == b"IDAT":
            idat += data
        at += 12 + n
    w, h, depth, colour, _, _, interlace = head
    assert (depth, colour, interlace) == (8, 6, 0)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    out = np.zeros((h, w * 4), np.uint8)
    for y in range(h):
        kind, line = rows[y, 0], rows[y, 1:]
        if kind == 0:
            out[y] = line
        elif kind == 1:
            out[y] = np.cumsum(line.reshape(w, 4), 0, dtype=np.uint8).ravel()
        elif kind == 2:
            out[y] = line + (out[y - 1] if y else 0)
        else:
            raise AssertionError(f"filter type {kind} in row {y}")
    return out.reshape(h, w, 4)


# ---------------------------------------------------------------------------------------------- 1. planes, denoise, denoise_guided

def test_planes_and_both_denoisers(rt, oracle, case):
    w, h, d = case
    H_, S = rt.host, "planes_denoise"
    used = log_of(rt, d, S)
    check_log(rt, used, [(1, 0), (2, 0), (3, 0), (4, 0)], S)
    image = load(d, S, "image", h, w)
    want = np.zeros((h, w, 4), f32)
    for u in used:
        oracle.render(scene_of(rt, d), params_of(rt, u), want, threads=4)
    assert same(image, want), "read_image() against the oracle"
    ctx = context(rt, d, w, h, H_.AOV_ALL)
    for u in used:
        ctx.render(params_of(rt, u))
    assert same(ctx.read_image(), image)
    planes = {}
    for name, bit in (("albedo", H_.AOV_ALBEDO), ("normal", H_.AOV_NORMAL), ("position", H_.AOV_POSITION)):
        planes[name] = load(d, S, name, h, w)
        assert same(planes[name], ctx.read_aov(bit)), f"read_aov<float>({name})"
        assert pfm_of(os.path.join(d, S, name + ".pfm"), planes[name]), f"save_aov_pfm({name})"
    assert same(load(d, S, "ids", h, w, np.int32), ctx.read_aov(H_.AOV_IDS)), "read_aov<int32_t>(ids)"
    ctx.close()
    assert not os.path.exists(os.path.join(d, S, "ids.pfm"))
    assert planes["position"][..., 3].any() and not planes["position"][..., 3].all()       # hits and misses
    # the mirrors, fed the program's own image and planes
    denoised = load(d, S, "denoised", h, w)
    assert same(denoised, dm.denoise(image, planes["albedo"], planes["normal"], planes["position"])), "denoise()"
    assert pfm_of(os.path.join(d, S, "denoised.pfm"), denoised), "save_denoised_pfm"
    guided, variance = dgm.denoise_guided(image, planes["albedo"], planes["normal"], planes["position"])
    assert same(load(d, S, "guided", h, w), guided), "denoise_guided()"
    assert same(load(d, S, "guided_variance", h, w), variance), "read_denoise_variance()"
    assert not same(guided, denoised) and not same(denoised, image)
    assert same(load(d, S, "image_after", h, w), image)


# ---------------------------------------------------------------------------------------------- 2. temporal, clip, moments, tonemap

@pytest.mark.parametrize("mode", [1, 2])
def test_temporal_sequence_and_display(rt, case, mode):
    w, h, d = case
    H_, S = rt.host, f"temporal_display_{mode}"
    used = log_of(rt, d, S)
    check_log(rt, used, [(1, 1)] * 6, S)
    cameras = [tuple(field(u, k) for k in CAMERA) for u in used]
    assert all(a != b for a, b in zip(cameras, cameras[1:])), "the camera moved before every frame"
    # the traced frames: the log replayed through a context
    ctx = context(rt, d, w, h, H_.AOV_ALBEDO | H_.AOV_NORMAL | H_.AOV_POSITION)
    frames = []
    for k, u in enumerate(used):
        ctx.render(params_of(rt, u))
        got = {name: load(d, S, f"f{k}_{name}", h, w) for name in ("image", "albedo", "normal", "position")}
        assert same(got["image"], ctx.read_image()), f"frame {k}: image"
        for name, bit in (("albedo", H_.AOV_ALBEDO), ("normal", H_.AOV_NORMAL), ("position", H_.AOV_POSITION)):
            assert same(got[name], ctx.read_aov(bit)), f"frame {k}: {name}"
        frames.append(got)
    ctx.close()
    # accumulate, clip and the moments: the mirror over the dumped frames
    sequence = [(f["image"], f["normal"], f["position"], u, f["albedo"]) for f, u in zip(frames, used)]
    steps = tcm.run(sequence, mode=mode, clip_params={})
    for k, (H0, H1, M0, M1) in enumerate(steps):
        assert same(load(d, S, f"f{k}_history", h, w), H0), f"frame {k}: read_temporal() after temporal_accumulate()"
        assert same(load(d, S, f"f{k}_moments", h, w), M0), f"frame {k}: read_temporal_moments() after temporal_accumulate()"
        assert same(load(d, S, f"f{k}_history_clipped", h, w), H1), f"frame {k}: read_temporal() after temporal_clip()"
        assert same(load(d, S, f"f{k}_moments_clipped", h, w), M1), f"frame {k}: read_temporal_moments() after temporal_clip()"
    assert (steps[-1][0][..., 3] > 1).any(), "no pixel found its history"
    last, history, moments = frames[-1], load(d, S, "f5_history_clipped", h, w), load(d, S, "f5_moments_clipped", h, w)
    # denoise_guided over the history with the temporal variance
    guided, variance = mm.denoise_guided_tvar(history, moments, last["albedo"], last["normal"], last["position"], demodulate=(mode == 2))
    got = load(d, S, "guided", h, w)
    assert same(got, guided), "denoise_guided() with denoise_source 1, denoise_variance 1"
    assert same(load(d, S, "guided_variance", h, w), variance)
    assert same(load(d, S, "guided_after_refusal", h, w), got)
    # tonemap of each source
    for name, source in (("image", last["image"]), ("denoised", got), ("temporal", history)):
        assert same(load(d, S, "display_" + name, h, w, np.uint8), tmm.tonemap(source)["display"]), f"tonemap(source = {name})"
    display = load(d, S, "display_temporal", h, w, np.uint8)
    flipped = load(d, S, "display_temporal_flipped", h, w, np.uint8)
    assert same(flipped, display[::-1]) and not same(flipped, display), "read_display(true)"
    assert same(decode_png(os.path.join(d, S, "display_temporal.png")), flipped), "save_display_png"
    # temporal_reset: the next accumulate starts without history
    state = mm.accumulate(None, last["image"], last["normal"], last["position"], used[-1], albedo=last["albedo"], mode=mode)
    assert same(load(d, S, "history_after_reset", h, w), state["H"]) and same(load(d, S, "moments_after_reset", h, w), state["M"])
    assert same(state["H"], tm.accumulate(None, last["image"], last["normal"], last["position"], used[-1])["H"])


# ---------------------------------------------------------------------------------------------- 3. render_until

def test_render_until(rt, oracle, case):
    w, h, d = case
    S = "until"
    used = log_of(rt, d, S)
    first_ret, first_logged, second_ret, logged = (int(v) for v in raw(d, S, "returns", np.int64))
    assert logged == len(used)
    check_log(rt, used, [(k + 1, 0) for k in range(len(used))], S)
    scene, image, est = scene_of(rt, d), np.zeros((h, w, 4), f32), em.Estimator()
    names = em.SUMMARY_INT + em.SUMMARY_FLOAT

    def rounds(at, threshold, max_frames, check_every):
        """the facade's loop over the mirror: (frames, the latest result)"""
        done, res = 0, None
        while done < max_frames:
            for _ in range(min(check_every, max_frames - done)):
                u = used[at + done]
                oracle.render(scene, params_of(rt, u), image, threads=4)
                est.frame(u.frames, u.reset_flag)
                done += 1
            res = est(image, threshold=threshold)
            seen.append((done, res["valid"], res["converged"]))
            if res["valid"] and res["converged"]:
                break
        return done, res

    def check_summary(name, want):
        s, got = summary_dict(rt, open(os.path.join(d, S, name + ".raw"), "rb").read(), rt.host.CErrorSummary, names)
        raw_words = np.frombuffer(bytes(s), f32)
        got.update(scale=raw_words[7], mse=raw_words[8], max_tile_mse=raw_words[9])
        bad = [k for k in em.SUMMARY_INT if int(got[k]) != int(want[k])] + [k for k in em.SUMMARY_FLOAT if words(f32(got[k])) != words(f32(want[k]))]
        assert not bad, f"{name}: {[(k, got[k], want[k]) for k in bad]}"

    seen = []
    done, res = rounds(0, 1.0e-6, 11, 4)
    assert seen == [(4, 0, 0), (8, 1, 0), (11, 1, 0)] and done == 11        # rounds of 4, 4 and 3, none converged
    assert first_ret == 11 and first_logged == 11
    assert same(load(d, S, "image_first", h, w), image), "the image after the first call against the oracle"
    check_summary("summary_first", res)
    assert (res["frames_now"], res["frames_snapshot"]) == (11, 8)
    seen = []
    done, res = rounds(11, 0.5, 6, 2)
    assert second_ret == done and done % 2 == 0 and len(used) == 11 + done, f"render_until returned {second_ret}, the mirror stops after {done}: {seen}"
    assert seen[-1][1:] == (1, 1) and all(s[2] == 0 for s in seen[:-1])      # it stopped because it converged, at the first round that did
    check_summary("summary_second", res)
    assert same(load(d, S, "image", h, w), image), "the final image against the oracle"


# ---------------------------------------------------------------------------------------------- 4. adaptive sampling

def adaptive_expectation(rt, d, w, h, used):
    """the mirror's two sessions over the one-frame images of the logged records: (frames of render_adaptive, its session and
    summary, the hand-driven session, the set mask, its image before the update and its summary)"""
    ones = one_frame_images(rt, d, w, h, used[:-2])
    auto = am.Session(h, w, **ADAPTIVE)
    summary, done = auto.update(), 0
    while not summary["converged"]:
        for _ in range(2):
            auto.frame(ones[done])
            done += 1
        summary = auto.update()
    hand = am.Session(h, w, **ADAPTIVE)
    s = am.shape(h, w)
    hand.set_mask((np.add.outer(np.arange(s["ty"]), np.arange(s["tx"])) % 2).astype(np.uint8))
    set_mask = hand.mask.copy()
    for k in range(3):
        hand.frame(ones[done + k])
    before = hand.image.copy()
    return done, auto, summary, hand, set_mask, before, hand.update()


def test_render_adaptive_and_a_session_by_hand(rt, case):
    w, h, d = case
    S = "adaptive"
    used = log_of(rt, d, S)
    ret, logged = (int(v) for v in raw(d, S, "returns", np.int64))
    assert logged == len(used) == ret + 5
    check_log(rt, used, [(0, 0)] * (ret + 3) + [(1, 0), (2, 0)], S)
    for u in used[:-2]:                                                # the session frames carry what render() marshals, field for field
        for k in SESSION_FIELDS:
            assert field(u, k) == field(used[-2], k), k
    done, auto, summary, hand, set_mask, before, hand_summary = adaptive_expectation(rt, d, w, h, used)
    ty, tx = auto.mask.shape
    assert (ty, tx) == ((h + 15) // 16, (w + 15) // 16)

    def check(prefix, sess, want):
        tiles = raw(d, S, prefix + "tiles", am.TILE_DTYPE)
        assert tiles.size == ty * tx and tiles.tobytes() == np.ascontiguousarray(sess.records).tobytes(), prefix + "read_adaptive_tiles()"
        mask = raw(d, S, prefix + "mask", np.uint8)
        assert mask.size == ty * tx and (mask.reshape(ty, tx) == sess.mask).all(), prefix + "adaptive_get_mask()"
        s = rt.host.CAdaptiveSummary.from_buffer_copy(open(os.path.join(d, S, prefix + "summary.raw"), "rb").read())
        got = {k: int(getattr(s, k)) for k in am.SUMMARY_INT}
        got["max_tile_mse"] = np.frombuffer(bytes(s), f32)[10]
        assert am.same_summary(got, want) == [], f"{prefix}summary: {got}, mirror {want}"
        assert same(load(d, S, prefix + "image", h, w), sess.image), prefix + "image"

    assert ret == done and 2 <= ret <= 6 and ret % 2 == 0
    assert summary["converged"] == 1 and summary["samples_min"] >= 2
    check("", auto, summary)
    got_set = raw(d, S, "hand_mask_set", np.uint8)
    assert got_set.size == ty * tx and (got_set.reshape(ty, tx) == set_mask).all() and 0 < set_mask.sum() < set_mask.size
    assert same(load(d, S, "hand_image_before_update", h, w), before)
    check("hand_", hand, hand_summary)
    assert (hand.n == 3 * set_mask).all()
    # the ordinary frames that end the session: the whole log replayed through a context
    ctx = context(rt, d, w, h)
    ctx.adaptive_begin(**ADAPTIVE)
    ctx.adaptive_set_mask(set_mask)
    for u in used[ret:ret + 3]:
        ctx.adaptive_frame(params_of(rt, u))
    assert same(ctx.read_image(), before)
    for u in used[-2:]:
        ctx.render(params_of(rt, u))
    assert same(load(d, S, "final_image", h, w), ctx.read_image())
    ctx.close()


# ---------------------------------------------------------------------------------------------- 5. robust accumulation

def test_render_robust(rt, case):
    w, h, d = case
    S = "robust"
    used = log_of(rt, d, S)
    first_ret, first_frames, second_ret, second_frames, logged = (int(v) for v in raw(d, S, "returns", np.int64))
    assert (first_ret, first_frames, second_ret, second_frames, logged) == (9, 9, 9, 9, 22) and len(used) == 22
    # two ordinary frames, then robust_frame: frames 0, reset_flag 1 whatever the count; the reset stays pending for run(), which sends the
    # count the sessions left alone
    check_log(rt, used, [(1, 0), (2, 0)] + [(0, 1)] * 18 + [(3, 1), (1, 0)], S)
    for u in used[2:20]:                                               # (m_time has moved on since the first frames: the reset frame carries it)
        for k in SESSION_FIELDS:
            assert field(u, k) == field(used[20], k), k
    assert used[20].time > 0
    ones = one_frame_images(rt, d, w, h, used[2:20])
    a, b = rm.Session(h, w, 4), rm.Session(h, w, 4)
    for k in range(9):
        a.accumulate(ones[k])
        b.accumulate(ones[9 + k])
    for j in range(4):
        assert same(load(d, S, f"bucket{j}", h, w), a.planes[j]), f"read_robust_bucket({j})"
        assert same(load(d, S, f"second_bucket{j}", h, w), b.planes[j]), f"read_robust_bucket({j}) of the second session"
    assert same(load(d, S, "robust", h, w), a.resolve(2.0)), "read_robust()"
    assert not same(a.resolve(2.0), a.resolve(0.0)), "gain 2 trims nothing here: the gain is not seen"
    assert same(load(d, S, "image_first", h, w), ones[8]), "a resolve into the buffer leaves the image at the last frame"
    assert same(load(d, S, "image_second", h, w), b.resolve(2.0, rm.DEST_IMAGE)), "to_image: read_image()"
    ctx = context(rt, d, w, h)
    ctx.write_image(b.resolve(2.0, rm.DEST_IMAGE))
    for u in used[20:]:
        ctx.render(params_of(rt, u))
    assert same(load(d, S, "final_image", h, w), ctx.read_image())
    ctx.close()


# ---------------------------------------------------------------------------------------------- 6. a window closed while rendering

def test_a_quit_cuts_every_loop_short_and_is_counted(rt, oracle, case):
    """SDL_QUIT polled in the second frame of render_until's second round (Window::run() still renders that frame), and SDL_QUIT
    waiting before the first: each loop returns the frames it rendered, which is the length of the log"""
    w, h, d = case
    S = "quit"
    scene = scene_of(rt, d)
    blob = open(os.path.join(d, S, "params_waiting.raw"), "rb").read()
    n = ctypes.sizeof(rt.host.CFrameParams)
    for name, used, want in (("", log_of(rt, d, S), 6), ("_waiting", [rt.host.CFrameParams.from_buffer_copy(blob[i:i + n]) for i in range(0, len(blob), n)], 1)):
        values = [int(v) for v in raw(d, S, "returns" + name, np.int64)]
        assert values[:2] == [want, want] and len(used) == want, f"render_until returned {values[0]} after {values[1]} logged frames"
        assert values[2:] == [0] * (len(values) - 2), "a loop rendered although the window was closed"
        check_log(rt, used, [(k + 1, 0) for k in range(want)], S + name)
        image, est, res = np.zeros((h, w, 4), f32), em.Estimator(), None
        for k, u in enumerate(used):
            oracle.render(scene, params_of(rt, u), image, threads=4)
            est.frame(u.frames, u.reset_flag)
            if k + 1 in (4, want):
                res = est(image, threshold=1.0e-6)
        assert same(load(d, S, "image" + name, h, w), image)
        if not name:                                                   # the estimate after the short round: frames 4 against 6
            s = rt.host.CErrorSummary.from_buffer_copy(open(os.path.join(d, S, "summary.raw"), "rb").read())
            got = np.frombuffer(bytes(s), f32)
            assert (s.valid, s.converged, s.frames_now, s.frames_snapshot) == (1, 0, 6, 4) == (res["valid"], res["converged"], res["frames_now"], res["frames_snapshot"])
            assert [words(got[i]) for i in (7, 8, 9)] == [words(f32(res[k])) for k in em.SUMMARY_FLOAT]


# ---------------------------------------------------------------------------------------------- 7. before the prerequisite call

def test_nothing_yet_still_renders(rt, case):
    """the refusals are the driver's own checks (its exit code); what is left to see is that none of them rendered or was logged, and
    that only the two refused adaptive_frame()s, which marshal their uniforms before the library refuses, drew from rand()"""
    w, h, d = case
    used = log_of(rt, d, "nothing_yet")
    check_log(rt, used, [(1, 0)], "nothing_yet", refused_before=2)
    ctx = context(rt, d, w, h)
    ctx.render(params_of(rt, used[0]))
    assert same(load(d, "nothing_yet", "image", h, w), ctx.read_image())
    ctx.close()
    assert not [f for f in os.listdir(os.path.join(d, "nothing_yet")) if f.endswith((".pfm", ".png"))]


# ---------------------------------------------------------------------------------------------- 8. the Python twin

def test_the_headless_renderer_is_the_facades_twin(rt, case):
    """host.HeadlessRenderer through the call sequences of the adaptive and robust scenarios: the same (frames, reset_flag, random) for
    every frame of any kind and the same pictures as the C++ program -- a session frame draws one word, does not advance the frame count
    and leaves a pending reset for the next ordinary frame"""
    w, h, d = case
    H_ = rt.host

    class Logging(H_.HeadlessRenderer):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.log = []

        def next_frame(self):
            self.log.append(super().next_frame())
            return self.log[-1]

        def session_frame(self, reset_flag=0):
            self.log.append(super().session_frame(reset_flag))
            return self.log[-1]

    def twin():
        r = Logging(w, h)
        r.set_scene(scene_of(rt, d))
        r.params = rt.scenes.FrameParams(max_bounce=BOUNCES)
        return r

    key = lambda entries: [(p.frames, p.reset_flag, p.random) for p in entries]
    # adaptive
    used = log_of(rt, d, "adaptive")
    r = twin()
    frames, summary = r.render_adaptive(ADAPTIVE["threshold"], ADAPTIVE["max_samples"], min_samples=ADAPTIVE["min_samples"], check_every=2)
    assert frames == int(raw(d, "adaptive", "returns", np.int64)[0]) and summary["converged"] == 1
    assert same(r.ctx.read_image(), load(d, "adaptive", "image", h, w))
    assert (r.m_frames, r.m_reset) == (0, False)
    r.ctx.adaptive_begin(**ADAPTIVE)
    s = am.shape(h, w)
    r.ctx.adaptive_set_mask((np.add.outer(np.arange(s["ty"]), np.arange(s["tx"])) % 2).astype(np.uint8))
    for _ in range(3):
        r.ctx.adaptive_frame(r.session_frame())
    r.ctx.adaptive_update()
    assert same(r.ctx.read_image(), load(d, "adaptive", "hand_image", h, w))
    r.run(2)
    assert key(r.log) == key(used)
    assert same(r.ctx.read_image(), load(d, "adaptive", "final_image", h, w))
    r.ctx.close()
    # robust
    used = log_of(rt, d, "robust")
    r = twin()
    r.run(2)
    assert same(r.render_robust(9, buckets=4, gain=2.0), load(d, "robust", "robust", h, w))
    assert (r.m_frames, r.m_reset) == (2, False) and r.ctx.robust_frames() == (9, 4)
    r.reset_buffer()
    assert same(r.render_robust(9, buckets=4, gain=2.0, to_image=True), load(d, "robust", "image_second", h, w))
    assert (r.m_frames, r.m_reset) == (2, True)
    r.run(2)
    assert key(r.log) == key(used)
    assert same(r.ctx.read_image(), load(d, "robust", "final_image", h, w))
    r.ctx.close()
