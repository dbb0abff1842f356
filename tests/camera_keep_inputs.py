"""Inputs for the kept bits of the camera-ray bounce (raytracer.glsl_amd/csrc/rt_camera_keep.hpp; rtgl_amd.hip, d_keep0): named and seeded
cameras, a Python restatement of the decision and of the host rules around it, and seeded lives of one context.  numpy only, no GPU.

    cameras()            -> [Camera(name, family, fields)]    fields: the camera fields of FrameParams (use_dof included)
    camera_words(p)      -> 16 uint32 words laid out like rt_camera_keep::Camera
    widening(words)      -> (ok, ro_add, sigma_add)           widening() restated in float32
    decide(key, frame)   -> (cached, have_bits, ro_add, sigma_add);  lean(decision, opt_camera_lean, aov)
    trace(seq) / model(seq) -> per rendered frame what the context decides: model() gives [reuses_bits], trace() the records
    sequence(seed)       -> Sequence(W, H, scene, options, steps): one context's life, 10..16 frames
    replay(seq)          -> [(scene as it stands, FrameParams, image written before the frame | None)] for every rendered frame

Camera families (FAMILIES)
  tame     |pos| <= 50, focal 5..60, aperture / focal in [1e-4, 0.2] (log-uniform), the reference's basis or a rotated orthonormal one
  limit    aperture / focal just below 0.25 (0.2499), at 0.25 and above it; negative aperture, negative focal, both negative
  far      the five cameras at which the bound of the first camera_lean version was too small, by name, and drawn ones: |pos| 1e2..1e6,
           aperture 0.2..20 ulps of |pos|, focal from 4.1 apertures to 100
  tiny     focal down to 1e-3 with aperture < focal / 4
  skew     forward, right and up neither unit length nor orthogonal (the shader normalises the direction either way); one with a zero
           forward vector, whose centre pixel has no direction at all (0 / 0) at even sizes
  no_dof   use_dof = 0 with any aperture (huge, NaN, above the focal length)
Four fov values and fields that are -0.0 occur across the families.

The decision model restates rtgl_amd.hip as far as the kept bits go:
  * a frame takes a decision only on kernel 4 with triangle visits and max_bounce > 0; other frames leave the key alone;
  * culled: option cull >= 1; single: one frame (no batch of two) of one sample; a frame that is not both is not cached and leaves the key alone;
  * a cached frame without usable bits drops the key and, because bounce 0 is culled, packet_cull_kernel is enqueued for it: the key is
    valid again with this frame's n0, words, scene_version and camera;
  * scene_version counts rebuilds of the triangles: the first frame after upload_vertices, upload_meshes or a changed mf_group_quads;
  * words = max(1, ceil(quads * 4 / 32)) with quads = ceil(visits / 40); the buffer only grows (room);
  * the lean bounce: a frame that reuses bits with camera_lean on and without first-hit planes;
  * a frame refused by the host's argument check (a node buffer over the visit cap: before the triangles are rebuilt and before anything
    is enqueued) changes nothing; a frame that fails later drops the key (Key.valid = 0 in decide(): tests/test_camera_keep_inputs.py).
Batching (option frame_batch): a frame is held back while the batch is not full and nothing else is asked of the context; every other
call submits what is held back.  Read-outs (counters, RNG states) and first-hit planes switch batching off.

Sequences: W in 40..136, H in 24..88 (most no multiple of 8), 50..1500 triangles placed relative to the camera with
mesh_fuzz_inputs._vertices(extras=True), optional spheres and cube map, max_bounce 1..4.  EVENT_KINDS lists what happens between frames;
sequence(s) holds the kinds EVENT_KINDS[(5 s + i) mod n], i < 5, and random further ones, so the twelve default seeds cover every kind twice.
SKIPPED_SEEDS: seeds whose oracle images hold a NaN, with the reason; default_seeds() leaves them out (at most 2).
"""
from collections import namedtuple

import numpy as np

import mesh_fuzz_inputs as mf
import scene_fuzz_inputs as sf

sc = sf.sc
FAMILIES = ("tame", "limit", "far", "tiny", "skew", "no_dof")
Camera = namedtuple("Camera", "name family fields")
F32 = np.float32
FOVS = (0.3, float(sc.radians_f32(33.0)), 1.2, 2.2)
DEFAULT_SEQUENCES = 12
SKIPPED_SEEDS = ()                                     # (seed, reason) pairs, measured on the CPU oracle (tests/test_camera_keep_inputs.py): none

# the rows of the table in DESIGN.md (camera keep): position, aperture, focal, largest |d_k - d_1| the CPU oracle gave over 12 frames
FAR_NAMED = (("far_1e4_x", (1.0e4, 50.0, -30.0), 0.01, 2.0, 0.010291),
             ("far_3e4_x", (3.0e4, 0.0, -30.0), 0.005, 1.0, 0.011717),
             ("far_1e4_diagonal", (1.0e4, 1.0e4, 1.0e4), 0.004, 0.5, 0.017818),
             ("far_300_tiny_focal", (300.0, 20.0, -30.0), 0.0002, 0.01, 0.041532),
             ("far_5e5_x", (5.0e5, 0.0, -30.0), 0.05, 0.3, 0.4299))


def default_seeds(n=DEFAULT_SEQUENCES, start=0):
    out, s, skipped = [], start, {seed for seed, _ in SKIPPED_SEEDS}
    while len(out) < n:
        if s not in skipped:
            out.append(s)
        s += 1
    return out


# ------------------------------------------------------------------------------------------------ cameras

def _f32t(v):
    return tuple(float(x) for x in np.asarray(v, F32))


def _basis(rng, style):
    """forward, up, right: 0 the reference's, 1 rotated orthonormal, 2 rotated, non-unit and skewed"""
    fwd, up, right = np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0]), np.array([-1.0, 0.0, 0.0])
    if style:
        yaw, pitch, roll = rng.uniform(-3.0, 3.0), rng.uniform(-1.2, 1.2), rng.uniform(-0.6, 0.6)
        fwd = np.array([np.sin(yaw) * np.cos(pitch), np.sin(pitch), np.cos(yaw) * np.cos(pitch)])
        r0 = sf._unit(np.array([-np.cos(yaw), 0.0, np.sin(yaw)]))
        u0 = np.cross(r0, fwd)
        right, up = np.cos(roll) * r0 + np.sin(roll) * u0, np.cos(roll) * u0 - np.sin(roll) * r0
    if style == 2:
        s = rng.uniform(0.3, 2.5, 3)
        fwd, up, right = s[0] * fwd + 0.2 * up, s[1] * up + 0.15 * right, s[2] * right - 0.1 * fwd
    return fwd, up, right


def _fields(pos, aperture, focal, fov=FOVS[1], basis=None, use_dof=1):
    fwd, up, right = basis if basis is not None else _basis(None, 0)
    return dict(camera_position=_f32t(pos), camera_forward=_f32t(fwd), camera_up=_f32t(up), camera_right=_f32t(right), camera_fov=float(F32(fov)),
                camera_aperture=float(F32(aperture)), camera_focal_length=float(F32(focal)), use_dof=int(use_dof))


def cameras():
    out = []
    rng = np.random.default_rng([20262, 1])
    for i in range(8):                                     # tame
        pos = sf._unit(rng.normal(size=3)) * rng.uniform(0.0, 50.0)
        if i == 1:
            pos = np.array([-0.0, 0.0, -30.0])
        focal = rng.uniform(5.0, 60.0)
        ratio = 10.0 ** rng.uniform(-4.0, np.log10(0.2))
        out.append(Camera(f"tame_{i}", "tame", _fields(pos, ratio * focal, focal, FOVS[i % 4], _basis(rng, i % 2))))
    out.append(Camera("tame_c5", "tame", _fields((0.0, 0.0, -30.0), 0.5, 38.0)))
    out.append(Camera("tame_ratio_0.2", "tame", _fields((3.0, -2.0, -30.0), 2.0, 10.0, FOVS[2])))
    at = (0.0, 0.0, -30.0)                                 # limit
    for name, a, f in (("limit_0.2499", 2.499, 10.0), ("limit_0.25", 2.5, 10.0), ("limit_above", 2.6, 10.0), ("limit_0.24", 2.4, 10.0),
                       ("limit_neg_aperture", -2.499, 10.0), ("limit_neg_focal", 2.4, -10.0), ("limit_both_neg", -2.4, -10.0),
                       ("limit_0.2499_of_38", 0.2499 * 38.0, 38.0), ("limit_neg_aperture_above", -2.5, 10.0)):
        out.append(Camera(name, "limit", _fields(at, a, f, FOVS[len(out) % 4])))
    for name, pos, a, f, _ in FAR_NAMED:                   # far
        out.append(Camera(name, "far", _fields(pos, a, f)))
    for i in range(10):
        pn = 10.0 ** rng.uniform(2.0, 6.0)
        pos = sf._unit(rng.normal(size=3)) * pn
        a = float(np.spacing(F32(pn))) * 10.0 ** rng.uniform(np.log10(0.2), np.log10(20.0))
        focal = 10.0 ** rng.uniform(np.log10(4.1 * a), 2.0)
        out.append(Camera(f"far_drawn_{i}", "far", _fields(pos, a if i % 3 else -a, focal, FOVS[i % 4], _basis(rng, i % 2))))
    for i, (f, ratio) in enumerate(((1.0e-3, 0.2), (1.0e-3, 0.01), (3.0e-3, 0.24), (0.01, 0.1), (0.05, 0.2499), (0.2, 1.0e-3))):      # tiny
        pos = (0.0, -0.0, -30.0) if i % 2 else sf._unit(rng.normal(size=3)) * rng.uniform(1.0, 50.0)
        out.append(Camera(f"tiny_{i}", "tiny", _fields(pos, ratio * f, f, FOVS[i % 4], _basis(rng, i % 2))))
    for i in range(5):                                     # skew
        pos = sf._unit(rng.normal(size=3)) * rng.uniform(0.0, 50.0)
        out.append(Camera(f"skew_{i}", "skew", _fields(pos, (0.001, 0.5, 2.0)[i % 3], 10.0 + 7.0 * i, FOVS[i % 4], _basis(rng, 2))))
    out.append(Camera("skew_zero_forward", "skew", _fields(at, 0.5, 38.0, FOVS[1], (np.zeros(3), np.array([0.0, 1.5, 0.1]), np.array([-0.7, 0.2, 0.0])))))
    for i, a in enumerate((0.0, 0.5, 100.0, float("nan"), -1.0e30)):                     # no_dof
        pos = (0.0, 0.0, -30.0) if i % 2 else (1.0e4, 50.0, -30.0)
        out.append(Camera(f"no_dof_{i}", "no_dof", _fields(pos, a, (10.0, 1.0)[i % 2], FOVS[i % 4], _basis(rng, i % 3), use_dof=0)))
    assert len({c.name for c in out}) == len(out)
    return out


def camera_named(name):
    return next(c for c in cameras() if c.name == name)


def camera_words(p):
    """the 16 words of rt_camera_keep::Camera for FrameParams-like `p` (or a dict of its camera fields)"""
    g = p.get if isinstance(p, dict) else lambda k: getattr(p, k)
    w = np.zeros(16, np.uint32)
    w[0] = np.uint32(int(g("use_dof")) & 0xFFFFFFFF)
    w[1:].view(F32)[:] = [g("camera_fov"), g("camera_aperture"), g("camera_focal_length"), *g("camera_position"), *g("camera_forward"), *g("camera_up"), *g("camera_right")]
    return w


# ------------------------------------------------------------------------------------------------ the decision, restated

def widening(words):
    """rt_camera_keep::widening in float32, operation by operation"""
    f32 = np.asarray(words, np.uint32).view(F32)
    zero = F32(0.0)
    if int(np.asarray(words, np.uint32)[0]) == 0:
        return True, zero, zero
    with np.errstate(all="ignore"):
        a, f = np.abs(f32[2]), np.abs(f32[3])
        x, y, z = f32[4], f32[5], f32[6]
        pn = np.sqrt(F32(F32(x * x + y * y) + z * z))
        if not a < F32(0.25) * f or not f < F32(1.0e18) or not pn < F32(1.0e18):
            return False, zero, zero
        r = F32(4.76837158203125e-7) * F32(pn + f)
        if not F32(f - a) >= F32(4.0) * r:
            return False, zero, zero
        two_a = F32(F32(2.0) * a) * F32(1.001)
        ro = F32(two_a + F32(F32(1.0e-5) * F32(F32(1.0) + pn)))
        sigma = F32(F32(F32(two_a + r) / F32(F32(f - a) - r)) + F32(4.0e-6))
    return True, ro, sigma


Key = namedtuple("Key", "valid n0 words scene camera")                         # camera: the 16 words as bytes
Frame = namedtuple("Frame", "culled single enabled room n0 words scene camera")
Decision = namedtuple("Decision", "cached have_bits ro_add sigma_add")


def same_camera(a, b):
    """field for field as the header compares them: fov, aperture and focal by value (NaN differs from itself), the vectors by their bytes
    (-0.0 is not 0.0)"""
    wa, wb = np.frombuffer(a, np.uint32), np.frombuffer(b, np.uint32)
    fa, fb = wa.view(F32), wb.view(F32)
    return bool(wa[0] == wb[0] and fa[1] == fb[1] and fa[2] == fb[2] and fa[3] == fb[3] and a[16:] == b[16:])


def decide(key, frame):
    zero = F32(0.0)
    if not (frame.culled and frame.single and frame.enabled):
        return Decision(False, False, zero, zero)
    ok, ro, sigma = widening(np.frombuffer(frame.camera, np.uint32))
    if not ok:
        return Decision(False, False, zero, zero)
    have = bool(key.valid and frame.room and key.n0 == frame.n0 and key.words == frame.words and key.scene == frame.scene and same_camera(key.camera, frame.camera))
    return Decision(True, have, ro, sigma)


def lean(d, opt_camera_lean, aov):
    return bool(d.cached and d.have_bits and opt_camera_lean != 0 and not aov)


def keep_words(visits):
    quads = -(-visits // 40)
    return max(1, (quads * 4 + 31) // 32)


# ------------------------------------------------------------------------------------------------ one context's life

# a step: `pre` actions, then one frame (refused: the frame is expected to fail the argument check and renders nothing), then, where
# `check`, a read-out.  sync False: the frame is submitted without waiting, so a batching context may hold it back.
Step = namedtuple("Step", "pre params sync check refused kinds")
Sequence = namedtuple("Sequence", "W H scene options steps camera")
# actions: ("option", key, value) | ("upload", what, array) | ("write_image", array)
Record = namedtuple("Record", "step decided key frame decision lean batched")    # what the context decides for one rendered frame

EVENT_KINDS = ("up_materials", "up_spheres", "up_nodes", "up_envmap", "up_vertices", "up_meshes", "write_image", "reset_flag", "samples2",
               "move_ab", "move_aba", "neg_zero", "dof_toggle", "aperture_wide_and_back", "camera_lean", "cull", "scan_waves", "scan_dynamic",
               "narrow_fused", "mf_chunk_quads", "mf_group_quads", "sort_min_rays", "aov", "kernel2", "batch2", "unsynced_pair", "refused")
OPTION_DEFAULTS = dict(kernel=4, cull=3, camera_lean=1, frame_batch=1, aov=0, counters=0, rng_state=0, mf_group_quads=32)


def footprint(W, H):
    return (W // 8 * 8) * (H // 8 * 8)


def trace(seq, n0=None, options=()):
    """[Record] for every rendered frame of `seq`, in order.  n0: the ray slots of one frame (default: the 8 x 8-aligned footprint).
    options: a control run -- set after the sequence's own and pinned: the sequence's later changes of these options are left out."""
    n0 = footprint(seq.W, seq.H) if n0 is None else n0
    opt = dict(OPTION_DEFAULTS)
    st = dict(kernel_explicit=False, group_explicit=False, tris_dirty=True, version=0, visits=0, group_quads=32, capacity=0,
              meshes=seq.scene.meshes, vertices=seq.scene.vertices)
    key = Key(False, 0, 0, 0, bytes(64))
    pending, out = [], []

    def set_option(k, v):
        flush()
        if k == "kernel":
            st["kernel_explicit"] = True
        if k == "mf_group_quads":
            if v != st["group_quads"]:
                st["tris_dirty"] = True
            st["group_explicit"] = True
        opt[k] = v

    def render_batch(batch):
        nonlocal key
        if st["tris_dirty"]:
            st["visits"] = mf.count(st["meshes"], st["vertices"].shape[0] // 3)
            st["version"] += 1
            if st["visits"]:
                st["group_quads"] = opt["mf_group_quads"] if st["group_explicit"] else 32
            st["tris_dirty"] = False
        p0 = batch[0][1]
        kernel = 0 if st["visits"] == 0 and not st["kernel_explicit"] else opt["kernel"]
        wavefront = kernel != 0 and p0.max_bounce > 0
        if len(batch) > 1 and not (wavefront and n0 > 0):
            for b in batch:
                render_batch([b])
            return
        B = len(batch)
        if not (wavefront and n0 > 0 and kernel == 4 and st["visits"] > 0):
            out.extend(Record(i, False, key, None, Decision(False, False, F32(0), F32(0)), False, B > 1) for i, _ in batch)
            return
        words = keep_words(st["visits"])
        need = (n0 * B // 128 + 16) * words
        fr = Frame(opt["cull"] >= 1, B == 1 and p0.samples == 1, True, st["capacity"] >= need, n0 * B, words, st["version"], camera_words(p0).tobytes())
        d = decide(key, fr)
        before = key
        if d.cached:
            st["capacity"] = max(st["capacity"], need)
            if not d.have_bits:                            # bounce 0 is culled: packet_cull_kernel runs and the bits are this frame's
                key = Key(True, fr.n0, fr.words, fr.scene, fr.camera)
        is_lean = lean(d, opt["camera_lean"], opt["aov"] != 0)
        out.extend(Record(i, True, before, fr, d, is_lean, B > 1) for i, _ in batch)

    def flush():
        nonlocal pending
        if pending:
            batch, pending = pending, []
            render_batch(batch)

    def compatible(a, b):
        return a.samples == b.samples and a.max_bounce == b.max_bounce and a.use_envmap == b.use_envmap and tuple(a.background) == tuple(b.background)

    for k, v in seq.options:
        set_option(k, v)
    for k, v in options:
        set_option(k, v)
    pinned = {k for k, _ in options}
    for i, s in enumerate(seq.steps):
        for act in s.pre:
            flush()
            if act[0] == "option" and act[1] not in pinned:
                set_option(act[1], act[2])
            elif act[0] == "upload":
                if act[1] in ("meshes", "vertices"):
                    st[act[1]] = act[2]
                    st["tris_dirty"] = True
        if s.refused:
            assert not pending and opt["frame_batch"] == 1
            continue                                       # refused before the triangles are rebuilt: nothing changes
        p = s.params
        batchable = (opt["frame_batch"] > 1 and p.samples == 1 and p.max_bounce > 0 and not opt["counters"] and not opt["rng_state"] and not opt["aov"]
                     and (st["visits"] > 0 or st["tris_dirty"] or st["kernel_explicit"]) and opt["kernel"] != 0)
        if pending and (not batchable or not compatible(pending[0][1], p)):
            flush()
        if batchable:
            pending.append((i, p))
            if len(pending) >= opt["frame_batch"]:
                flush()
        else:
            render_batch([(i, p)])
        if s.sync or s.check:
            flush()
    flush()
    assert [r.step for r in out] == [i for i, s in enumerate(seq.steps) if not s.refused]
    return out


def model(seq, **kw):
    """[reuses_bits] per rendered frame"""
    return [r.decision.have_bits for r in trace(seq, **kw)]


def lean_counts(seq, **kw):
    """step index -> camera_lean_frames after that step's frame has been submitted"""
    n, out = 0, {}
    for r in trace(seq, **kw):
        n += int(r.lean)
        out[r.step] = n
    return out


# ------------------------------------------------------------------------------------------------ sequences

REFUSED_SPHERES = 17


def refused_uploads():
    """(spheres, nodes) of the two-node cycle over 17 spheres: 65535 pops x 17 sphere tests > 2^20, refused by the host before any launch"""
    spheres = sc.make_spheres([(-16.0 + 2.0 * i, -4.0 + (i % 3), 0.0, 1.0, i % 8) for i in range(REFUSED_SPHERES)])
    box = ((-1e5,) * 3, (1e5,) * 3)
    nodes = sc.make_nodes([box + (1, sf.INVALID, 0, REFUSED_SPHERES), box + (0, sf.INVALID, 0, REFUSED_SPHERES)])
    assert sf.walk(nodes).visits > 1 << 20
    return spheres, nodes


def view_axes(fields):
    """position and the unit view axes the geometry is placed by (a negative focal length with depth of field looks backwards)"""
    pos = np.array(fields["camera_position"], np.float64)
    fwd, up, right = (np.array(fields[k], np.float64) for k in ("camera_forward", "camera_up", "camera_right"))
    fwd = sf._unit(fwd) if fwd.any() else np.array([0.0, 0.0, 1.0])
    if fields["use_dof"] and fields["camera_focal_length"] < 0:
        fwd = -fwd
    right = right - fwd * (right @ fwd)
    right = sf._unit(right) if right.any() else sf._unit(np.cross(fwd, [0.3, 1.0, 0.2]))
    return pos, fwd, right, sf._unit(np.cross(fwd, right))


def scene_around(rng, fields, n_tris, spheres=True, env=True):
    pos, fwd, right, up = view_axes(fields)
    mats = mf._materials(rng)
    if spheres:
        sp = sf._spheres(rng, mats, pos, fwd, right, up)
        nodes = sf._bounded_nodes(rng, sp.shape[0], False)
    else:
        sp, nodes = np.zeros((0, 8), np.float32), np.zeros((0, 12), np.float32)
    scene = sc.Scene(spheres=sp, materials=mats, nodes=nodes, env=sc.noise_cubemap(int(rng.choice([2, 8])), 4, seed=int(rng.integers(1, 1000))) if env else None)
    scene.vertices = mf._vertices(rng, n_tris, mats.shape[0], pos, fwd, right, up, extras=True)
    scene.meshes = _meshes(rng, n_tris)
    return scene


def _meshes(rng, n):
    if n > 1 and rng.random() < 0.4:
        k = int(rng.integers(1, n))
        return mf.make_meshes([(0, k), (k, n - k)])
    return mf.make_meshes([(0, n)])


SEQUENCE_CAMERAS = ("tame_0", "tame_c5", "far_1e4_x", "limit_0.2499", "tame_3", "far_300_tiny_focal", "limit_neg_focal", "tiny_3", "far_1e4_diagonal",
                    "skew_1", "tame_ratio_0.2", "far_3e4_x")


def sequence(seed):
    seed = int(seed)
    rng = np.random.default_rng([seed, 13, 20262])
    W, H = int(rng.integers(40, 137)), int(rng.integers(24, 89))
    cam = camera_named(SEQUENCE_CAMERAS[seed % len(SEQUENCE_CAMERAS)])
    A = dict(cam.fields)
    pos, fwd, right, up = view_axes(A)
    n_tris = int(rng.integers(50, 1501) if rng.random() < 0.3 else rng.integers(50, 500))
    scene = scene_around(rng, A, n_tris, spheres=rng.random() < 0.6, env=rng.random() < 0.6)
    n_mat = scene.materials.shape[0]
    options = (("kernel", 4), ("scan_waves", int(rng.integers(0, 3))), ("scan_dynamic", int(rng.integers(0, 5))), ("cull", int(rng.choice([1, 2, 3, 3]))),
               ("sort_min_rays", int(rng.choice([0, 65536]))), ("mf_chunk_quads", int(rng.choice(mf.CHUNK_QUADS))), ("rng_state", 1), ("counters", 1))
    base = sc.FrameParams(max_bounce=int(rng.integers(1, 5)), samples=1, use_envmap=int(rng.random() < 0.7),
                          background=tuple(float(F32(x)) for x in rng.uniform(0.0, 1.5, 3)), **A)
    B = dict(A, camera_position=_f32t(pos + right * rng.uniform(0.5, 3.0) + up * rng.uniform(-1.0, 1.0)))
    n_frames = int(rng.integers(10, 17))
    n_kinds = len(EVENT_KINDS)
    todo = [EVENT_KINDS[(5 * seed + i) % n_kinds] for i in range(5)]
    g = sc.GlibcRand(seed + 2000)
    state = dict(cam=dict(A), opts=dict(options), m_frames=0)
    steps, restore = [], []                                # restore: actions and camera changes that undo a one-frame event, for the next step

    def frame(pre, kinds, sync=True, check=True, refused=False, **kw):
        state["m_frames"] += 1
        p = base.replace(frames=state["m_frames"], random=g.rand(), **dict(state["cam"], **kw))
        steps.append(Step(tuple(pre), p, sync, check, refused, tuple(kinds)))
        if p.reset_flag:
            state["m_frames"] = 0

    def flip(key, choices):
        v = int(rng.choice([c for c in choices if c != state["opts"].get(key, OPTION_DEFAULTS.get(key))]))
        state["opts"][key] = v
        return ("option", key, v)

    need = dict(move_ab=2, move_aba=3, dof_toggle=2, aperture_wide_and_back=3, cull=3, aov=2, batch2=2, unsynced_pair=2, refused=0)
    n_frames = min(16, max(n_frames, 2 + sum(need.get(k, 1) for k in todo)))
    while sum(not s.refused for s in steps) < n_frames - 2:
        pre, restore = list(restore), []
        left = n_frames - 2 - sum(not s.refused for s in steps)
        owed = sum(need.get(k, 1) for k in todo)
        kind = None
        if todo and (rng.random() < 0.5 or left <= owed):
            kind = todo.pop(0)
        elif rng.random() < 0.55:
            kind = str(rng.choice(EVENT_KINDS))
            if need.get(kind, 1) > left - owed:
                kind = None
        if kind is None:
            frame(pre, ())
        elif kind == "up_materials":
            m = scene.materials.copy()
            m[:, 0:3] *= F32(rng.choice([1.0, 0.8]))
            frame(pre + [("upload", "materials", m)], (kind,))
        elif kind == "up_spheres":
            sp = scene.spheres.copy()
            if sp.size:
                sp[:, 3] *= F32(0.9)
            frame(pre + [("upload", "spheres", sp)], (kind,))
        elif kind == "up_nodes":
            frame(pre + [("upload", "nodes", sc.single_leaf(scene.spheres.shape[0]) if scene.spheres.shape[0] else scene.nodes)], (kind,))
        elif kind == "up_envmap":
            frame(pre + [("upload", "envmap", sc.noise_cubemap(int(rng.choice([1, 3, 8])), int(rng.choice([3, 4])), seed=int(rng.integers(1, 1000))))], (kind,))
        elif kind == "up_vertices":
            n = scene.vertices.shape[0] // 3 if rng.random() < 0.5 else int(rng.integers(50, 500))
            frame(pre + [("upload", "vertices", mf._vertices(rng, n, n_mat, pos, fwd, right, up, extras=True))], (kind,))
        elif kind == "up_meshes":
            frame(pre + [("upload", "meshes", _meshes(rng, int(rng.integers(40, 500))))], (kind,))
        elif kind == "write_image":
            img = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
            frame(pre + [("write_image", img)], (kind,))
        elif kind == "reset_flag":
            frame(pre, (kind,), reset_flag=1)
        elif kind == "samples2":
            frame(pre, (kind,), samples=2)
        elif kind in ("move_ab", "move_aba"):
            state["cam"] = dict(B) if state["cam"]["camera_position"] == A["camera_position"] else dict(A)
            frame(pre, (kind,))
            frame([], ())
            if kind == "move_aba":
                state["cam"] = dict(B) if state["cam"]["camera_position"] == A["camera_position"] else dict(A)
                frame([], ())
        elif kind == "neg_zero":                           # 0.0 -> -0.0 in one field: another camera byte for byte, the same rays
            fields = [k for k in ("camera_up", "camera_right", "camera_forward", "camera_position") if 0.0 in state["cam"][k]]
            field = str(rng.choice(fields)) if fields else "camera_up"
            v = list(state["cam"][field])
            zeros = [j for j, x in enumerate(v) if x == 0.0]
            if zeros:
                j = zeros[int(rng.integers(len(zeros)))]
                v[j] = -v[j] if np.signbit(v[j]) else -0.0
                state["cam"][field] = tuple(v)
                frame(pre, (kind,))
            else:
                frame(pre, ())
        elif kind == "dof_toggle":
            state["cam"]["use_dof"] = 1 - state["cam"]["use_dof"]
            frame(pre, (kind,))
            frame([], ())
        elif kind == "aperture_wide_and_back":
            keep = state["cam"]["camera_aperture"]
            state["cam"]["camera_aperture"] = float(F32(abs(state["cam"]["camera_focal_length"]) * rng.choice([0.25, 0.3, 1.5])))
            frame(pre, (kind,))
            frame([], ())
            state["cam"]["camera_aperture"] = keep
            frame([], ())
        elif kind in ("camera_lean", "narrow_fused"):
            frame(pre + [flip(kind, (0, 1))], (kind,))
        elif kind == "cull":
            frame(pre + [flip("cull", (0, 1, 2, 3))], (kind,))
            if state["opts"]["cull"] == 0:
                frame([], ())
                frame([flip("cull", (1, 3))], ("cull",))
        elif kind == "scan_waves":
            frame(pre + [flip(kind, (0, 1, 2))], (kind,))
        elif kind == "scan_dynamic":
            frame(pre + [flip(kind, (0, 1, 2, 3, 4))], (kind,))
        elif kind == "mf_chunk_quads":
            frame(pre + [flip(kind, mf.CHUNK_QUADS)], (kind,))
        elif kind == "mf_group_quads":
            frame(pre + [flip(kind, mf.GROUP_QUADS)], (kind,))
        elif kind == "sort_min_rays":
            frame(pre + [flip(kind, (0, 65536))], (kind,))
        elif kind == "aov":
            frame(pre + [("option", "aov", 15)], (kind,))
            frame([], ())
            restore = [("option", "aov", 0)]
        elif kind == "kernel2":
            frame(pre + [("option", "kernel", 2)], (kind,))
            restore = [("option", "kernel", 4)]
        elif kind == "batch2":                             # a pair in one set of launches: no read-outs while it lasts
            frame(pre + [("option", "rng_state", 0), ("option", "counters", 0), ("option", "frame_batch", 2)], (kind,), sync=False, check=False)
            frame([], (), sync=False, check=True)
            restore = [("option", "frame_batch", 1), ("option", "rng_state", 1), ("option", "counters", 1)]
        elif kind == "unsynced_pair":
            frame(pre, (kind,), sync=False, check=False)
            frame([], (), sync=False, check=True)
        elif kind == "refused":
            sp, cycle = refused_uploads()
            frame(pre + [("upload", "spheres", sp), ("upload", "nodes", cycle)], (kind,), refused=True)
            state["m_frames"] -= 1                         # the application's frame did not happen
            sane = scene.spheres if scene.spheres.shape[0] else sp
            restore = [("upload", "spheres", sane), ("upload", "nodes", sc.single_leaf(sane.shape[0]))]
    frame(restore, ())
    frame([], ())
    return Sequence(W, H, scene, options, tuple(steps), cam.name)


def replay(seq):
    """[(scene as it stands, FrameParams, image written before the frame or None)] for every rendered frame"""
    cur = dict(spheres=seq.scene.spheres, materials=seq.scene.materials, meshes=seq.scene.meshes, vertices=seq.scene.vertices, nodes=seq.scene.nodes, envmap=seq.scene.env)
    out, written = [], None
    for s in seq.steps:
        for act in s.pre:
            if act[0] == "upload":
                cur[act[1]] = act[2]
            elif act[0] == "write_image":
                written = act[1]
        if s.refused:
            continue
        out.append((sc.Scene(cur["spheres"], cur["materials"], cur["meshes"], cur["vertices"], cur["nodes"], cur["envmap"]), s.params, written))
        written = None
    return out


def coverage(seeds=None):
    """event kind -> steps of that kind over the sequences of `seeds`"""
    out = {k: 0 for k in EVENT_KINDS}
    for seed in (default_seeds() if seeds is None else seeds):
        for s in sequence(seed).steps:
            for k in s.kinds:
                out[k] += 1
    return out


# ------------------------------------------------------------------------------------------------ the oracle's camera rays

def oracle_rays(oracle, p, W, H):
    """(h, w, 6) float32 o.xyz d.xyz of the camera rays of one frame over the 8 x 8-aligned footprint, from the CPU oracle"""
    import ctypes as C
    buf = np.full((H * W, 6), np.nan, np.float32)
    oracle.lib.oracle_set_ray_dump(buf.ctypes.data_as(C.c_void_p), C.c_uint32(0))
    try:
        oracle.render(sc.Scene(), p.replace(max_bounce=1, samples=1, use_envmap=0), np.zeros((H, W, 4), np.float32), threads=4)
    finally:
        oracle.lib.oracle_set_ray_dump(None, C.c_uint32(0))
    return buf.reshape(H, W, 6)[:H // 8 * 8, :W // 8 * 8]
