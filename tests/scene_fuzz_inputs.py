"""Seeded scene-content fuzz inputs: spheres, node graphs, materials, cube maps, cameras and frame sequences.  numpy only, no GPU.

    case(seed, family) -> (scene, base FrameParams, W, H, frames)        frames: the list of per-frame FrameParams to render in order;
                                                                         the returned tuple also carries .init ("zeros" | "ramp", the
                                                                         image the context is preloaded with: golden_cases.initial_image)
                                                                         and, for "mixed", .options (kernel-4 scan options)

Families (FAMILIES):
  tame   1..24 spheres (radii 0.01 .. 1e4; in front of, around and enclosing the camera; exact duplicates with another material, so the
         first visit must win the tie; nested glass), 1..10 materials of types 0, 1, 2 and the unknown 3, 7 (smoothness inside and outside
         [0, 1], emission on a quarter), sphere material ids that include -1 and ids past the table, node graphs of 1..12 nodes (forward
         links, INVALID, both children equal, nodes reachable twice, combs that overflow the 5-entry stack, leaves with count 0, inner
         nodes with spheres, overlapping ranges, ranges that end past the sphere buffer), cube maps (none, noise_cubemap of face size
         1, 2, 3, 8 with 3 or 4 channels, 5 faces only; use_envmap on and off, also on without a cube map: shader_params()), cameras
         (fov in (0.2, 2.4), rotated / non-unit / slightly non-orthogonal basis, aperture 0 / 0.001 / 0.5, focal length 5..45),
         background outside [0, 1], max_bounce 0..10, samples 1..3, 1..3 frames with a reset frame in mid-sequence, a preloaded ramp image.
  wild   tame plus: one special value (NaN, +-inf, 1e30, negative) in one material field; a sphere of radius 0, negative, NaN or inf; an
         infinite centre; back links and self links (cycles); child ids past the node buffer; offset / count that wrap in 32 bits:
         (k, 0xFFFFFFFF), (k, 2^32 - k), (0xFFFFFFF0, 0x20).
  mixed  tame spheres, nodes and materials plus a soup of 1..300 triangles whose w material ids come from the same out-of-range-rich
         set; .options holds random kernel-4 scan options in the ranges of tests/test_gpu_fuzz_parity.py.

Sizes: W in 16..96, H in 8..64 (mostly no multiple of 8).

Hard condition on every node buffer drawn here: walk() below -- the plain restatement of the reference's node walk (stack of 5 with
dropped pushes, 65535-pop cap, loop bound offset + count in uint32) -- makes at most VISIT_BOUND = 4096 sphere tests per ray; a draw over
the bound is drawn again from the same generator.  (A cycle with a large count would otherwise make the CPU oracle run for hours.)

NaN conditions (tests/test_scene_fuzz_inputs.py asserts them on the CPU oracle over default_seeds(family)):
  tame, mixed   no NaN in any image;
  wild          at most 2 % of the pixels of the family, at most 25 % of any single case.
Seeds that break their family's condition are listed in SKIPPED_SEEDS, which default_seeds() leaves out.
SKIPPED_SEEDS was measured on the CPU oracle over seeds 0..63 of every family (a longer campaign extends it first).  The NaN in the
tame and mixed seeds it lists comes from a specular material with smoothness outside [0, 1]: the bounced direction is not normalised
(the reference's own quirk), and with |d| > 1 the all-zero sphere of an index past the buffer can be "hit", which divides by its radius 0.
Measured shares, all frames of every case, a pixel counted when any component is a NaN after any frame:
  seeds 0..63       tame 1 case with NaN (5 pixels)   mixed 2 cases (4 and 206 pixels)   wild 9 cases, 4 of them over 25 %
  24 default seeds  tame 0 of 47,552 pixels           mixed 0 of 41,856 pixels            wild 14 of 38,336 pixels = 0.04 %, in 2 cases,
                                                                                          largest single case 0.78 %
"""
from collections import namedtuple

import numpy as np

import raytracer_glsl_amd

sc = raytracer_glsl_amd.scenes
INVALID = sc.INVALID
NO_SPHERE = 0xFFFFFFFF                 # kNoSphere: how the flattened walk names the all-zero sphere of an index past the buffer

FAMILIES = ("tame", "wild", "mixed")
DEFAULT_CASES = 24
VISIT_BOUND = 4096
STACK, POP_CAP = 5, 65535
NAN_CAP_FAMILY, NAN_CAP_CASE = 0.02, 0.25
# seeds whose oracle images break the family's NaN condition (measured on the CPU oracle, seeds 0..63); default_seeds() skips them
SKIPPED_SEEDS = {"tame": (52,), "wild": (3, 39, 42, 55), "mixed": (9, 25)}


def default_seeds(family, n=DEFAULT_CASES, start=0):
    """the first n seeds from `start` that SKIPPED_SEEDS does not list"""
    out, s = [], start
    while len(out) < n:
        if s not in SKIPPED_SEEDS[family]:
            out.append(s)
        s += 1
    return out


# ------------------------------------------------------------------------------------------------ the node walk, restated

Walk = namedtuple("Walk", "runs visits dropped pops")     # runs: [(first index, bound)] of every non-empty sphere loop, in test order


def walk(nodes, bound=None):
    """The reference's traverse() over `nodes` as far as it does not depend on the ray.  None when the walk makes more than `bound`
    sphere tests."""
    u = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12).view(np.uint32)
    n = u.shape[0]
    rec = [tuple(int(x) for x in u[i, 8:12]) for i in range(n)]
    runs, visits, dropped, pops = [], 0, 0, 0
    stack = [0] if n else []
    while stack and pops < POP_CAP:
        node = stack.pop()
        pops += 1
        left, right, offset, count = rec[node] if node < n else (INVALID, INVALID, 0, 0)
        for child in (left, right):
            if child != INVALID:
                if len(stack) < STACK:
                    stack.append(child)
                else:
                    dropped += 1
        end = (offset + count) & 0xFFFFFFFF
        if end > offset:
            runs.append((offset, end))
            visits += end - offset
            if bound is not None and visits > bound:
                return None
    return Walk(runs, visits, dropped, pops)


def expand(w):
    """every sphere index the walk tests, in order"""
    return [i for a, b in w.runs for i in range(a, b)]


def device_visits(w, n_spheres):
    """the walk as the device reads it: indices inside the buffer, and ONE NO_SPHERE for the rest of a loop that leaves the buffer"""
    out = []
    for a, b in w.runs:
        out.extend(range(a, min(b, n_spheres)))
        if b > n_spheres:
            out.append(NO_SPHERE)
    return out


def wrapped_nodes(nodes):
    """indices of the node records whose offset + count wraps in 32 bits"""
    u = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12).view(np.uint32).astype(np.uint64)
    return [i for i in range(u.shape[0]) if u[i, 11] and u[i, 10] + u[i, 11] >= (1 << 32)]


# ------------------------------------------------------------------------------------------------ pieces

def _unit(v):
    return v / np.sqrt((v * v).sum())


def _camera(rng):
    pos = rng.uniform([-5, -4, -40], [5, 2, -20])
    fwd, up, right = np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0]), np.array([-1.0, 0.0, 0.0])
    style = int(rng.integers(3))                       # 0: the reference's basis, 1: rotated, 2: rotated, non-unit and skewed
    if style:
        yaw, pitch, roll = rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(-0.6, 0.6)
        fwd = np.array([np.sin(yaw) * np.cos(pitch), np.sin(pitch), np.cos(yaw) * np.cos(pitch)])
        r0 = _unit(np.array([-np.cos(yaw), 0.0, np.sin(yaw)]))
        u0 = np.cross(r0, fwd)
        right, up = np.cos(roll) * r0 + np.sin(roll) * u0, np.cos(roll) * u0 - np.sin(roll) * r0
    if style == 2:
        s = rng.uniform(0.5, 1.6, 3)
        fwd, up, right = s[0] * fwd + 0.04 * up, s[1] * up + 0.05 * right, s[2] * right - 0.03 * fwd
    f32 = lambda v: tuple(float(x) for x in np.asarray(v, np.float32))
    kw = dict(camera_position=f32(pos), camera_forward=f32(fwd), camera_up=f32(up), camera_right=f32(right),
              camera_fov=float(np.float32(rng.uniform(0.2, 2.4))), camera_aperture=float(rng.choice([0.0, 0.001, 0.5])),
              camera_focal_length=float(np.float32(rng.uniform(5, 45))), use_dof=int(rng.integers(2)))
    return kw, pos, _unit(fwd), _unit(right), _unit(up)


def _materials(rng):
    n = int(rng.integers(1, 11))
    items = []
    for _ in range(n):
        typ = int(rng.choice([0, 1, 2, 3, 7], p=[0.3, 0.25, 0.25, 0.1, 0.1]))
        smooth = float(rng.uniform(0, 1)) if rng.random() < 0.6 else float(rng.choice([-0.5, 0.0, 1.0, 1.5, 3.0]))
        emission = tuple(rng.uniform(0, 20, 3)) if rng.random() < 0.25 else (0.0, 0.0, 0.0)
        items.append((tuple(rng.uniform(0.05, 1.1, 3)), emission, smooth, typ))
    return sc.make_materials(items)


def _material_ids(rng, n_mat, size):
    """valid ids, -1 and ids past the table"""
    odd = np.array([-1, n_mat, n_mat + 3, 1 << 20, -(1 << 31)], np.int64)
    ids = np.where(rng.random(size) < 0.75, rng.integers(0, n_mat, size), rng.choice(odd, size))
    return ids.astype(np.int64)


def _spheres(rng, mats, pos, fwd, right, up):
    n = int(rng.integers(1, 25))
    n_mat = mats.shape[0]
    glass = [i for i in range(n_mat) if mats[i, 7:8].view(np.uint32)[0] == 2]
    ids = _material_ids(rng, n_mat, n)
    items = []

    def direction():
        return _unit(rng.normal(size=3))

    for k in range(n):
        kind = "front" if k == 0 else str(rng.choice(["front", "small", "wall", "enclose", "duplicate", "nested"], p=[0.3, 0.1, 0.15, 0.15, 0.15, 0.15]))
        m = int(ids[k])
        if kind in ("duplicate", "nested") and items:
            cx, cy, cz, r, m0 = items[int(rng.integers(len(items)))]
            if kind == "duplicate":                    # the same sphere again, usually with another material: the first visit wins the tie
                items.append((cx, cy, cz, r, m))
            else:                                      # a glass shell and a glass core
                items.append((cx, cy, cz, float(np.float32(r * rng.uniform(0.3, 0.9))), int(rng.choice(glass)) if glass else m))
            continue
        if kind == "wall":                             # a huge sphere whose surface passes close to the camera
            r = 10.0 ** rng.uniform(2, 4)
            c = pos + direction() * (r + rng.uniform(1, 25))
        elif kind == "enclose":                        # the camera inside, off centre (glass: total internal reflection at grazing angles)
            r = 10.0 ** rng.uniform(0.5, 3)
            c = pos + direction() * (r * rng.uniform(0.0, 0.9))
            if glass and rng.random() < 0.6:
                m = int(rng.choice(glass))
        elif kind == "small":
            r = 10.0 ** rng.uniform(-2, 0)
            c = pos + fwd * rng.uniform(1, 8) + right * rng.uniform(-1, 1) + up * rng.uniform(-1, 1)
        else:
            dist = rng.uniform(6, 60)
            r = rng.uniform(0.5, 0.35 * dist)
            spread = 0.0 if k == 0 else 0.5 * dist
            c = pos + fwd * dist + right * rng.uniform(-spread, spread) + up * rng.uniform(-spread, spread)
        c = np.asarray(c, np.float32)
        items.append((float(c[0]), float(c[1]), float(c[2]), float(np.float32(r)), m))
    return sc.make_spheres(items)


def _nodes(rng, n_spheres, wild):
    n = int(rng.integers(1, 13))
    comb = rng.random() < 0.3                          # both children on every inner node: the pending right-hand sides overflow the stack
    items = []
    for i in range(n):
        def child():
            r = rng.random()
            if wild and r < 0.12:
                return int(rng.integers(0, i + 1))     # back link or self link
            if wild and r < 0.2:
                return n + int(rng.integers(0, 4))     # past the node buffer (not INVALID)
            if i + 1 < n and (comb or r < 0.7):
                return int(rng.integers(i + 1, n))     # forward link
            return INVALID
        left = child()
        right = left if rng.random() < 0.15 else child()
        if comb and i + 2 < n:
            left, right = int(rng.integers(i + 2, n)), i + 1      # the right child is popped first: the left ones wait on the stack
        inner = left != INVALID or right != INVALID
        offset = int(rng.integers(0, n_spheres + 1))
        r = rng.random()
        if r < (0.5 if inner else 0.15):
            count = 0
        elif r < 0.8:
            count = int(rng.integers(1, max(n_spheres - offset, 1) + 1))          # inside the buffer, up to its end exactly
        else:
            count = max(n_spheres - offset, 0) + int(rng.choice([1, 2, 7, 40]))   # ends past the buffer
        if i == 0 and n == 1 and rng.random() < 0.7:
            offset, count = 0, n_spheres
        if wild and rng.random() < 0.2:
            k = int(rng.integers(0, n_spheres + 1))
            offset, count = [(k, 0xFFFFFFFF), (k, (1 << 32) - k), (0xFFFFFFF0, 0x20)][int(rng.integers(3))]
            count &= 0xFFFFFFFF
        items.append(((-1e5,) * 3, (1e5,) * 3, left, right, offset, count))
    return sc.make_nodes(items)


def _bounded_nodes(rng, n_spheres, wild):
    while True:
        nodes = _nodes(rng, n_spheres, wild)
        if walk(nodes, VISIT_BOUND) is not None:
            return nodes


def _env(rng):
    r = rng.random()
    if r < 0.25:
        return None
    env = sc.noise_cubemap(int(rng.choice([1, 2, 3, 8])), int(rng.choice([3, 4])), seed=int(rng.integers(1, 1000)))
    return env[:5] if r < 0.4 else env


SPECIALS = (float("nan"), float("inf"), -float("inf"), 1e30, -0.75)


def _make_wild(rng, spheres, mats, pos, fwd, right, up):
    """one special value in one material field; one sphere of radius 0 / negative / NaN / inf; sometimes an infinite centre; sometimes a
    small sphere in view that wears the special material, so that what the value does shows in a part of the image"""
    n = spheres.shape[0]
    special = int(rng.integers(mats.shape[0]))
    mats[special, int(rng.integers(0, 7))] = np.float32(rng.choice(SPECIALS))
    k = int(rng.integers(n))
    spheres[k, 3] = np.float32(rng.choice([0.0, -1.0, -spheres[k, 3], float("nan"), float("inf")]))
    if rng.random() < 0.3:
        spheres[int(rng.integers(n)), int(rng.integers(0, 3))] = np.float32(rng.choice([float("inf"), -float("inf")]))
    if n >= 3 and rng.random() < 0.5:
        j = n - 1 if k != n - 1 else n - 2
        dist = rng.uniform(8, 30)
        c = pos + fwd * dist + right * (rng.uniform(-0.2, 0.2) * dist) + up * (rng.uniform(-0.2, 0.2) * dist)
        spheres[j, :3] = c.astype(np.float32)
        spheres[j, 3] = np.float32(rng.uniform(0.3, 0.12 * dist))
        spheres[j, 4:5].view(np.int32)[0] = special


def _soup(rng, n_mat, pos, fwd, right, up):
    n = int(rng.integers(1, 301))
    dist = rng.uniform(5, 50, n)
    c = pos + fwd * dist[:, None] + right * (rng.uniform(-0.5, 0.5, n) * dist)[:, None] + up * (rng.uniform(-0.5, 0.5, n) * dist)[:, None]
    size = np.where(rng.random(n) < 0.1, rng.uniform(3, 12, n), rng.uniform(0.05, 2.0, n))
    tri = c[:, None, :] + rng.normal(size=(n, 3, 3)) * size[:, None, None]
    v = np.zeros((n, 3, 4), np.float32)
    v[..., :3] = tri.astype(np.float32)
    v[..., 3] = _material_ids(rng, n_mat, n).astype(np.float32)[:, None]
    split = int(rng.integers(0, n + 1)) if rng.random() < 0.4 else n
    meshes = sc.make_meshes([(0, split, 0)] + ([(split, n - split, 0)] if split < n else []))
    return v.reshape(-1, 4), meshes


def shader_params(scene, p):
    """the uniforms the shader receives for the application's `p`: without a cube map object the reference's host uploads u_use_envmap =
    false whatever the application asked for (src/renderer.cpp:104-110), and so does the library; the oracle restates the shader alone"""
    return p if scene.env is not None else p.replace(use_envmap=0)


class Case(tuple):
    """(scene, base FrameParams, W, H, frames) with .init and .options"""
    init = "zeros"
    options = ()


def case(seed, family):
    assert family in FAMILIES
    rng = np.random.default_rng([int(seed), FAMILIES.index(family), 20260])
    wild = family == "wild"
    W = int(rng.integers(16, 97))
    H = int(rng.integers(8, 65))
    cam, pos, fwd, right, up = _camera(rng)
    mats = _materials(rng)
    spheres = _spheres(rng, mats, pos, fwd, right, up)
    if wild:
        _make_wild(rng, spheres, mats, pos, fwd, right, up)
    nodes = _bounded_nodes(rng, spheres.shape[0], wild)
    scene = sc.Scene(spheres=spheres, materials=mats, nodes=nodes, env=_env(rng))
    if family == "mixed":
        scene.vertices, scene.meshes = _soup(rng, mats.shape[0], pos, fwd, right, up)
    base = sc.FrameParams(max_bounce=int(rng.integers(0, 11)), samples=int(rng.integers(1, 4)), use_envmap=int(rng.random() < 0.6),
                          background=tuple(float(np.float32(x)) for x in rng.uniform(-0.5, 2.0, 3)), **cam)
    n_frames = int(rng.integers(1, 4))
    reset_at = int(rng.integers(2, n_frames + 1)) if n_frames > 1 and rng.random() < 0.5 else 0
    g = sc.GlibcRand(int(seed))
    frames, m_frames = [], 0
    for i in range(1, n_frames + 1):                    # the reference's frame loop (golden_cases.frame_sequence)
        m_frames += 1
        frames.append(base.replace(frames=m_frames, random=g.rand(), reset_flag=int(i == reset_at)))
        if i == reset_at:
            m_frames = 0
    out = Case((scene, base, W, H, frames))
    out.init = "ramp" if rng.random() < 0.3 else "zeros"
    if family == "mixed":
        out.options = (("kernel", 4), ("scan_waves", int(rng.integers(0, 3))), ("scan_dynamic", int(rng.integers(0, 5))), ("cull", int(rng.integers(0, 4))),
                       ("sort_min_rays", int(rng.choice([0, 0, 3000, 65536]))), ("mf_chunk_quads", int(rng.choice([1, 2, 3, 5, 8, 16, 32]))),
                       ("mf_group_quads", int(rng.choice([1, 2, 4, 8, 32, 64]))))
    return out
