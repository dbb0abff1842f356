"""Seeded mesh-record fuzz inputs: what find_closest_mesh (:331-361) loops over, as drawn records over one vertex buffer.  numpy only, no GPU.

    visits(meshes, n_tris) -> [(mesh, triangle)]     the reference's mesh loops restated: meshes in order, each over [start, end) with
                                                     end = (start + size) mod 2^32 as the shader's `offset + count` in uint (:341), without
                                                     the indices >= n_tris (all-zero vertices: the edge tests `> 0` never pass).  Indices
                                                     only grow inside one loop, so a loop is over at min(end, n_tris): never 2^32 steps.
    kinds(meshes, n_tris)  -> set of KINDS           what the records ARE (derived from the records, not from how they were drawn)
    case(seed)     -> (scene, base FrameParams, W, H, frames) with .init, .options (kernel-4 scan options) and .target
    sequence(seed) -> Sequence(base scene, W, H, options, steps); a step = (what, meshes | None, vertices | None, FrameParams): one
                      context uploads only what the step names ("meshes", "vertices", "both") and renders the frame

Records: 0..12 over a vertex buffer of 0..400 triangles, of the kinds
  in_range       start + size <= n_tris, size > 0
  overlap        two records visit a common triangle without being the same record
  descending     a record that visits starts below the start of the visiting record before it
  gap            some triangle of the buffer is never visited although others are
  size_zero      size 0
  start_past     start >= n_tris (no wrap)
  end_past       start < n_tris < start + size (no wrap): the loop leaves the buffer
  same_twice     one visiting (start, size) listed twice
  wrap_ones      (k, 0xFFFFFFFF): end = k - 1, nothing
  wrap_to_zero   (k, 2^32 - k), k > 0: end = 0, nothing
  wrap_plus_j    (k, 2^32 - k + j), 0 < j < k (the size is a uint32): end = j, below the start, nothing
  wrap_far       (0xFFFFFFF0, 0x20): end = 0x10, nothing
  garbage_words  anything in the record's third and fourth words, which the shader never reads
Hard condition: len(visits) <= VISIT_BOUND = 2048 (a draw over it is drawn again from the same generator): the CPU oracle stays at seconds.

Visit counts are steered to the structure edges of the kernel-4 scan (10-triangle tiles, 40-triangle quads, 64-triangle bound groups,
groups and chunks of the drawn mf_group_quads / mf_chunk_quads quads, the zero quad behind the last group): EDGES, and 40 q +- 1 for the
case's own two q (left out where 40 q + 1 > VISIT_BOUND: q = 64).  case(seed) takes EDGES[seed mod 17] for seed mod 24 < 17, else one of
its own 40 q +- 1 or a free count; the steps of sequence(seed) draw from the same pool.

Geometry: a soup as scene_fuzz_inputs._soup; on half of the cases exact duplicates of earlier triangles with another material id (the
first visit in visits() order must win the tie, :349) and triangles behind and around the camera.  Materials: the tame generator's with
smoothness clamped into [0, 1] -- the tame family's only NaN source (scene_fuzz_inputs.py) is absent, the oracle's images hold no NaN.
Vertex w: material ids that fit an int32 (valid, -1, past the table, 2^20, -2^31 + 128); int() of anything else is undefined in GLSL and
is not fuzzed against the reference.  The vertex buffer always holds whole triangles.
Sizes W in 16..96, H in 8..64 (mostly no multiple of 8); 1..3 frames with an optional reset frame; max_bounce 0..8; samples 1..2.

SKIPPED_SEEDS: seeds whose oracle image breaks the no-NaN condition, with the reason; default_seeds() leaves them out (at most 2).
"""
from collections import namedtuple

import numpy as np

import golden_cases as gc
import scene_fuzz_inputs as sf

sc = sf.sc
M32 = 0xFFFFFFFF
VISIT_BOUND = 2048
MAX_RECORDS, MAX_TRIS = 12, 400
DEFAULT_CASES = 24
EDGES = (0, 1, 9, 10, 11, 39, 40, 41, 63, 64, 65, 79, 80, 81, 127, 128, 129)
KINDS = ("in_range", "overlap", "descending", "gap", "size_zero", "start_past", "end_past", "same_twice",
         "wrap_ones", "wrap_to_zero", "wrap_plus_j", "wrap_far", "garbage_words")
CHUNK_QUADS, GROUP_QUADS = (1, 2, 3, 5, 8, 16, 32), (1, 2, 4, 8, 32, 64)
SKIPPED_SEEDS = ()                                     # (seed, reason) pairs, measured on the CPU oracle (tests/test_mesh_fuzz_inputs.py): none


def default_seeds(n=DEFAULT_CASES, start=0):
    out, s, skipped = [], start, {seed for seed, _ in SKIPPED_SEEDS}
    while len(out) < n:
        if s not in skipped:
            out.append(s)
        s += 1
    return out


# ------------------------------------------------------------------------------------------------ the mesh loops, restated

def _records(meshes):
    u = np.ascontiguousarray(meshes, np.uint32).reshape(-1, 4)
    return [(int(u[i, 0]), int(u[i, 1])) for i in range(u.shape[0])]


def spans(meshes, n_tris):
    """[(mesh, first, end)] of every record that visits something: triangles first .. end - 1"""
    out = []
    for m, (start, size) in enumerate(_records(meshes)):
        end = min((start + size) & M32, n_tris)            # uint32 like the shader's; past the buffer nothing can be hit
        if start < end:
            out.append((m, start, end))
    return out


def visits(meshes, n_tris):
    return [(m, t) for m, a, b in spans(meshes, n_tris) for t in range(a, b)]


def count(meshes, n_tris):
    return sum(b - a for _, a, b in spans(meshes, n_tris))


def kinds(meshes, n_tris):
    u = np.ascontiguousarray(meshes, np.uint32).reshape(-1, 4)
    recs, sp, out = _records(u), spans(u, n_tris), set()
    for start, size in recs:
        total = start + size
        if size == 0:
            out.add("size_zero")
        if (start, size) == (0xFFFFFFF0, 0x20):
            out.add("wrap_far")
        elif size == M32 and total > M32:
            out.add("wrap_ones")
        elif total == 1 << 32:
            out.add("wrap_to_zero")
        elif total > 1 << 32:
            out.add("wrap_plus_j")
        elif start >= n_tris:
            out.add("start_past")
        elif total > n_tris:
            out.add("end_past")
        elif size:
            out.add("in_range")
    if u[:, 2:].any():
        out.add("garbage_words")
    seen = set()
    for i, (m, a, b) in enumerate(sp):
        if i and a < sp[i - 1][1]:
            out.add("descending")
        if recs[m] in seen:
            out.add("same_twice")
        seen.add(recs[m])
        if any(a < b0 and a0 < b and recs[m] != recs[m0] for m0, a0, b0 in sp[:i]):
            out.add("overlap")
    if sp and len({t for _, a, b in sp for t in range(a, b)}) < n_tris:
        out.add("gap")
    return out


def duplicate_groups(vertices):
    """triangle index -> key shared by the triangles with identical vertex positions"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3, 4)
    return [v[i, :, :3].tobytes() for i in range(v.shape[0])]


# ------------------------------------------------------------------------------------------------ records

def _draw_records(rng, n, target):
    """up to MAX_RECORDS records over n triangles whose visits() count is `target`; None when the draw does not get there"""
    recs, c = [], 0
    n_rec = int(rng.integers(0, MAX_RECORDS + 1))
    names = ["in_range", "overlap", "descending", "gap", "size_zero", "start_past", "end_past", "same_twice", "wrap_ones", "wrap_to_zero",
             "wrap_plus_j", "wrap_far"]

    def visiting():
        return [r for r in recs if count(np.array([r + (0, 0)], np.uint32), n)]

    for _ in range(n_rec):
        room = target - c
        kind = str(rng.choice(names))
        k = int(rng.integers(0, n + 1))
        rec = None
        if kind == "size_zero":
            rec = (int(rng.integers(0, n + 8)), 0)
        elif kind == "start_past":
            rec = (n + int(rng.choice([0, 1, 7, 1000, 1 << 30])), int(rng.integers(1, 50)))
        elif kind == "wrap_ones":
            rec = (k, M32)
        elif kind == "wrap_to_zero":
            rec = (max(k, 1), (1 << 32) - max(k, 1))
        elif kind == "wrap_far":
            rec = (0xFFFFFFF0, 0x20)
        elif kind == "wrap_plus_j":
            k = max(k, 2)                                  # (the size is a uint32: j < k)
            rec = (k, (1 << 32) - k + int(rng.integers(1, k)))
        elif n and room > 0:
            prev = visiting()
            if kind == "same_twice" and prev:
                rec = prev[int(rng.integers(len(prev)))]
            elif kind == "end_past":                       # the last `size` triangles and on past the buffer
                size = int(rng.integers(1, min(room, n) + 1))
                rec = (n - size, size + int(rng.choice([1, 2, 7, 40, 1 << 20])))
            elif kind == "overlap" and prev:               # begins inside an earlier record
                a, s = prev[int(rng.integers(len(prev)))]
                a = min(a, n - 1)
                start = int(rng.integers(a, min(a + s, n)))
                rec = (start, int(rng.integers(1, min(room, n - start) + 1)))
            elif kind == "descending" and prev and prev[-1][0] > 0:
                start = int(rng.integers(0, min(prev[-1][0], n)))
                rec = (start, int(rng.integers(1, min(room, n - start) + 1)))
            else:                                          # in_range; gap: a short one somewhere
                start = int(rng.integers(0, n))
                most = min(room, n - start)
                rec = (start, int(rng.integers(1, (min(most, 5) if kind == "gap" else most) + 1)))
        if rec is None:
            continue
        got = count(np.array([rec + (0, 0)], np.uint32), n)
        if c + got > target:
            continue
        recs.append(rec)
        c += got
    while c < target and n:                                # the rest in range
        size = min(target - c, n)
        recs.append((int(rng.integers(0, n - size + 1)), size))
        c += size
    if c != target or len(recs) > MAX_RECORDS:
        return None
    if len(recs) > 1 and rng.random() < 0.5:               # the fill-up records do not always come last
        order = rng.permutation(len(recs))
        recs = [recs[i] for i in order]
    out = np.zeros((len(recs), 4), np.uint32)
    for i, (start, size) in enumerate(recs):
        out[i, 0], out[i, 1] = start, size
    if len(recs) and rng.random() < 0.5:                   # the words the shader never reads
        rows = rng.random(len(recs)) < 0.6
        out[rows, 2:] = rng.integers(0, 1 << 32, (int(rows.sum()), 2), dtype=np.uint64).astype(np.uint32)
    return out


def records(rng, n, target):
    """the hard conditions hold by redrawing from the same generator"""
    assert target <= min(VISIT_BOUND, MAX_RECORDS * n)
    while True:
        out = _draw_records(rng, n, target)
        if out is not None and count(out, n) == target <= VISIT_BOUND:
            return out


# ------------------------------------------------------------------------------------------------ pieces

def _target_pool(options):
    o = dict(options)
    own = [40 * q + d for q in (o["mf_group_quads"], o["mf_chunk_quads"]) for d in (-1, 1) if 40 * q + 1 <= VISIT_BOUND]
    return own


def _options(rng):
    return (("kernel", 4), ("scan_waves", int(rng.integers(0, 3))), ("scan_dynamic", int(rng.integers(0, 5))), ("cull", int(rng.integers(0, 4))),
            ("sort_min_rays", int(rng.choice([0, 0, 3000, 65536]))), ("mf_chunk_quads", int(rng.choice(CHUNK_QUADS))),
            ("mf_group_quads", int(rng.choice(GROUP_QUADS))))


def _n_tris_for(rng, target):
    if target == 0:
        return 0 if rng.random() < 0.25 else int(rng.integers(1, MAX_TRIS + 1))
    return int(rng.integers(max(1, -(-target // 6)), MAX_TRIS + 1))


def _material_ids(rng, n_mat, size):
    """valid ids, -1 and ids past the table -- every one an int32 that float32 holds exactly"""
    odd = np.array([-1, n_mat, n_mat + 3, 1 << 20, -(1 << 31) + 128], np.int64)
    return np.where(rng.random(size) < 0.75, rng.integers(0, n_mat, size), rng.choice(odd, size)).astype(np.int64)


def _vertices(rng, n, n_mat, pos, fwd, right, up, extras):
    """(3 n, 4) float32: a soup in front of the camera; with `extras` also triangles behind and around the camera and exact duplicates
    of earlier triangles under another material id"""
    if n == 0:
        return np.zeros((0, 4), np.float32)
    dist = rng.uniform(5, 50, n)
    c = pos + fwd * dist[:, None] + right * (rng.uniform(-0.5, 0.5, n) * dist)[:, None] + up * (rng.uniform(-0.5, 0.5, n) * dist)[:, None]
    size = np.where(rng.random(n) < 0.1, rng.uniform(3, 12, n), rng.uniform(0.05, 2.0, n))
    if extras:
        behind = rng.random(n) < 0.1                       # behind the camera: never seen directly, hit by bounced rays
        c[behind] = pos - fwd * dist[behind, None] + right * rng.uniform(-8, 8, (int(behind.sum()), 1))
        around = rng.random(n) < 0.06                      # large, within a few units of the camera: some enclose its ray origins' plane
        c[around] = pos + rng.normal(size=(int(around.sum()), 3)) * 2.0
        size[around] = rng.uniform(4, 30, int(around.sum()))
    tri = c[:, None, :] + rng.normal(size=(n, 3, 3)) * size[:, None, None]
    v = np.zeros((n, 3, 4), np.float32)
    v[..., :3] = tri.astype(np.float32)
    ids = _material_ids(rng, n_mat, n)
    if extras and n > 1:
        for j in np.flatnonzero(rng.random(n) < 0.15):
            if j:
                i = int(rng.integers(0, j))
                v[j, :, :3] = v[i, :, :3]
                ids[j] = (ids[i] + 1 + int(rng.integers(0, max(n_mat - 1, 1)))) % n_mat if 0 <= ids[i] < n_mat and n_mat > 1 else int(rng.integers(0, n_mat))
    v[..., 3] = ids.astype(np.float32)[:, None]
    assert (v[..., 3].astype(np.int64) == ids[:, None]).all()
    return v.reshape(-1, 4)


def _materials(rng):
    mats = sf._materials(rng)
    mats[:, 3] = np.clip(mats[:, 3], 0.0, 1.0)             # smoothness: the tame family's NaN source (scene_fuzz_inputs.py) left out
    return mats


def _base_scene(rng, pos, fwd, right, up):
    mats = _materials(rng)
    if rng.random() < 0.5:
        spheres = sf._spheres(rng, mats, pos, fwd, right, up)
        nodes = sf._bounded_nodes(rng, spheres.shape[0], False)
    else:
        spheres, nodes = np.zeros((0, 8), np.float32), np.zeros((0, 12), np.float32)
    return sc.Scene(spheres=spheres, materials=mats, nodes=nodes, env=sf._env(rng))


def _params(rng, cam):
    return sc.FrameParams(max_bounce=int(rng.integers(0, 9)), samples=int(rng.integers(1, 3)), use_envmap=int(rng.random() < 0.6),
                          background=tuple(float(np.float32(x)) for x in rng.uniform(-0.5, 2.0, 3)), **cam)


class Case(tuple):
    """(scene, base FrameParams, W, H, frames) with .init, .options and .target"""
    init = "zeros"
    options = ()
    target = 0


def case(seed):
    rng = np.random.default_rng([int(seed), 7, 20261])
    W, H = int(rng.integers(16, 97)), int(rng.integers(8, 65))
    cam, pos, fwd, right, up = sf._camera(rng)
    scene = _base_scene(rng, pos, fwd, right, up)
    options = _options(rng)
    slot = int(seed) % DEFAULT_CASES
    if slot < len(EDGES):
        target = EDGES[slot]
    else:
        own = _target_pool(options)
        target = int(rng.choice(own)) if own and rng.random() < 0.7 else int(rng.integers(0, 600))
    n = _n_tris_for(rng, target)
    scene.vertices = _vertices(rng, n, scene.materials.shape[0], pos, fwd, right, up, extras=rng.random() < 0.5)
    scene.meshes = records(rng, n, target)
    base = _params(rng, cam)
    n_frames = int(rng.integers(1, 4))
    reset_at = int(rng.integers(2, n_frames + 1)) if n_frames > 1 and rng.random() < 0.5 else 0
    g = sc.GlibcRand(int(seed))
    frames, m_frames = [], 0
    for i in range(1, n_frames + 1):                   # the reference's frame loop (golden_cases.frame_sequence)
        m_frames += 1
        frames.append(base.replace(frames=m_frames, random=g.rand(), reset_flag=int(i == reset_at)))
        if i == reset_at:
            m_frames = 0
    out = Case((scene, base, W, H, frames))
    out.init = "ramp" if rng.random() < 0.3 else "zeros"
    out.options, out.target = options, target
    return out


# ------------------------------------------------------------------------------------------------ upload sequences

Sequence = namedtuple("Sequence", "scene W H options steps")      # scene: spheres, materials, nodes, cube map; no meshes, no vertices
Step = namedtuple("Step", "what meshes vertices params")           # what: "meshes" | "vertices" | "both"; the part not uploaded is None


def sequence(seed):
    """4..6 steps on one context, a frame after each.  Holds a step of zero visits with vertices present that a visiting step follows, and
    a step with more visits than every step before it (it comes after the zero step: buffers shrink, then grow past their old size)."""
    rng = np.random.default_rng([int(seed), 11, 20261])
    W, H = int(rng.integers(16, 97)), int(rng.integers(8, 65))
    cam, pos, fwd, right, up = sf._camera(rng)
    scene = _base_scene(rng, pos, fwd, right, up)
    n_mat = scene.materials.shape[0]
    options = tuple((k, v) for k, v in _options(rng) if k not in ("cull", "sort_min_rays")) + (("cull", 3), ("sort_min_rays", 0))
    pool = [e for e in EDGES if e] + _target_pool(options)
    base = _params(rng, cam).replace(max_bounce=int(rng.integers(1, 7)))
    n_steps = int(rng.integers(4, 7))
    zero_at = int(rng.integers(1, n_steps - 1))
    grow_at = int(rng.integers(zero_at + 1, n_steps))
    g = sc.GlibcRand(int(seed) + 1000)
    steps, n, meshes, most, m_frames = [], 0, None, 0, 0
    for i in range(n_steps):
        what = "both" if i == 0 else str(rng.choice(["meshes", "vertices", "both"]))
        if i in (zero_at, grow_at) and what == "vertices":
            what = "meshes"
        target = 0 if i == zero_at else int(rng.choice(pool))
        if i == grow_at:
            bigger = [e for e in pool if e > most]
            target = int(rng.choice(bigger)) if bigger else most + int(rng.integers(1, 60))
        new_v = new_m = None
        if what in ("vertices", "both"):
            if what == "vertices":                         # the records stay: the count follows from the new buffer's size
                other = n if rng.random() < 0.5 else int(rng.integers(1, MAX_TRIS + 1))
                n = other if count(meshes, other) <= VISIT_BOUND else n
            else:
                n = int(rng.integers(max(1, -(-max(target, 1) // 6)), MAX_TRIS + 1))
            new_v = _vertices(rng, n, n_mat, pos, fwd, right, up, extras=rng.random() < 0.5)
        if what in ("meshes", "both"):
            target = min(target, 6 * n)
            if i == grow_at and target <= most:            # the buffer on the device is too small for more visits: new vertices too
                what, n = "both", int(rng.integers(max(1, -(-(most + 60) // 6)), MAX_TRIS + 1))
                new_v = _vertices(rng, n, n_mat, pos, fwd, right, up, extras=False)
                target = most + int(rng.integers(1, 60))
            meshes = new_m = records(rng, n, target)
        most = max(most, count(meshes, n))
        m_frames += 1
        reset = int(i > 0 and rng.random() < 0.25)
        steps.append(Step(what, new_m, new_v, base.replace(frames=m_frames, random=g.rand(), reset_flag=reset)))
        if reset:
            m_frames = 0
    return Sequence(scene, W, H, options, steps)


def replay(seq):
    """[(scene as it stands after step k, FrameParams of step k)]"""
    out, meshes, vertices = [], None, None
    for st in seq.steps:
        meshes = st.meshes if st.meshes is not None else meshes
        vertices = st.vertices if st.vertices is not None else vertices
        out.append((sc.Scene(seq.scene.spheres, seq.scene.materials, meshes, vertices, seq.scene.nodes, seq.scene.env), st.params))
    return out


# ------------------------------------------------------------------------------------------------ named records

def named_records(n):
    """name -> [(start, size)]: the record sets of the reference goldens tests/golden/meshrec_<name>.npz, over a buffer of n triangles"""
    return gc.mesh_record_sets(n)


def make_meshes(recs):
    return gc.mesh_records(recs)
