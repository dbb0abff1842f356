"""tests/mesh_fuzz_inputs.py on the CPU: the generator is deterministic and keeps its conditions, the default seeds cover every record kind
and every visit-count edge, the oracle's images hold no NaN, the C oracle's mesh loops make exactly the triangle tests that the Python
restatement visits() lists, and the library's own expansion (raytracer.glsl_amd/csrc/rt_mesh_visits.hpp, built alone with the host
compiler and the sanitizers through tests/cpp/mesh_visits_check.cpp) equals visits() on the named records, the fuzz cases and every step
of the upload sequences.

How the oracle's counter is tied to visits(): find_closest_mesh runs once per path segment, so
  * on the case's last frame, triangle_tests == segments x len(visits), both counters of the same render;
  * on a frame of one bounce the number of segments does not depend on what is hit; there it is taken from the triangle_tests counter
    of the same scene under the single record (0, 1), and triangle_tests of the case's records == len(visits) x that number."""
import os
import re
import subprocess

import numpy as np
import pytest

import golden_cases as gc
import mesh_fuzz_inputs as mf
import scene_fuzz_inputs as sf
from test_scene_fuzz_inputs import scene_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer.glsl_amd", "csrc")
SEEDS = mf.default_seeds()


# ------------------------------------------------------------------------------------------------ visits()

T = 1 << 32
NAMED_VISITS = {                                       # (records, n_tris, visits)
    "in_range": ([(2, 3)], 6, [(0, 2), (0, 3), (0, 4)]),
    "bound_is_n_tris": ([(4, 2)], 6, [(0, 4), (0, 5)]),
    "end_past": ([(4, 9)], 6, [(0, 4), (0, 5)]),
    "far_past_without_wrap": ([(5, T - 6)], 6, [(0, 5)]),
    "start_at_n_tris": ([(6, 1)], 6, []),
    "start_past": ([(9, 3)], 6, []),
    "size_zero": ([(3, 0)], 6, []),
    "wrap_ones": ([(2, T - 1)], 6, []),
    "wrap_ones_at_zero": ([(0, T - 1)], 6, [(0, t) for t in range(6)]),      # 0 + (2^32 - 1) does not wrap
    "wrap_to_zero": ([(2, T - 2)], 6, []),
    "wrap_plus_j": ([(5, T - 5 + 2)], 6, []),          # end = 2, below the start (j < k always: the size is a uint32)
    "wrap_far": ([(0xFFFFFFF0, 0x20)], 6, []),
    "wrap_to_n_tris": ([(T - 10, 16)], 6, []),
    "wrap_then_whole": ([(3, T - 1), (0, 6)], 6, [(1, t) for t in range(6)]),
    "overlap_descending": ([(3, 3), (1, 4)], 6, [(0, 3), (0, 4), (0, 5), (1, 1), (1, 2), (1, 3), (1, 4)]),
    "same_twice": ([(1, 2), (1, 2)], 6, [(0, 1), (0, 2), (1, 1), (1, 2)]),
    "no_records": ([], 6, []),
    "no_triangles": ([(0, 3), (0, T - 1)], 0, []),
}


@pytest.fixture(scope="module")
def library_visits(tmp_path_factory):
    """tests/cpp/mesh_visits_check.cpp under the address and undefined-behaviour sanitizers: [(meshes, n_tris)] -> [[(mesh, tri)]]"""
    exe = str(tmp_path_factory.mktemp("mesh_visits") / "mesh_visits_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "mesh_visits_check.cpp"), "-o", exe])

    def run(sets):
        lines = []
        for meshes, n in sets:
            u = np.ascontiguousarray(meshes, np.uint32).reshape(-1, 4)
            lines.append(" ".join(str(int(x)) for x in [n, u.shape[0]] + u.ravel().tolist()))
        done = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert done.returncode == 0, done.stderr
        out = []
        for line in done.stdout.splitlines():
            w = [int(x) for x in line.split()]
            assert len(w) == 1 + 2 * w[0]
            out.append(list(zip(w[1::2], w[2::2])))
        assert len(out) == len(sets)
        return out
    return run


def test_visits_of_named_records_and_the_library_expansion(library_visits):
    names = sorted(NAMED_VISITS)
    sets = [(gc.mesh_records(NAMED_VISITS[k][0]), NAMED_VISITS[k][1]) for k in names]
    got = library_visits(sets)
    for k, (meshes, n), g in zip(names, sets, got):
        assert mf.visits(meshes, n) == NAMED_VISITS[k][2], k
        assert g == NAMED_VISITS[k][2], f"{k}: the library expands to {g}"
        assert mf.count(meshes, n) == len(g)


def test_library_expansion_equals_visits_on_goldens_cases_and_sequences(library_visits):
    sets = [(gc.mesh_records(r), 400) for r in mf.named_records(400).values()]
    for seed in range(64):
        scene = mf.case(seed)[0]
        sets.append((scene.meshes, scene.n_triangles))
        sets += [(s.meshes, s.n_triangles) for s, _ in mf.replay(mf.sequence(seed))]
    got = library_visits(sets)
    wrapped = 0
    for (meshes, n), g in zip(sets, got):
        assert g == mf.visits(meshes, n)
        wrapped += bool(mf.kinds(meshes, n) & {"wrap_ones", "wrap_to_zero", "wrap_plus_j", "wrap_far"})
    assert wrapped > 100


def test_the_wrapped_golden_records_visit_nothing_where_a_64_bit_bound_visits_the_rest():
    rec = mf.named_records(400)
    for name, start in (("wrap_all_ones", 5), ("wrap_below_start", 100), ("wrap_to_zero", 7)):
        (s, size), = rec[name]
        assert s == start and mf.visits(gc.mesh_records(rec[name]), 400) == [] and min(s + size, 400) - s == 400 - start
    assert [len(mf.visits(gc.mesh_records(rec[k]), 400)) for k in ("wrap_far_start", "wrap_to_n", "wrap_then_whole", "start_past_buffer", "zero_sizes_and_gaps",
                                                                  "reversed_overlap", "no_records", "single_triangles_134")] == [0, 0, 400, 200, 88, 600, 0, 134]


def test_the_library_calls_the_header_and_keeps_no_copy():
    with open(os.path.join(CSRC, "rt_mesh_visits.hpp")) as f:
        header = f.read()
    assert sorted(re.findall(r"#include\s+(\S+)", header)) == ["<cstddef>", "<cstdint>", "<cstring>", "<vector>"]
    with open(os.path.join(CSRC, "rtgl_amd.hip")) as f:
        code = "".join(re.sub(r"//.*", "", line) for line in f)
    assert "rt_mesh_visits::expand(" in code
    assert not re.search(r"\(uint64_t\)\s*start\s*\+\s*size", code)
    with open(os.path.join(ROOT, "oracle", "pathtrace_oracle.c")) as f:
        assert not re.search(r"\(uint64_t\)\s*start\s*\+\s*size", f.read())


# ------------------------------------------------------------------------------------------------ generator

def test_generator_is_deterministic_and_keeps_its_conditions():
    odd_sizes = 0
    for seed in range(40):
        a, b = mf.case(seed), mf.case(seed)
        assert scene_bytes(a[0]) == scene_bytes(b[0]) and a[1:] == b[1:] and (a.init, a.options, a.target) == (b.init, b.options, b.target)
        scene, base, W, H, frames = a
        n = scene.n_triangles
        assert 16 <= W <= 96 and 8 <= H <= 64 and 1 <= len(frames) <= 3 and sum(p.reset_flag for p in frames) <= 1
        assert 0 <= n <= mf.MAX_TRIS and scene.vertices.shape[0] == 3 * n and 0 <= scene.meshes.shape[0] <= mf.MAX_RECORDS
        assert 0 <= base.max_bounce <= 8 and 1 <= base.samples <= 2
        assert len(mf.visits(scene.meshes, n)) == mf.count(scene.meshes, n) == a.target <= mf.VISIT_BOUND
        assert ((scene.materials[:, 3] >= 0) & (scene.materials[:, 3] <= 1)).all()
        w = scene.vertices[:, 3]
        assert (w == np.trunc(w)).all() and (np.abs(w) < 2.0 ** 31).all(), "a vertex w that is no int32"
        o = dict(a.options)
        assert o["kernel"] == 4 and o["mf_chunk_quads"] in mf.CHUNK_QUADS and o["mf_group_quads"] in mf.GROUP_QUADS
        odd_sizes += bool(W % 8 or H % 8)
    assert odd_sizes > 20
    assert scene_bytes(mf.case(0)[0]) != scene_bytes(mf.case(1)[0])


def test_sequences_are_deterministic_and_hold_a_zero_step_and_a_growing_step():
    whats = set()
    for seed in range(40):
        a, b = mf.sequence(seed), mf.sequence(seed)
        assert scene_bytes(a.scene) == scene_bytes(b.scene) and a[1:4] == b[1:4] and len(a.steps) == len(b.steps)
        for x, y in zip(a.steps, b.steps):
            assert x.what == y.what and x.params == y.params
            for p, q in ((x.meshes, y.meshes), (x.vertices, y.vertices)):
                assert (p is None) == (q is None) and (p is None or p.tobytes() == q.tobytes())
            assert (x.meshes is not None) == (x.what in ("meshes", "both")) and (x.vertices is not None) == (x.what in ("vertices", "both"))
        assert 4 <= len(a.steps) <= 6 and a.steps[0].what == "both"
        assert dict(a.options)["cull"] == 3 and dict(a.options)["sort_min_rays"] == 0 and dict(a.options)["kernel"] == 4
        counts = [mf.count(s.meshes, s.n_triangles) for s, _ in mf.replay(a)]
        assert max(counts) <= mf.VISIT_BOUND
        zero = [i for i, c in enumerate(counts) if c == 0]
        assert any(max(counts[:i], default=0) > 0 and max(counts[i + 1:], default=0) > 0 for i in zero), f"seed {seed}: no change to zero visits and back: {counts}"
        assert all(s.n_triangles > 0 for (s, _), c in zip(mf.replay(a), counts) if c == 0), "zero visits without vertices"
        assert any(i > zero[0] and c > max(counts[:i]) for i, c in enumerate(counts) if i), f"seed {seed}: no step with more visits than every earlier one: {counts}"
        whats |= {s.what for s in a.steps}
    assert whats == {"meshes", "vertices", "both"}


def test_default_seeds_cover_every_record_kind_and_visit_edge():
    """every kind and every edge at least twice over the default seeds: the records of case(seed) and of every step of sequence(seed)
    for the kinds; the visit counts of both for the edges (17 edges twice are more than 24 single cases can hold)"""
    kinds_case, kinds_seq = {k: 0 for k in mf.KINDS}, {k: 0 for k in mf.KINDS}
    edges_case, edges_seq = {e: 0 for e in mf.EDGES}, {e: 0 for e in mf.EDGES}
    own = 0
    for seed in SEEDS:
        c = mf.case(seed)
        scene = c[0]
        for k in mf.kinds(scene.meshes, scene.n_triangles):
            kinds_case[k] += 1
        n = mf.count(scene.meshes, scene.n_triangles)
        if n in edges_case:
            edges_case[n] += 1
        q = mf.sequence(seed)
        for (s, _) in mf.replay(q):
            for k in mf.kinds(s.meshes, s.n_triangles):
                kinds_seq[k] += 1
            m = mf.count(s.meshes, s.n_triangles)
            if m in edges_seq:
                edges_seq[m] += 1
            own += m in mf._target_pool(q.options)
        own += n in mf._target_pool(c.options)
    print("record kind        cases  sequence steps")
    for k in mf.KINDS:
        print(f"  {k:16s} {kinds_case[k]:5d}  {kinds_seq[k]:5d}")
    print("visit count        cases  sequence steps")
    for e in mf.EDGES:
        print(f"  {e:16d} {edges_case[e]:5d}  {edges_seq[e]:5d}")
    print("  40 q +- 1 of the run's own mf_group_quads / mf_chunk_quads:", own)
    assert all(kinds_case[k] >= 2 for k in mf.KINDS), "a record kind occurs in fewer than two of the default cases"
    assert all(edges_case[e] >= 1 and edges_case[e] + edges_seq[e] >= 2 for e in mf.EDGES)
    assert own >= 2


# ------------------------------------------------------------------------------------------------ the oracle

def test_default_seeds_skip_at_most_two():
    assert len(SEEDS) == mf.DEFAULT_CASES == len(set(SEEDS)) and not set(SEEDS) & {s for s, _ in mf.SKIPPED_SEEDS} and len(mf.SKIPPED_SEEDS) <= 2
    assert all(isinstance(r, str) and r for _, r in mf.SKIPPED_SEEDS)


def test_oracle_images_hold_no_nan_and_its_triangle_tests_are_the_python_visits(oracle):
    bad = total = 0
    for seed in SEEDS:
        case = mf.case(seed)
        scene, _, W, H, frames = case
        n_visits = len(mf.visits(scene.meshes, scene.n_triangles))
        img = gc.initial_image(case.init, W, H)
        nan = np.zeros((H, W), bool)
        for p in frames:
            cnt, _ = oracle.render(scene, sf.shader_params(scene, p), img, threads=8)
            nan |= np.isnan(img).any(axis=2)
        bad += int(nan.sum())
        total += (H // 8 * 8) * (W // 8 * 8)
        assert cnt["triangle_tests"] == cnt["segments"] * n_visits, f"seed {seed}: oracle {cnt['triangle_tests']} tests, {cnt['segments']} segments x {n_visits} visits"
        # one bounce: the rays do not depend on the records; their number from the same counter under the single record (0, 1)
        p1 = sf.shader_params(scene, frames[-1].replace(max_bounce=1))
        small = np.zeros((8, 16, 4), np.float32)
        one = sf.sc.Scene(scene.spheres, scene.materials, gc.mesh_records([(0, 1)]), scene.vertices, scene.nodes, scene.env)
        rays = oracle.render(one, p1, small, threads=4)[0]["triangle_tests"]
        assert rays == (16 * 8 * p1.samples if scene.n_triangles else 0)
        got = oracle.render(scene, p1, small, threads=4)[0]["triangle_tests"]
        assert got == n_visits * rays, f"seed {seed}: oracle {got} tests, {rays} rays x {n_visits} visits"
    print("NaN pixels", bad, "of", total)
    assert bad == 0


def test_sequence_steps_hold_no_nan(oracle):
    bad = 0
    for seed in SEEDS:
        q = mf.sequence(seed)
        img = np.zeros((q.H, q.W, 4), np.float32)
        for scene, p in mf.replay(q):
            cnt, _ = oracle.render(scene, sf.shader_params(scene, p), img, threads=8)
            assert cnt["triangle_tests"] == cnt["segments"] * mf.count(scene.meshes, scene.n_triangles)
            bad += int(np.isnan(img).any(axis=2).sum())
    assert bad == 0
