"""Mesh-record fuzz on the device against the CPU oracle: the cases and upload sequences of tests/mesh_fuzz_inputs.py (records that wrap in
32 bits, overlap, descend, leave gaps, start or end past the buffer; visit counts on the edges of the scan's tiles, quads, groups and
chunks), the ids plane against the Python restatement visits(), and record sets that expand to nothing over a buffer that holds vertices.

Comparison rule (tests/test_gpu_scene_fuzz.py): the oracle's images hold no NaN here (tests/test_mesh_fuzz_inputs.py), so every component
has the oracle's bits, no tolerance; the final RNG states over the 8 x 8-aligned footprint and the counters paths, segments, env_lookups
and triangle_tests of the last frame are equal.

In the suite: MESH_FUZZ_CASES cases (default 24) from MESH_FUZZ_SEED (default 0), each on kernels 0, 1 and 2 (wf_chunk 64) and 4 (with
the case's scan options); cases of several frames also run once as one batch of frames."""
import os

import numpy as np
import pytest

import golden_cases as gc
import mesh_fuzz_inputs as mf
import scene_fuzz_inputs as sf
from test_gpu_scene_fuzz import check_case, differences, oracle_run

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "segments", "env_lookups", "triangle_tests")
WRAPS = {"wrap_ones", "wrap_to_zero", "wrap_plus_j", "wrap_far"}


def fuzz_seeds():
    return mf.default_seeds(int(os.environ.get("MESH_FUZZ_CASES", str(mf.DEFAULT_CASES))), int(os.environ.get("MESH_FUZZ_SEED", "0")))


def variants(options):
    return [(("kernel", 0),), (("kernel", 1), ("wf_chunk", 64)), (("kernel", 2), ("wf_chunk", 64)), tuple(options)]


# ------------------------------------------------------------------------------------------------ every case against the oracle

def test_mesh_record_cases_match_the_oracle_on_every_kernel(rt, oracle):
    seeds = fuzz_seeds()
    bad = bad_wrapped = wrapped = 0
    for seed in seeds:
        case = mf.case(seed)
        scene, _, W, H, frames = case
        b = check_case(rt, oracle, ("meshrec", seed), scene, frames, W, H, variants(case.options), case.init, batch_options=case.options, counters=COUNTERS)
        is_wrapped = bool(mf.kinds(scene.meshes, scene.n_triangles) & WRAPS)
        if b:
            print("  seed", seed, "records", [tuple(int(x) for x in r[:2]) for r in scene.meshes], "triangles", scene.n_triangles, "visits", case.target, flush=True)
        bad, wrapped, bad_wrapped = bad + b, wrapped + is_wrapped, bad_wrapped + bool(b and is_wrapped)
    print("mesh-record cases", len(seeds), "with a wrapping record", wrapped, "| differing runs:", bad, "| differing cases with a wrapping record:", bad_wrapped)
    assert bad == 0, f"{bad} runs of {len(seeds)} cases differ from the oracle (see the lines printed above)"


# ------------------------------------------------------------------------------------------------ the ids plane

def duplicate_scene(sc, duplicates_first):
    """the 400-triangle grid and, behind it in the buffer, exact copies of its first 200 triangles under another material id; the copies'
    record comes first or last"""
    s = sc.scene_mesh(20, 10, env_size=16)
    copy = np.array(s.vertices[:600])
    copy[:, 3] = np.where(copy[:, 3] == 5.0, 0.0, 5.0)
    s.vertices = np.concatenate([s.vertices, copy], axis=0)
    s.meshes = gc.mesh_records([(400, 200), (0, 400)] if duplicates_first else [(0, 400), (400, 200), (100, 50)])
    return s


def ids_scenes(sc):
    """name -> (scene, W, H, base FrameParams)"""
    P = sc.params_c2().replace(use_dof=0, frames=1, random=sc.GlibcRand(0).rand())
    out = {"meshrec_" + name: (gc.scene_mesh_records(sc, name), 48, 32, P) for name in gc.mesh_record_sets(400)}
    out["duplicates_first"] = (duplicate_scene(sc, True), 48, 32, P)
    out["duplicates_last"] = (duplicate_scene(sc, False), 48, 32, P)
    with_duplicates = 0
    for seed in mf.default_seeds():
        case = mf.case(seed)
        scene = case[0]
        groups = mf.duplicate_groups(scene.vertices)
        visited = {t for _, t in mf.visits(scene.meshes, scene.n_triangles)}
        if len({groups[t] for t in visited}) < len(visited) and with_duplicates < 6:
            with_duplicates += 1
            out[f"case_{seed}"] = (scene, case[2], case[3], case[4][0])
    assert with_duplicates >= 4
    return out


IDS_NAMES = ["meshrec_" + n for n in gc.mesh_record_sets(400)] + ["duplicates_first", "duplicates_last", "fuzz_cases_with_duplicates"]


@pytest.mark.parametrize("name", IDS_NAMES)
def test_ids_plane_names_the_first_visit(name, rt):
    H_ = rt.host
    every = ids_scenes(rt.scenes)
    picked = {k: v for k, v in every.items() if k.startswith("case_")} if name == "fuzz_cases_with_duplicates" else {name: every[name]}
    tie_seen = False
    for key, (scene, W, H, p) in picked.items():
        n = scene.n_triangles
        order = mf.visits(scene.meshes, n)
        groups = mf.duplicate_groups(scene.vertices)
        first_of, listed = {}, set(order)
        for m, t in order:
            first_of.setdefault(groups[t], (m, t))
        p = p.replace(reset_flag=1, samples=1, max_bounce=2)
        planes = {}
        for options in ((("kernel", 0),), (("kernel", 4),)):
            ctx = rt.host.Context(W, H)
            for k, v in options:
                ctx.set_option(k, v)
            ctx.set_aov(H_.AOV_ALL)
            ctx.upload_scene(scene)
            ctx.render(sf.shader_params(scene, p))
            ids = ctx.read_aov(H_.AOV_IDS)[:H // 8 * 8, :W // 8 * 8]
            ctx.close()
            planes[options] = ids
            tri = ids[..., 0] == 2
            if not order:
                assert not tri.any(), f"{key} {dict(options)}: a triangle is reported although the records expand to nothing"
                continue
            pairs = {(int(m), int(t)) for m, t in ids[tri][:, 1:3]}
            for m, t in pairs:
                assert (m, t) in listed, f"{key} {dict(options)}: (mesh {m}, triangle {t}) is reported and never visited"
                assert first_of[groups[t]] == (m, t), f"{key} {dict(options)}: (mesh {m}, triangle {t}) is reported; the first visit of these vertices is {first_of[groups[t]]}"
                tie_seen |= sum(1 for _, t2 in order if groups[t2] == groups[t]) > 1
        a, b = planes.values()
        assert (a == b).all(), f"{key}: the ids of kernel 4 differ from kernel 0's"
    if name in ("duplicates_first", "duplicates_last", "fuzz_cases_with_duplicates", "meshrec_reversed_overlap"):
        assert tie_seen, "no reported triangle is visited twice: the test has no teeth"


# ------------------------------------------------------------------------------------------------ upload sequences

def test_upload_sequences_match_the_oracle_after_every_step_and_a_fresh_context(rt, oracle):
    """one context through the steps of mesh_fuzz_inputs.sequence (new records, new vertices or both; to zero visits and back; to more visits
    than ever before), binned queues and cull records rebuilt each time (sort_min_rays 0, cull 3) -- after every frame the oracle's image,
    RNG states and counters, and the same from a fresh context that starts from the oracle's image of the step before"""
    seeds = fuzz_seeds()
    bad = 0
    for seed in seeds:
        q = mf.sequence(seed)
        ctx = rt.host.Context(q.W, q.H)
        for k, v in q.options + (("rng_state", 1), ("counters", 1)):
            ctx.set_option(k, v)
        ctx.upload_spheres(q.scene.spheres); ctx.upload_materials(q.scene.materials); ctx.upload_nodes(q.scene.nodes); ctx.upload_envmap(q.scene.env)
        img_o = np.zeros((q.H, q.W, 4), np.float32)
        counts = []
        for i, (st, (scene, p)) in enumerate(zip(q.steps, mf.replay(q))):
            before = img_o.copy()
            cnt_o, seeds_o = oracle.render(scene, sf.shader_params(scene, p), img_o, threads=16, want_seeds=True)
            want = (img_o.copy(), seeds_o, cnt_o)
            if st.meshes is not None:
                ctx.upload_meshes(st.meshes)
            if st.vertices is not None:
                ctx.upload_vertices(st.vertices)
            ctx.render(p)
            d = differences((ctx.read_image(), ctx.read_rng_state(), ctx.counters()), want, q.W, q.H, COUNTERS)
            fresh = rt.host.Context(q.W, q.H)
            for k, v in q.options + (("rng_state", 1), ("counters", 1)):
                fresh.set_option(k, v)
            fresh.upload_scene(scene)
            fresh.write_image(before)
            fresh.render(p)
            d2 = differences((fresh.read_image(), fresh.read_rng_state(), fresh.counters()), want, q.W, q.H, COUNTERS)
            fresh.close()
            counts.append(mf.count(scene.meshes, scene.n_triangles))
            for who, dd in (("the sequence's context", d), ("a fresh context", d2)):
                if dd:
                    bad += 1
                    print("sequence", seed, "step", i, st.what, "visits", counts, who, ":", "; ".join(dd), "|", q.W, "x", q.H, dict(q.options), flush=True)
        ctx.close()
    print("upload sequences", len(seeds), "differing frames:", bad)
    assert bad == 0, f"{bad} frames of {len(seeds)} upload sequences differ from the oracle (see the lines printed above)"


# ------------------------------------------------------------------------------------------------ zero visits with vertices present

@pytest.mark.parametrize("name", ["wrap_all_ones", "wrap_to_zero", "wrap_far_start", "no_records"])
def test_records_that_expand_to_nothing_behave_like_a_triangle_free_scene(name, rt, oracle):
    sc = rt.scenes
    W, H = 48, 32
    scene = gc.scene_mesh_records(sc, name)
    assert scene.n_triangles == 400 and mf.visits(scene.meshes, 400) == []
    bare = sc.Scene(spheres=scene.spheres, materials=scene.materials, nodes=scene.nodes, env=scene.env)
    frames = gc.frame_sequence(sc, sc.params_c2().replace(use_dof=0, max_bounce=3), 2)
    want = oracle_run(oracle, ("nothing", name), scene, frames, W, H)
    want_bare = oracle_run(oracle, ("nothing", "bare"), bare, frames, W, H)
    assert (want[0].view(np.uint32) == want_bare[0].view(np.uint32)).all()
    in_use = {}
    for which, s in (("records", scene), ("bare", bare)):
        ctx = rt.host.Context(W, H)
        ctx.set_option("rng_state", 1)
        ctx.set_option("counters", 1)
        ctx.upload_scene(s)
        for p in frames:
            ctx.render(p)
        in_use[which] = ctx.get_option("kernel_in_use")
        d = differences((ctx.read_image(), ctx.read_rng_state(), ctx.counters()), want, W, H, COUNTERS)
        ctx.close()
        assert not d, which + ": " + "; ".join(d)
    assert in_use["records"] == in_use["bare"], "the default kernel choice counts vertices, not visits"
    for options in ((("kernel", 4),), (("kernel", 4), ("cull", 3), ("sort_min_rays", 0)), (("kernel", 4), ("cull", 2), ("scan_dynamic", 2), ("mf_chunk_quads", 1), ("mf_group_quads", 1))):
        ctx = rt.host.Context(W, H)
        for k, v in options + (("rng_state", 1), ("counters", 1)):
            ctx.set_option(k, v)
        ctx.upload_scene(scene)
        for p in frames:
            ctx.render(p)
        assert ctx.get_option("kernel_in_use") == 4
        d = differences((ctx.read_image(), ctx.read_rng_state(), ctx.counters()), want, W, H, COUNTERS)
        ctx.close()
        assert not d, f"{dict(options)}: " + "; ".join(d)
