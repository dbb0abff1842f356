"""tests/scene_fuzz_inputs.py on the CPU: the generator is deterministic and keeps its conditions, its Python node walk counts exactly the
sphere tests the oracle makes, the library's host-side walk (raytracer.glsl_amd/csrc/rt_node_walk.hpp, built alone with the host compiler
through tests/cpp/node_walk_shim.cpp) equals it, every family exercises what it is there for, and the oracle's NaN share stays under the
caps that keep the GPU comparison rule (tests/test_gpu_scene_fuzz.py: bits where the oracle has a number, any NaN where it has a NaN)
from hiding a failure."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import golden_cases as gc
import scene_fuzz_inputs as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK_SEEDS = range(200)
SMALL = (16, 8)                                        # the size the walks are checked at


def small_frame(case):
    """first frame of the case as one 16 x 8 reset frame with one sample"""
    return sf.shader_params(case[0], case[4][0].replace(samples=1, reset_flag=1, frames=1))


def render_small(oracle, scene, p):
    img = np.zeros((SMALL[1], SMALL[0], 4), np.float32)
    cnt, _ = oracle.render(scene, p, img, threads=4)
    return img, cnt


def scene_bytes(scene):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (scene.spheres, scene.materials, scene.meshes, scene.vertices, scene.nodes)) + \
        (b"" if scene.env is None else scene.env.tobytes())


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """tests/cpp/node_walk_shim.cpp built with the host compiler: no HIP anywhere in what it includes"""
    so = str(tmp_path_factory.mktemp("node_walk") / "node_walk_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "raytracer.glsl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "node_walk_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.node_walk_shim.restype = C.c_longlong
    lib.node_walk_shim.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_ulonglong, C.c_void_p, C.c_ulonglong]

    def run(nodes, n_spheres, max_visits=1 << 20):
        nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12)
        out = np.zeros(min(max_visits, 1 << 21) + 1, np.uint32)
        n = lib.node_walk_shim(nodes.ctypes.data_as(C.c_void_p) if nodes.size else None, nodes.shape[0], n_spheres, max_visits,
                               out.ctypes.data_as(C.c_void_p), out.size)
        return None if n < 0 else [int(x) for x in out[:n]]
    return run


# ------------------------------------------------------------------------------------------------ generator

@pytest.mark.parametrize("family", sf.FAMILIES)
def test_generator_is_deterministic_and_keeps_its_conditions(family):
    odd_sizes = 0
    for seed in range(40):
        a, b = sf.case(seed, family), sf.case(seed, family)
        assert scene_bytes(a[0]) == scene_bytes(b[0]) and a[1:] == b[1:] and a.init == b.init and a.options == b.options
        scene, base, W, H, frames = a
        assert 16 <= W <= 96 and 8 <= H <= 64 and 1 <= len(frames) <= 3
        assert 1 <= scene.spheres.shape[0] <= 24 and 1 <= scene.materials.shape[0] <= 10 and 1 <= scene.nodes.shape[0] <= 12
        assert 0.2 < base.camera_fov < 2.4 and 0 <= base.max_bounce <= 10 and 1 <= base.samples <= 3
        assert (family == "mixed") == (scene.n_triangles > 0) and scene.n_triangles <= 300
        w = sf.walk(scene.nodes)
        assert w.visits <= sf.VISIT_BOUND and w.pops <= sf.POP_CAP
        odd_sizes += bool(W % 8 or H % 8)
    assert odd_sizes > 20
    assert scene_bytes(sf.case(0, family)[0]) != scene_bytes(sf.case(1, family)[0])


def test_default_seeds_skip_the_listed_ones():
    for family in sf.FAMILIES:
        seeds = sf.default_seeds(family)
        assert len(seeds) == sf.DEFAULT_CASES == len(set(seeds)) and not set(seeds) & set(sf.SKIPPED_SEEDS[family])


# ------------------------------------------------------------------------------------------------ the walks

# fixed node records next to the drawn ones: (nodes, n_spheres, the walk as the device reads it)
N = sf.NO_SPHERE
I = sf.INVALID


def _nodes(*recs):
    return sf.sc.make_nodes([((0,) * 3, (0,) * 3) + r for r in recs])


NAMED_WALKS = {
    "wrap_to_below_offset": (_nodes((I, I, 2, 0xFFFFFFFF)), 6, []),
    "wrap_to_zero": (_nodes((I, I, 2, (1 << 32) - 2)), 6, []),
    "wrap_far_offset": (_nodes((I, I, 0xFFFFFFF0, 0x20)), 6, []),
    "wrap_then_sane_child": (_nodes((1, I, 1, 0xFFFFFFFF), (I, I, 4, 2)), 6, [4, 5]),
    "bound_is_n_spheres": (_nodes((I, I, 2, 4)), 6, [2, 3, 4, 5]),
    "bound_inside": (_nodes((I, I, 1, 2)), 6, [1, 2]),
    "one_past": (_nodes((I, I, 4, 3)), 6, [4, 5, N]),
    "far_past_is_one_zero_visit": (_nodes((I, I, 4, 0xFFFFFFF0)), 6, [4, 5, N]),
    "offset_past": (_nodes((I, I, 9, 3)), 6, [N]),
    "largest_bound_without_wrap": (_nodes((I, I, 5, 0xFFFFFFFA)), 6, [5, N]),
    "child_past_the_buffer": (_nodes((7, 1, 0, 1), (I, I, 1, 1)), 6, [0, 1]),
    "both_children_root": (_nodes((0, 0, 0, 1)), 6, None),          # a cycle: 65535 pops, filled in below
    "no_nodes": (np.zeros((0, 12), np.float32), 6, []),
    "no_spheres": (_nodes((I, I, 0, 3)), 0, [N]),
}


@pytest.mark.parametrize("name", sorted(NAMED_WALKS))
def test_named_records_walk_as_written(name, shim):
    nodes, n_spheres, want = NAMED_WALKS[name]
    w = sf.walk(nodes)
    if name == "both_children_root":
        # pop 1 pushes two, every later pop finds the stack short of full by one or two: never empties, stops at the pop cap
        assert w.pops == sf.POP_CAP and w.dropped > 0
        want = [0] * sf.POP_CAP
    assert sf.device_visits(w, n_spheres) == want
    assert shim(nodes, n_spheres) == want


@pytest.mark.parametrize("family", sf.FAMILIES)
def test_python_walk_counts_the_oracles_sphere_tests(family, oracle):
    for seed in WALK_SEEDS:
        case = sf.case(seed, family)
        _, cnt = render_small(oracle, case[0], small_frame(case))
        w = sf.walk(case[0].nodes)
        assert cnt["sphere_tests"] == cnt["segments"] * w.visits, f"{family} seed {seed}: oracle {cnt['sphere_tests']} tests, {cnt['segments']} segments x {w.visits} visits"
        assert len(sf.expand(w)) == w.visits


@pytest.mark.parametrize("family", sf.FAMILIES)
def test_library_walk_equals_the_python_walk(family, shim):
    """the uint32 bound: a (k, 0xFFFFFFFF) record of the wild family visits nothing; a 64-bit bound visits k .. n-1 and the zero sphere"""
    wrapped = 0
    for seed in WALK_SEEDS:
        scene = sf.case(seed, family)[0]
        want = sf.device_visits(sf.walk(scene.nodes), scene.spheres.shape[0])
        assert shim(scene.nodes, scene.spheres.shape[0]) == want, f"{family} seed {seed}"
        wrapped += bool(sf.wrapped_nodes(scene.nodes))
    assert (wrapped > 20) == (family == "wild")


def test_library_walk_reports_too_many_on_every_push(shim):
    cycle = _nodes((1, I, 0, 3), (0, I, 3, 2))           # 65535 pops: 32768 x 3 + 32767 x 2 visits
    total = 32768 * 3 + 32767 * 2
    assert len(shim(cycle, 8, max_visits=total)) == total
    assert shim(cycle, 8, max_visits=total - 1) is None
    # the zero-sphere visit counts too: the parent checked the cap only after a visit inside the buffer
    past = _nodes((I, I, 6, 4))
    assert shim(past, 6, max_visits=1) == [N]
    assert shim(past, 6, max_visits=0) is None
    assert shim(_nodes((I, I, 4, 4)), 6, max_visits=2) is None and shim(_nodes((I, I, 4, 4)), 6, max_visits=3) == [4, 5, N]


# ------------------------------------------------------------------------------------------------ every family has teeth

def _ends_by_total_internal_reflection(oracle, scene, p):
    """some pixel's path stops before max_bounce without a miss: with use_envmap on every miss is counted as one cube-map lookup"""
    if p.max_bounce < 2:
        return False
    p = p.replace(use_envmap=1)
    img = np.zeros((SMALL[1], SMALL[0], 4), np.float32)
    for y in range(SMALL[1]):
        for x in range(SMALL[0]):
            cnt, _ = oracle.render(scene, p, img, rect=(x, y, x + 1, y + 1))
            if cnt["env_lookups"] == 0 and cnt["segments"] < p.max_bounce:
                return True
    return False


@pytest.mark.parametrize("family", sf.FAMILIES)
def test_family_has_teeth(family, oracle):
    types_hit, tir, dropped, duplicate, zero_sphere, wrap_matters = set(), False, False, False, False, False
    for seed in sf.default_seeds(family):
        case = sf.case(seed, family)
        scene, p = case[0], small_frame(case)
        img, _ = render_small(oracle, scene, p)
        mtype = scene.materials[:, 7].view(np.uint32)
        for t in (0, 1, 2, 3, 7):                        # a material is hit where a change of its emission changes the image
            if t not in types_hit and (mtype == t).any():
                m = scene.materials.copy()
                m[mtype == t, 4:7] = 3.0
                other, _ = render_small(oracle, sf.sc.Scene(scene.spheres, m, scene.meshes, scene.vertices, scene.nodes, scene.env), p)
                if (other.view(np.uint32) != img.view(np.uint32)).any():
                    types_hit.add(t)
        tir = tir or _ends_by_total_internal_reflection(oracle, scene, p)
        w = sf.walk(scene.nodes)
        visits = sf.expand(w)
        dropped |= w.dropped > 0
        duplicate |= len(set(visits)) < len(visits)
        zero_sphere |= sf.NO_SPHERE in sf.device_visits(w, scene.spheres.shape[0])
        wrapped = sf.wrapped_nodes(scene.nodes)
        if wrapped and not wrap_matters:                 # the same scene with the counts un-wrapped: up to the end of the sphere buffer
            nodes = scene.nodes.copy()
            u = nodes.view(np.uint32)
            for i in wrapped:
                u[i, 11] = max(scene.spheres.shape[0] - int(u[i, 10]), 0) if u[i, 10] < scene.spheres.shape[0] else 0
            if sf.walk(nodes, sf.VISIT_BOUND) is not None:
                other, _ = render_small(oracle, sf.sc.Scene(scene.spheres, scene.materials, scene.meshes, scene.vertices, nodes, scene.env), p)
                wrap_matters = bool((other.view(np.uint32) != img.view(np.uint32)).any())
    assert types_hit == {0, 1, 2, 3, 7}, f"material types hit: {sorted(types_hit)}"
    assert tir, "no path ends by total internal reflection"
    assert dropped, "no walk drops a push"
    assert duplicate, "no walk visits a sphere twice"
    assert zero_sphere, "no walk visits the zero sphere"
    assert wrap_matters == (family == "wild"), "no wrapped bound empties a leaf that would otherwise be hit"


# ------------------------------------------------------------------------------------------------ NaN conditions

def nan_shares(oracle, family):
    """(NaN pixels, pixels, {seed: share}) over the default seeds: a pixel counts when any component is a NaN after any frame"""
    bad = total = 0
    per_case = {}
    for seed in sf.default_seeds(family):
        case = sf.case(seed, family)
        scene, _, W, H, frames = case
        img = gc.initial_image(case.init, W, H)
        nan = np.zeros((H, W), bool)
        for p in frames:
            oracle.render(scene, sf.shader_params(scene, p), img, threads=8)
            nan |= np.isnan(img).any(axis=2)
        fh, fw = H // 8 * 8, W // 8 * 8
        bad += int(nan.sum())
        total += fh * fw
        per_case[seed] = nan.sum() / (fh * fw)
    return bad, total, per_case


@pytest.mark.parametrize("family", sf.FAMILIES)
def test_nan_share_of_the_oracles_images(family, oracle):
    bad, total, per_case = nan_shares(oracle, family)
    worst = max(per_case.values())
    print(family, "NaN pixels", bad, "of", total, "worst case", worst, {s: round(float(v), 4) for s, v in per_case.items() if v})
    if family == "wild":
        assert worst <= sf.NAN_CAP_CASE and bad <= sf.NAN_CAP_FAMILY * total
    else:
        assert bad == 0
