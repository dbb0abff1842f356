"""The environment's tuning variables on the device: every accepted value renders what the oracle renders, bit for bit -- images and the
final PCG4D states (option "rng_state"), no tolerance.  The variables choose other code paths in the same kernels:

    RTGL_AMD_HYBRID_DIV  RTGL_AMD_SORT_OB  RTGL_AMD_SORT_DB  RTGL_AMD_BIN_SPLIT  RTGL_AMD_BIN_UNIT  RTGL_AMD_ITEMS_PER_WAVE
    RTGL_AMD_KD_LAMBDA  RTGL_AMD_ROW_GAMMA  RTGL_AMD_SCHED_FILL  RTGL_AMD_HIST_FILL

They are read when a context is created, a scene uploaded or a frame rendered, so every run here sets them (monkeypatch.setenv) before it
creates its context.  Only values that the CPU checks certify run here (tests/test_scan_items.py, tests/test_bin_plan.py): a pair of
SORT_OB / SORT_DB that rt_bin_plan.hpp refuses is run once, to see it fall back to the defaults and say so.

HYBRID_DIV: the shapes of tests/tuning_knob_cases.py, with "scan_dynamic" 4 (hybrid on every bounce).  On the camera bounce, for 256 CUs,
(blocks per chunk, step, turns of the busiest wave, n_tail), recomputed on the CPU by tests/test_scan_items.py:
    family "chunks" (280 chunks, one block each), scan_waves 1 / 2 -> step 4 / 8
        hybrid_div      1            2            3            4            7            64
        12 granules  (1,4,0,12)   (1,4,2,6)    (1,4,2,4)    (1,4,3,3)    (1,4,3,1)    (1,4,3,0)     step 8: 0, 1, 1, 2, 2, 2 turns
        13 granules  (1,4,0,13)   (1,4,2,6)    (1,4,3,4)    (1,4,3,3)    (1,4,3,1)    (1,4,4,0)     step 8: 0, 1, 2, 2, 2, 2
        25 granules  (1,4,0,25)   (1,4,4,12)   (1,4,5,8)    (1,4,5,6)    (1,4,6,3)    (1,4,7,0)     step 8: 0, 2, 3, 3, 3, 4
        40 granules  (1,4,0,40)   (1,4,5,20)   (1,4,7,13)   (1,4,8,10)   (1,4,9,5)    (1,4,10,0)    step 8: 0, 3, 4, 4, 5, 5
    family "blocks" (12 chunks, 21 blocks each, laid out by XCD), 352 granules
        step 84      (21,84,0,352) (21,84,3,176) (21,84,3,117) (21,84,4,88) (21,84,4,50) (21,84,5,5)
        step 168     (21,168,0,352) (21,168,2,176) (21,168,2,117) (21,168,2,88) (21,168,2,50) (21,168,3,5)
Later bounces have fewer rays and so fewer turns.  These runs cannot force the order of the atomic claims: whether a wave's first claimed
index meets the index of a record it read ahead in its turns is up to the hardware.  The proof that the switch from turns to tail forgets
such records is the model of tests/cpp/scan_items_check.cpp, and that the model would have seen the defect.  What the device adds: with
"cull" 1 and "counters" 1 the four tallies candidates / culled_tests / triangle_tests / segments equal those of fixed turns
("scan_dynamic" 1) -- a granule scanned twice moves them even where the image hides it.

Binning scenes: the rays that leave the mesh start inside its box (the inside cells of the key), those that leave the ground and the
spheres start outside (golden case mesh_env_dof: the camera's too); glass_inside_tir has no mesh and never bins -- the variables must
leave it alone.

The fuzz campaign: TUNING_FUZZ_CASES cases (default 24) from TUNING_FUZZ_SEED (default 0) of the "mixed" family of
tests/scene_fuzz_inputs.py, each with its own option set and a random accepted assignment of all the variables; a failing case prints
its environment."""
import os

import numpy as np
import pytest

import golden_cases as gc
import scene_fuzz_inputs as sf
import tuning_knob_cases as tk
from test_gpu_scene_fuzz import differences, gpu_run, oracle_run

pytestmark = pytest.mark.gpu

TALLIES = ("candidates", "culled_tests", "triangle_tests", "segments")
BIN_OPTIONS = (("kernel", 4), ("cull", 3), ("sort_min_rays", 0))
# every pair rt_bin_plan.hpp accepts (tests/cpp/bin_plan_check.cpp counts the same 19)
ACCEPTED_PAIRS = [(ob, db) for ob in range(2, 6) for db in range(2, 7) if (ob, db) != (5, 2)]
REFUSED_PAIR = (1, 6)

_scenes = {}


def named_scene(rt, name):
    """name -> (key, scene, frames, W, H, init); built once"""
    if name not in _scenes:
        sc = rt.scenes
        if name == "two_meshes_40x24":
            scene, (W, H), init = gc.scene_two_meshes(sc), (40, 24), "zeros"
            frames = gc.frame_sequence(sc, sc.params_c2().replace(use_dof=0, max_bounce=4), 2)
        elif name == "two_meshes_44x28":              # ragged: 40 x 24 is written
            scene, (W, H), init = gc.scene_two_meshes(sc), (44, 28), "ramp"
            frames = gc.frame_sequence(sc, sc.params_c2().replace(max_bounce=4), 2)
        else:                                         # a golden case by name
            case = gc.build_cases(sc)[name]
            scene, (W, H), init, frames = case["scene"](), (case["width"], case["height"]), case["init"], case["frames"]
        _scenes[name] = (("tuning", name), scene, frames, W, H, init)
    return _scenes[name]


def run_differs(rt, oracle, name, options, scene_override=None):
    key, scene, frames, W, H, init = scene_override or named_scene(rt, name)
    want = oracle_run(oracle, key, scene, frames, W, H, init)
    got = gpu_run(rt, scene, frames, W, H, options, init)
    return differences(got, want, W, H), got[2]


def set_env(monkeypatch, env):
    for k in ("HYBRID_DIV", "SORT_OB", "SORT_DB", "BIN_SPLIT", "BIN_UNIT", "ITEMS_PER_WAVE", "KD_LAMBDA", "ROW_GAMMA", "SCHED_FILL", "HIST_FILL"):
        monkeypatch.delenv("RTGL_AMD_" + k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


# ------------------------------------------------------------------------------------------------ RTGL_AMD_HYBRID_DIV

def hybrid_scene(rt, family, size):
    sc = rt.scenes
    key = ("tuning", "hybrid", family, size)
    if key not in _scenes:
        scene = sc.scene_mesh(*tk.CHUNKS_MESH, env_size=16) if family == "chunks" else gc.scene_two_meshes(sc)
        frames = gc.frame_sequence(sc, sc.params_c2().replace(max_bounce=4), 1, seed=size[0])
        _scenes[key] = (key, scene, frames, size[0], size[1], "zeros")
    return _scenes[key]


HYBRID_SHAPES = [("chunks", s) for s in tk.CHUNKS_SIZES] + [("blocks", s) for s in tk.BLOCKS_SIZES]


@pytest.mark.parametrize("waves", tk.SCAN_WAVES)
@pytest.mark.parametrize("family,size", HYBRID_SHAPES, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_hybrid_div_matches_the_oracle_and_the_tallies_of_fixed_turns(family, size, waves, rt, oracle, monkeypatch):
    case = hybrid_scene(rt, family, size)
    assert case[1].n_triangles == (11200 if family == "chunks" else 400)
    base = (("kernel", 4), ("mf_group_quads", 1), ("mf_chunk_quads", 1), ("scan_waves", waves))
    set_env(monkeypatch, {})
    d, fixed = run_differs(rt, oracle, None, base + (("scan_dynamic", 1), ("cull", 1)), case)
    assert not d, f"fixed turns: {d}"
    bad = []
    for div in tk.HYBRID_DIVS:
        set_env(monkeypatch, {"RTGL_AMD_HYBRID_DIV": div})
        d, cnt = run_differs(rt, oracle, None, base + (("scan_dynamic", 4), ("cull", 1)), case)
        moved = [f"{k} {cnt[k]} != {fixed[k]}" for k in TALLIES if cnt[k] != fixed[k]]
        if d or moved:
            bad.append(f"hybrid_div {div} cull 1: {d + moved}")
        d, _ = run_differs(rt, oracle, None, base + (("scan_dynamic", 4), ("cull", 3), ("sort_min_rays", 0)), case)
        if d:
            bad.append(f"hybrid_div {div} cull 3: {d}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ RTGL_AMD_SORT_OB x RTGL_AMD_SORT_DB

BIN_SCENES = ["two_meshes_40x24", "mesh_env_dof", "glass_inside_tir"]


@pytest.mark.parametrize("name", BIN_SCENES)
def test_every_accepted_bin_plan_matches_the_oracle(name, rt, oracle, monkeypatch):
    bad = []
    for ob, db in ACCEPTED_PAIRS:
        set_env(monkeypatch, {"RTGL_AMD_SORT_OB": ob, "RTGL_AMD_SORT_DB": db})
        d, _ = run_differs(rt, oracle, name, BIN_OPTIONS)
        if d:
            bad.append(f"SORT_OB {ob} SORT_DB {db}: {d}")
    assert not bad, "\n".join(bad)


def test_a_refused_bin_plan_renders_as_the_default_and_says_so(rt, oracle, monkeypatch, capfd):
    name = "two_meshes_40x24"
    set_env(monkeypatch, {})
    d, default = run_differs(rt, oracle, name, BIN_OPTIONS)
    assert not d, d
    capfd.readouterr()
    set_env(monkeypatch, {"RTGL_AMD_SORT_OB": REFUSED_PAIR[0], "RTGL_AMD_SORT_DB": REFUSED_PAIR[1]})
    d, cnt = run_differs(rt, oracle, name, BIN_OPTIONS)
    err = capfd.readouterr().err
    assert not d, d
    assert cnt == default                                   # every tally: the same plan ran
    said = [line for line in err.splitlines() if "RTGL_AMD_SORT_OB=1 RTGL_AMD_SORT_DB=6 refused" in line]
    assert len(said) == 1 and "using 4 and 4" in said[0], err


# ------------------------------------------------------------------------------------------------ the other variables

OTHERS = ([("RTGL_AMD_BIN_SPLIT", 0)] + [("RTGL_AMD_BIN_UNIT", v) for v in ("0.5", "8", "64", "1e6")]
          + [("RTGL_AMD_KD_LAMBDA", v) for v in ("0", "0.01", "1", "1e6", "1.1e6", "-1", "nan", "inf")]      # (from 1.1e6 on: refused, the default's order)
          + [("RTGL_AMD_ROW_GAMMA", v) for v in ("0", "1.220703125e-4", "1e-2")] + [("RTGL_AMD_SCHED_FILL", 1), ("RTGL_AMD_HIST_FILL", 1)])
OTHER_SCENES = ["two_meshes_44x28", "mesh_env_dof", "glass_inside_tir"]


@pytest.mark.parametrize("name", OTHER_SCENES)
def test_cell_order_and_fill_variables_match_the_oracle(name, rt, oracle, monkeypatch):
    bad = []
    for var, value in OTHERS:
        set_env(monkeypatch, {var: value})
        d, _ = run_differs(rt, oracle, name, BIN_OPTIONS)
        if d:
            bad.append(f"{var}={value}: {d}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", OTHER_SCENES)
def test_items_per_wave_matches_the_oracle(name, rt, oracle, monkeypatch):
    bad = []
    for v in tk.ITEMS_PER_WAVE:
        set_env(monkeypatch, {"RTGL_AMD_ITEMS_PER_WAVE": v})
        d, _ = run_differs(rt, oracle, name, BIN_OPTIONS)
        if d:
            bad.append(f"ITEMS_PER_WAVE={v}: {d}")
    assert not bad, "\n".join(bad)


def test_items_per_wave_changes_the_chunking_and_nothing_else(rt, oracle, monkeypatch):
    """7,000 triangles = 175 quads in chunks of 32 at 256 x 176 (352 granules): with one item per wave the camera bounce has enough items (6 x
    352 >= 256 x 8) and keeps its 6 chunks of 32 quads, with two it halves them twice (22 chunks of 8), with 8 and 1000 down to 4 quads --
    tests/test_scan_items.py recomputes that through rt_scan_launch.hpp, which is what keeps this case from being vacuous: no counter of
    the library shows the chunking (measured: the four tallies are the same numbers under 6, 22 and 44 chunks -- they are sums over
    (granule, tile) pairs, however the tiles are cut into chunks; `segments` is the oracle's count of path segments).  So the tallies are
    asserted to stay put: an item lost or taken twice by a cut would move them.  The image and the states are the oracle's."""
    sc = rt.scenes
    key = ("tuning", "items_per_wave")
    if key not in _scenes:
        _scenes[key] = (key, sc.scene_mesh(*tk.ITEMS_MESH, env_size=16), gc.frame_sequence(sc, sc.params_c2().replace(max_bounce=3), 1), tk.ITEMS_SIZE[0], tk.ITEMS_SIZE[1], "zeros")
    assert _scenes[key][1].n_triangles == tk.ITEMS_QUADS * 40
    tallies = {}
    for v in tk.ITEMS_PER_WAVE:
        set_env(monkeypatch, {"RTGL_AMD_ITEMS_PER_WAVE": v})
        d, cnt = run_differs(rt, oracle, None, (("kernel", 4), ("cull", 1), ("scan_dynamic", 1)), _scenes[key])
        assert not d, f"ITEMS_PER_WAVE={v}: {d}"
        tallies[v] = {k: cnt[k] for k in TALLIES}
        print("ITEMS_PER_WAVE", v, tallies[v])
    assert all(tallies[v] == tallies[tk.ITEMS_PER_WAVE[0]] for v in tk.ITEMS_PER_WAVE), tallies


# ------------------------------------------------------------------------------------------------ fuzz

def random_environment(seed):
    rng = np.random.default_rng([int(seed), 7717])
    ob, db = ACCEPTED_PAIRS[int(rng.integers(0, len(ACCEPTED_PAIRS)))]
    return {"RTGL_AMD_HYBRID_DIV": int(rng.choice([1, 2, 2, 3, 4, 5, 7, 16, 64])), "RTGL_AMD_SORT_OB": ob, "RTGL_AMD_SORT_DB": db,
            "RTGL_AMD_BIN_SPLIT": int(rng.integers(0, 2)), "RTGL_AMD_BIN_UNIT": str(rng.choice(["0.5", "2", "8", "64", "1e6"])),
            "RTGL_AMD_ITEMS_PER_WAVE": int(rng.choice([1, 2, 3, 8, 1000])), "RTGL_AMD_KD_LAMBDA": str(rng.choice(["0", "0.01", "0.4", "1"])),
            "RTGL_AMD_ROW_GAMMA": str(rng.choice(["0", "1.220703125e-4", "1e-2"])),
            **({"RTGL_AMD_SCHED_FILL": 1} if rng.random() < 0.5 else {}), **({"RTGL_AMD_HIST_FILL": 1} if rng.random() < 0.5 else {})}


def test_random_scenes_options_and_environments_match_the_oracle(rt, oracle, monkeypatch):
    n, start = int(os.environ.get("TUNING_FUZZ_CASES", "24")), int(os.environ.get("TUNING_FUZZ_SEED", "0"))
    seeds = sf.default_seeds("mixed", n, start)
    bad = 0
    for seed in seeds:
        case = sf.case(seed, "mixed")
        scene, _, W, H, frames = case
        env = random_environment(seed)
        set_env(monkeypatch, env)
        d = differences(gpu_run(rt, scene, frames, W, H, case.options, case.init), oracle_run(oracle, ("mixed", seed), scene, frames, W, H, case.init), W, H)
        if d:
            bad += 1
            print("case", seed, dict(case.options), " ".join(f"{k}={v}" for k, v in env.items()), ":", "; ".join(d), "|", W, "x", H, "triangles", scene.n_triangles,
                  "bounces", frames[0].max_bounce, "frames", len(frames), "init", case.init, flush=True)
    print("tuning fuzz cases", len(seeds), "from seed", start, "differing:", bad if bad else "none differs")
    assert bad == 0, f"{bad} of {len(seeds)} cases differ from the oracle (see the lines printed above)"
