"""Scene-content fuzz on the device against the CPU oracle: the families of tests/scene_fuzz_inputs.py (spheres, node graphs, materials, cube
maps, cameras, frame sequences; tame, wild and mixed with triangles), named node records, the first-hit planes and the visit cap.

Comparison rule (that of the temporal tests): where the oracle's component is not a NaN the kernel's has the same bits, no tolerance;
where it is a NaN, any NaN will do.  tests/test_scene_fuzz_inputs.py holds the oracle's NaN share to 0 (tame, mixed) and to 2 % / 25 % per
case (wild), so the rule cannot hide a failure.  The final RNG states over the 8 x 8-aligned footprint and the counters paths, segments
and env_lookups of the last frame are equal.

In the suite: SCENE_FUZZ_CASES cases per family (default 24) from SCENE_FUZZ_SEED (default 0), each on kernels 0, 1, 2 and 4 (mixed:
kernel 4 with random scan options); cases of several frames also run once as one batch of frames (option "frame_batch")."""
import os

import numpy as np
import pytest

import golden_cases as gc
import scene_fuzz_inputs as sf
from test_gpu_aov import oracle_dump

pytestmark = pytest.mark.gpu

KERNELS = (0, 1, 2, 4)
ERR_INVALID = -1
_oracle_cache = {}


def oracle_run(oracle, key, scene, frames, W, H, init="zeros"):
    """the oracle's image, final RNG states and last frame's counters; computed once per key, never modified"""
    if key not in _oracle_cache:
        img = gc.initial_image(init, W, H)
        cnt = seeds = None
        for p in frames:
            cnt, seeds = oracle.render(scene, sf.shader_params(scene, p), img, threads=16, want_seeds=True)
        for a in (img, seeds):
            if a is not None:
                a.setflags(write=False)
        _oracle_cache[key] = (img, seeds, cnt)
    return _oracle_cache[key]


def gpu_run(rt, scene, frames, W, H, options, init="zeros", batch=False):
    ctx = rt.host.Context(W, H)
    for k, v in options:
        ctx.set_option(k, v)
    if batch:
        ctx.set_option("frame_batch", len(frames))
    else:
        ctx.set_option("rng_state", 1)
        ctx.set_option("counters", 1)
    ctx.upload_scene(scene)
    if init != "zeros":
        ctx.write_image(gc.initial_image(init, W, H))
    for p in frames:
        ctx.render(p, sync=not batch)
    img = ctx.read_image()
    seeds, cnt = (None, None) if batch or not frames else (ctx.read_rng_state(), ctx.counters())
    ctx.close()
    return img, seeds, cnt


def differences(got, want, W, H, counters=("paths", "segments", "env_lookups")):
    """[] when `got` equals the oracle's `want` under the module's rule, else what differs"""
    (img_g, seeds_g, cnt_g), (img_o, seeds_o, cnt_o) = got, want
    out = []
    nan = np.isnan(img_o)
    wrong = np.where(nan, ~np.isnan(img_g), img_g.view(np.uint32) != img_o.view(np.uint32)).any(axis=2)
    if wrong.any():
        out.append(f"pixels {int(wrong.sum())} (first {np.argwhere(wrong)[0].tolist()})")
    if seeds_g is not None:
        dh, dw = H // 8 * 8, W // 8 * 8
        s = int((seeds_g[:dh, :dw] != seeds_o[:dh, :dw]).any(axis=-1).sum())
        if s:
            out.append(f"rng states {s}")
        for k in counters:
            if cnt_g[k] != cnt_o[k]:
                out.append(f"{k} {cnt_g[k]} != {cnt_o[k]}")
    return out


def check_case(rt, oracle, key, scene, frames, W, H, variants, init="zeros", batch_options=None, counters=("paths", "segments", "env_lookups")):
    """number of differing runs of one case; one printed line each"""
    want = oracle_run(oracle, key, scene, frames, W, H, init)
    bad = 0
    for options in variants:
        d = differences(gpu_run(rt, scene, frames, W, H, options, init), want, W, H, counters)
        if d:
            bad += 1
            print("case", key, dict(options), ":", "; ".join(d), "|", W, "x", H, "spheres", scene.spheres.shape[0], "nodes", scene.nodes.shape[0],
                  "triangles", scene.n_triangles, "bounces", frames[0].max_bounce, "samples", frames[0].samples, "frames", len(frames), "init", init, flush=True)
    if batch_options is not None and len(frames) > 1:
        d = differences(gpu_run(rt, scene, frames, W, H, batch_options, init, batch=True), want, W, H)
        if d:
            bad += 1
            print("case", key, dict(batch_options), "as one batch of frames:", "; ".join(d), "|", W, "x", H, "frames", len(frames), flush=True)
    return bad


def fuzz_seeds(family):
    n, start = int(os.environ.get("SCENE_FUZZ_CASES", str(sf.DEFAULT_CASES))), int(os.environ.get("SCENE_FUZZ_SEED", "0"))
    return sf.default_seeds(family, n, start)


# ------------------------------------------------------------------------------------------------ fuzz

@pytest.mark.parametrize("family", ["tame", "wild"])
def test_sphere_scenes_match_the_oracle_on_every_kernel(family, rt, oracle):
    seeds = fuzz_seeds(family)
    bad = 0
    for seed in seeds:
        case = sf.case(seed, family)
        scene, _, W, H, frames = case
        bad += check_case(rt, oracle, (family, seed), scene, frames, W, H, [(("kernel", k),) for k in KERNELS], case.init, batch_options=(("kernel", 4),))
    print(family, "cases", len(seeds), "differing runs:", bad)
    assert bad == 0, f"{bad} runs of {len(seeds)} {family} cases differ from the oracle (see the lines printed above)"


def test_mixed_scenes_match_the_oracle_under_random_scan_options(rt, oracle):
    seeds = fuzz_seeds("mixed")
    bad = 0
    for seed in seeds:
        case = sf.case(seed, "mixed")
        scene, _, W, H, frames = case
        bad += check_case(rt, oracle, ("mixed", seed), scene, frames, W, H, [case.options], case.init, batch_options=case.options)
    print("mixed cases", len(seeds), "differing runs:", bad)
    assert bad == 0, f"{bad} runs of {len(seeds)} mixed cases differ from the oracle (see the lines printed above)"


# ------------------------------------------------------------------------------------------------ named node records

I = sf.INVALID
BOX = ((-1e5,) * 3, (1e5,) * 3)


def named_nodes(sc, n):
    """name -> (node records, W, H, max_bounce, what the Python walk must say); n = number of spheres (5: the demo set with its light)"""
    def nodes(*recs):
        return sc.make_nodes([BOX + r for r in recs])
    return {
        "wrapped_bound_empties_a_leaf": (nodes((1, 2, 0, 0), (I, I, 0, 2), (I, I, 2, (1 << 32) - 2)), 24, 16, 5, lambda w: sf.expand(w) == [0, 1]),
        "wrapped_bound_lands_inside_the_buffer": (nodes((1, 2, 0, 0), (I, I, 0, 1), (I, I, 3, 0xFFFFFFFF)), 24, 16, 5, lambda w: sf.expand(w) == [0]),
        "bound_exactly_n_spheres": (nodes((1, 2, 0, 0), (I, I, 0, 2), (I, I, 2, n - 2)), 24, 16, 5, lambda w: sf.expand(w) == [2, 3, 4, 0, 1]),
        "offset_past_the_buffer": (nodes((1, 2, 0, 0), (I, I, 0, n), (I, I, n + 3, 2)), 24, 16, 5, lambda w: sf.device_visits(w, n) == [sf.NO_SPHERE, 0, 1, 2, 3, 4]),
        "child_id_past_the_node_buffer": (nodes((9, 1, 0, 1), (I, I, 1, n - 1)), 24, 16, 5, lambda w: sf.expand(w) == [0, 1, 2, 3, 4] and w.pops == 3),
        "root_with_both_children_0": (nodes((0, 0, 0, 2)), 24, 16, 3, lambda w: w.pops == sf.POP_CAP and w.visits == 2 * sf.POP_CAP),
        "two_node_cycle": (nodes((1, I, 0, 1), (0, I, 2, 1)), 16, 8, 2, lambda w: w.pops == sf.POP_CAP and w.visits == sf.POP_CAP),
        "chain_of_9_drops_pushes": (nodes(*[(i + 1, i + 1, i % n, 1) for i in range(8)] + [(I, I, 0, n)]), 24, 16, 5, lambda w: w.dropped > 0 and w.visits <= sf.VISIT_BOUND),
    }


NAMED = ["wrapped_bound_empties_a_leaf", "wrapped_bound_lands_inside_the_buffer", "bound_exactly_n_spheres", "offset_past_the_buffer",
         "child_id_past_the_node_buffer", "root_with_both_children_0", "two_node_cycle", "chain_of_9_drops_pushes"]


@pytest.mark.parametrize("name", NAMED)
def test_named_node_records(name, rt, oracle):
    sc = rt.scenes
    spheres = sc.demo_spheres(True)
    nodes, W, H, bounces, expected = named_nodes(sc, spheres.shape[0])[name]
    assert expected(sf.walk(nodes)), "the record does not walk as its name says"
    scene = sc.Scene(spheres=spheres, materials=sc.demo_materials(), nodes=nodes)
    frames = gc.frame_sequence(sc, sc.params_c1().replace(max_bounce=bounces), 2)
    bad = check_case(rt, oracle, ("named", name), scene, frames, W, H, [(("kernel", k),) for k in KERNELS])
    assert bad == 0, f"{bad} kernels differ from the oracle (see the lines printed above)"
    full = sc.Scene(spheres=spheres, materials=sc.demo_materials(), nodes=sc.single_leaf(spheres.shape[0]))
    if name in ("wrapped_bound_empties_a_leaf", "wrapped_bound_lands_inside_the_buffer", "root_with_both_children_0", "two_node_cycle"):      # spheres left out
        other = oracle_run(oracle, ("named", "single_leaf", W, H, bounces), full, frames, W, H)
        assert (other[0].view(np.uint32) != _oracle_cache[("named", name)][0].view(np.uint32)).any(), "the record shows what a single leaf shows: no teeth"


def test_envmap_on_without_a_cube_map_renders_the_background(rt, oracle):
    """found by the fuzz as a mistake of the test's: the reference's host uploads u_use_envmap = false while no cube map exists
    (src/renderer.cpp:104-110) and the library does the same; the shader alone, as the oracle restates it, would look up black"""
    sc = rt.scenes
    W, H = 24, 16
    scene = sc.scene_c1()
    frames = gc.frame_sequence(sc, sc.params_c1().replace(use_envmap=1), 2)
    assert check_case(rt, oracle, ("named", "envmap_on_without_a_cube_map"), scene, frames, W, H, [(("kernel", k),) for k in KERNELS]) == 0
    black = np.zeros((H, W, 4), np.float32)
    for p in frames:
        oracle.render(scene, p, black, threads=4)
    assert (black.view(np.uint32) != _oracle_cache[("named", "envmap_on_without_a_cube_map")][0].view(np.uint32)).any(), "no ray misses: no teeth"


# ------------------------------------------------------------------------------------------------ first-hit planes

@pytest.mark.parametrize("seed", sf.default_seeds("tame", 8))
def test_first_hit_planes_on_tame_scenes(seed, rt, oracle):
    H_ = rt.host
    planes = (H_.AOV_ALBEDO, H_.AOV_NORMAL, H_.AOV_POSITION, H_.AOV_IDS)
    scene, _, W, H, frames = sf.case(seed, "tame")
    p = frames[0].replace(reset_flag=1, samples=1, max_bounce=2)
    got = {}
    for kernel in KERNELS:
        ctx = rt.host.Context(W, H)
        ctx.set_option("kernel", kernel)
        ctx.set_aov(H_.AOV_ALL)
        ctx.upload_scene(scene)
        ctx.render(p)
        got[kernel] = {pl: ctx.read_aov(pl) for pl in planes}
        ctx.close()
    for kernel in KERNELS[1:]:
        for pl in planes:
            assert (got[kernel][pl].view(np.uint32) == got[0][pl].view(np.uint32)).all(), f"kernel {kernel}: plane {pl} differs from kernel 0's"
    fh, fw = H // 8 * 8, W // 8 * 8
    pos, ids = got[0][H_.AOV_POSITION][:fh, :fw], got[0][H_.AOV_IDS][:fh, :fw]
    d1 = oracle_dump(oracle, scene, p, W, H, 1)[:fh, :fw]
    traced = ~np.isnan(d1[..., 0])
    kind, obj = ids[..., 0], ids[..., 1]
    assert not (traced & (kind == 0)).any()
    assert (pos[traced][:, :3].view(np.uint32) == np.ascontiguousarray(d1[traced][:, :3]).view(np.uint32)).all(), "position is not the origin of the oracle's next ray"
    # the sphere named is one the walk visits, and among records with the same centre and radius (equal t) the first one visited
    n = scene.spheres.shape[0]
    order = sf.device_visits(sf.walk(scene.nodes), n)
    geometry = [scene.spheres[i, :4].tobytes() for i in range(n)]
    first_of = {}
    for i in order:
        if i != sf.NO_SPHERE:
            first_of.setdefault(geometry[i], i)
    assert (kind[kind != 0] == 1).all()
    for i in np.unique(obj[kind == 1]):
        if i < 0:
            assert sf.NO_SPHERE in order, "the zero sphere is reported but the walk never leaves the buffer"
        else:
            assert i in order and first_of[geometry[i]] == i, f"sphere {i} is reported; its first equal record in walk order is {first_of.get(geometry[i])}"


# ------------------------------------------------------------------------------------------------ visit cap

def test_visit_cap_fails_the_frame_and_a_sane_upload_recovers(rt, oracle):
    sc = rt.scenes
    W, H, n = 24, 16, 17
    spheres = sc.make_spheres([(-16.0 + 2.0 * i, -4.0 + (i % 3), 0.0, 1.0, i % 8) for i in range(n)])
    cycle = sc.make_nodes([BOX + (1, I, 0, n), BOX + (0, I, 0, n)])          # 65535 pops x 17 spheres > 2^20
    assert sf.walk(cycle).visits == sf.POP_CAP * n > 1 << 20
    scene = sc.Scene(spheres=spheres, materials=sc.demo_materials(), nodes=cycle)
    frames = gc.frame_sequence(sc, sc.params_c1(), 1)
    ctx = rt.host.Context(W, H)
    ctx.upload_scene(scene)
    ctx.set_params(frames[0])
    assert ctx.lib.rtgl_render_frame(ctx.h) == ERR_INVALID
    assert b"node buffer expands to more than 2^20 sphere tests per ray" in ctx.lib.rtgl_last_error(ctx.h)
    assert ctx.lib.rtgl_render_frame(ctx.h) == ERR_INVALID, "the refused buffer must stay refused"
    # exactly 2^20 is allowed: 65535 pops cannot reach it exactly, a single leaf can -- not rendered here (a million tests per ray)
    ctx.upload_nodes(sc.single_leaf(n))
    ctx.set_option("rng_state", 1)
    ctx.set_option("counters", 1)
    ctx.render(frames[0])
    got = (ctx.read_image(), ctx.read_rng_state(), ctx.counters())
    ctx.close()
    scene.nodes = sc.single_leaf(n)
    d = differences(got, oracle_run(oracle, ("cap", "sane"), scene, frames, W, H), W, H)
    assert not d, "; ".join(d)
