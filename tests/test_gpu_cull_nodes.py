"""Packet culling in nodes of 4, 16 or 64 tiles (rt_scan.hpp `packet_cull_kernel`, switch RTGL_AMD_CULL_NODE) on the
device: the images stay bit for bit what the reference shader and the oracle compute, and the node pass only ever adds culled tiles.

The switch is read when the triangles are uploaded, so every context here is created and loaded with the environment set."""
import os

import numpy as np
import pytest

import golden_cases as gc
from test_oracle_golden import CASE_FILES, load_case

pytestmark = pytest.mark.gpu

NODE_SIZES = [4, 16, 64]


def render_case(rt, meta, scene, frames, options=()):
    W, H = meta["width"], meta["height"]
    ctx = rt.host.Context(W, H)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.upload_scene(scene)
    ctx.write_image(gc.initial_image(meta["init"], W, H))
    for p in frames:
        ctx.render(p)
    img = ctx.read_image()
    ctx.close()
    return img


@pytest.mark.parametrize("node", NODE_SIZES)
@pytest.mark.parametrize("path", CASE_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_node_culling_matches_reference_shader_output(path, node, rt, monkeypatch):
    """every golden case with every queue binned and culled (`sort_min_rays` = 0) and small chunks, node culling on"""
    monkeypatch.setenv("RTGL_AMD_CULL_NODE", str(node))
    meta, scene, frames, expected = load_case(path, rt)
    img = render_case(rt, meta, scene, frames, options=(("kernel", 4), ("cull", 3), ("sort_min_rays", 0), ("mf_chunk_quads", 2)))
    neq = (img.view(np.uint32) != expected.view(np.uint32)).any(axis=2)
    assert not neq.any(), f"node {node}: {int(neq.sum())} of {neq.size} pixels differ from the reference shader's output"


@pytest.mark.parametrize("node", NODE_SIZES)
def test_c2_full_frame_with_node_culling_matches_oracle(node, rt, oracle, monkeypatch):
    """the whole C2 frame (1920 x 1080, 8 bounces, 10,000 triangles), every bounce binned and culled: image and final RNG states"""
    monkeypatch.setenv("RTGL_AMD_CULL_NODE", str(node))
    sc = rt.scenes
    cfg = sc.CONFIGS["C2"]
    W, H = cfg["width"], cfg["height"]
    scene = cfg["scene"]()
    ctx = rt.host.Context(W, H)
    ctx.set_option("rng_state", 1)
    ctx.set_option("sort_min_rays", 0)
    ctx.upload_scene(scene)
    p = cfg["params"]().replace(frames=1, random=sc.GlibcRand(0).rand())
    ctx.render(p)
    img, seeds = ctx.read_image(), ctx.read_rng_state()
    ctx.close()
    want = np.zeros_like(img)
    _, want_seeds = oracle.render(scene, p, want, threads=16, want_seeds=True)
    neq = (img.view(np.uint32) != want.view(np.uint32)).any(axis=2)
    assert not neq.any(), f"node {node}: {int(neq.sum())} of {neq.size} pixels differ from the oracle"
    assert (seeds.reshape(H, W, 4) == want_seeds).all()


def camera_bounce(rt, cfg_name, node, monkeypatch):
    """one frame, camera rays only (their queue order is fixed: the culled count is a function of the keep bits alone)"""
    monkeypatch.setenv("RTGL_AMD_CULL_NODE", str(node))
    sc = rt.scenes
    cfg = sc.CONFIGS[cfg_name]
    ctx = rt.host.Context(cfg["width"], cfg["height"])
    ctx.set_option("counters", 1)
    ctx.set_option("cull", 1)
    ctx.upload_scene(cfg["scene"]())
    ctx.render(cfg["params"]().replace(frames=1, max_bounce=1, random=sc.GlibcRand(0).rand()))
    cnt, img = ctx.counters(), ctx.read_image()
    ctx.close()
    return cnt, img


@pytest.mark.parametrize("cfg_name", ["C2", "C4"])
def test_node_culling_culls_at_least_what_the_flat_sweep_culls(cfg_name, rt, monkeypatch):
    """the same queue culled tile by tile and in nodes: a node certificate only adds culled tiles, so the culled tests can only grow
    (and the per-tile evaluation of open nodes is the flat sweep's); the images are identical"""
    flat, img0 = camera_bounce(rt, cfg_name, 0, monkeypatch)
    assert flat["culled_tests"] > 0
    for node in NODE_SIZES:
        cnt, img = camera_bounce(rt, cfg_name, node, monkeypatch)
        assert cnt["culled_tests"] >= flat["culled_tests"], f"node {node}: {cnt['culled_tests']} < flat {flat['culled_tests']}"
        assert cnt["triangle_tests"] == flat["triangle_tests"] and cnt["segments"] == flat["segments"]
        assert (img.view(np.uint32) == img0.view(np.uint32)).all()
