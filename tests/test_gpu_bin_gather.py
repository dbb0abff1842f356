"""Ray binning's move (rt_wavefront.hpp, sort_place_kernel; rt_scan.hpp, packet_cull_kernel's gather; switch RTGL_AMD_SORT_MOVE) on the
device.  Both moves put every ray at the same slot of the binned queue, and queue order never shows in a result, so the images stay bit
for bit what the reference shader and the oracle compute, under the gather (1, default) as under the scatter (0).

The switch is read when a context is created, so every context here is created with the environment set."""
import os

import numpy as np
import pytest

import golden_cases as gc
from test_oracle_golden import CASE_FILES, load_case

pytestmark = pytest.mark.gpu

MOVES = [0, 1]


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


def render_cfg(rt, cfg_name, frames=1, options=(), batch=1):
    sc = rt.scenes
    cfg = sc.CONFIGS[cfg_name]
    scene = cfg["scene"]()
    ctx = rt.host.Context(cfg["width"], cfg["height"])
    for k, v in options:
        ctx.set_option(k, v)
    if batch > 1:
        ctx.set_option("frame_batch", batch)
    ctx.upload_scene(scene)
    g = sc.GlibcRand(0)
    plist = []
    for f in range(1, frames + 1):
        p = cfg["params"]().replace(frames=f, random=g.rand())
        ctx.render(p, sync=batch == 1)
        plist.append(p)
    img = ctx.read_image()
    seeds = ctx.read_rng_state() if dict(options).get("rng_state") else None
    cnt = ctx.counters() if dict(options).get("counters") else None
    ctx.close()
    return img, seeds, cnt, scene, plist


@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("path", CASE_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_every_queue_binned_matches_reference_shader_output(path, move, rt, monkeypatch):
    """every golden case with every queue binned and culled (`sort_min_rays` = 0) and small chunks"""
    monkeypatch.setenv("RTGL_AMD_SORT_MOVE", str(move))
    meta, scene, frames, expected = load_case(path, rt)
    img = render_case(rt, meta, scene, frames, options=(("kernel", 4), ("cull", 3), ("sort_min_rays", 0), ("mf_chunk_quads", 2)))
    neq = (img.view(np.uint32) != expected.view(np.uint32)).any(axis=2)
    assert not neq.any(), f"move {move}: {int(neq.sum())} of {neq.size} pixels differ from the reference shader's output"


@pytest.fixture(scope="module")
def c2_oracle_frame(rt, oracle):
    sc = rt.scenes
    cfg = sc.CONFIGS["C2"]
    scene = cfg["scene"]()
    p = cfg["params"]().replace(frames=1, random=sc.GlibcRand(0).rand())
    want = np.zeros((cfg["height"], cfg["width"], 4), np.float32)
    _, want_seeds = oracle.render(scene, p, want, threads=16, want_seeds=True)
    return want, want_seeds


@pytest.mark.parametrize("node", [0, 16])
@pytest.mark.parametrize("move", MOVES)
def test_c2_full_frame_matches_oracle(move, node, c2_oracle_frame, rt, monkeypatch):
    """the whole C2 frame (1920 x 1080, 8 bounces, 10,000 triangles), every bounce binned and culled, packet culling tile by tile and in
    nodes of 16: image and final RNG states"""
    monkeypatch.setenv("RTGL_AMD_SORT_MOVE", str(move))
    monkeypatch.setenv("RTGL_AMD_CULL_NODE", str(node))
    img, seeds, _, _, _ = render_cfg(rt, "C2", options=(("rng_state", 1), ("sort_min_rays", 0)))
    want, want_seeds = c2_oracle_frame
    neq = (img.view(np.uint32) != want.view(np.uint32)).any(axis=2)
    assert not neq.any(), f"move {move}, node {node}: {int(neq.sum())} of {neq.size} pixels differ from the oracle"
    assert (seeds.reshape(want_seeds.shape) == want_seeds).all()


@pytest.mark.parametrize("move", MOVES)
def test_c2_batch_of_eight_frames_equals_frame_by_frame(move, rt, monkeypatch):
    """option "frame_batch" = 8: one set of launches for 16.6 M camera rays, the binned queues eight frames long"""
    monkeypatch.setenv("RTGL_AMD_SORT_MOVE", str(move))
    ref = render_cfg(rt, "C2", frames=8)[0]
    got = render_cfg(rt, "C2", frames=8, batch=8)[0]
    assert (ref.view(np.uint32) == got.view(np.uint32)).all()


def test_gather_culls_what_the_scatter_culls(rt, monkeypatch):
    """The two moves fill the binned queues in the same order up to the ranks inside a bin, which come from atomics: the share of a C2
    frame's tests that packet culling spares the scan stays within one point, and the images are identical."""
    res = {}
    for move in MOVES:
        monkeypatch.setenv("RTGL_AMD_SORT_MOVE", str(move))
        img, _, cnt, _, _ = render_cfg(rt, "C2", frames=2, options=(("kernel", 4), ("counters", 1)))
        res[move] = (img, cnt["culled_tests"] / cnt["triangle_tests"], cnt)
    (img0, share0, cnt0), (img1, share1, cnt1) = res[0], res[1]
    assert share0 > 0.5 and abs(share1 - share0) <= 0.01, f"culled share: scatter {share0:.4f}, gather {share1:.4f}"
    assert cnt0["triangle_tests"] == cnt1["triangle_tests"] and cnt0["segments"] == cnt1["segments"]
    assert (img0.view(np.uint32) == img1.view(np.uint32)).all()
