"""Option "shade_pass" (rtgl_amd.hip, launch_shade; rt_shade_launch.hpp: the rule; rt_wavefront.hpp: shade_kernel, shade_stride_kernel).
1: a shade launch makes ONE pass -- block b takes slots 256 b .. 256 b + 255, a block behind the queue's end leaves at once -- with a
block per 256 slots of queue 0; 0: every launch in grid-stride passes with a grid from the estimate, as before.  The same body runs in
both, so the image is the same bit for bit, and the reference shader's (tests/golden/).

`shade_pass_launches` (read-only) counts the launches of a context that took the one-pass kernel.  Every test here checks it against
the number of shade launches the frames make (sets of launches x samples x bounces, less the lean camera launches, which are
shade_camera_kernel's), so that a fallback cannot pass for the new path or the other way round.  At these sizes the rule takes one pass
for every launch: the estimate is at least min(n0, 2048) and n0 at most 32,768, far inside one block in 64.

What the one-pass form can get wrong, and the case that would show it:
  * a last block that is partly valid: every bounce behind the first of every case (a queue's length is whatever survived), and a
    72 x 40 image whose queue 0 is 11.25 blocks (c1_ragged_70x53 dispatches 64 x 48 pixels = 12 blocks exactly);
  * the binning and the plain instance: `sort_min_rays` 0 and the default, with one and two scan waves per SIMD;
  * a queue far shorter than the grid, almost every block empty: env_disabled_background, and the bounces behind a camera bounce that
    hits nothing (the stale-estimate test's first scene);
  * no launch at all, several samples per frame, a batch of two frames (n0 = 2 x n0_frame), the first-hit planes (kAov), the work
    counters (kCount: `segments` is added by block 0, `env_lookups` by every thread);
  * a grid that does not cover the queue: an estimate left by another scene (test_estimate_of_another_scene).
"""
import os

import numpy as np
import pytest

import golden_cases as gc
from test_oracle_golden import GOLDEN_DIR, load_case

pytestmark = pytest.mark.gpu

MESH_CASES = ["mesh_env_dof", "mesh_two_meshes_overlap", "mesh_stacked_duplicates"]
OTHER_CASES = ["c1_ragged_70x53", "env_disabled_background", "zero_bounces_three_samples", "mesh_three_samples"]


@pytest.fixture(scope="module")
def cases(rt):
    """name -> (meta, scene, frames, expected image); loaded once, never written to"""
    out = {}
    for name in MESH_CASES + OTHER_CASES + ["env_noise_cube"]:
        meta, scene, frames, expected = load_case(os.path.join(GOLDEN_DIR, name + ".npz"), rt)
        expected.setflags(write=False)
        out[name] = (meta, scene, frames, expected)
    return out


def shade_launches(frames, sets, lean_frames):
    """shade_kernel / shade_stride_kernel launches of `sets` sets of launches: one per sample and bounce, less the lean camera launches"""
    p = frames[0]
    return sets * int(p.samples) * int(p.max_bounce) - lean_frames


def render(rt, case, options, sync=True, counters=False):
    """-> (image, shade_pass_launches, camera_lean_frames, counters or None)"""
    meta, scene, frames, _ = case
    W, H = meta["width"], meta["height"]
    ctx = rt.host.Context(W, H)
    ctx.set_option("kernel", 4)
    for k, v in options:
        ctx.set_option(k, v)
    if counters:
        ctx.set_option("counters", 1)
    ctx.upload_scene(scene)
    ctx.write_image(gc.initial_image(meta["init"], W, H))
    work = None
    for p in frames:
        ctx.render(p, sync=sync)
        if counters:
            c = ctx.counters()
            work = c if work is None else {k: work[k] + c[k] for k in c}
    img = ctx.read_image()
    out = (img, ctx.get_option("shade_pass_launches"), ctx.get_option("camera_lean_frames"), work)
    ctx.close()
    return out


def assert_golden(img, expected, what):
    neq = (img.view(np.uint32) != expected.view(np.uint32)).any(axis=2)
    assert not neq.any(), f"{what}: {int(neq.sum())} of {neq.size} pixels differ from the reference shader's output, first at {np.argwhere(neq)[:4].tolist()}"


def both_arms(rt, case, options, what, sets=None, **kw):
    """renders with shade_pass 0 and 1, checks the counter of each arm and that the two images are the same bits; -> the two results"""
    frames = case[2]
    sets = len(frames) if sets is None else sets
    res = []
    for arm in (0, 1):
        r = render(rt, case, tuple(options) + (("shade_pass", arm),), **kw)
        want = shade_launches(frames, sets, r[2]) if arm else 0
        assert r[1] == want, f"{what}, shade_pass {arm}: {r[1]} one-pass launches, expected {want} ({r[2]} lean frames)"
        res.append(r)
    assert np.array_equal(res[0][0].view(np.uint32), res[1][0].view(np.uint32)), f"{what}: the two arms differ"
    return res


def test_option_round_trip(rt):
    ctx = rt.host.Context(16, 16)
    assert ctx.get_option("shade_pass") == 1
    for v in (0, 1):
        ctx.set_option("shade_pass", v)
        assert ctx.get_option("shade_pass") == v
    for v in (-1, 2):
        with pytest.raises(rt.host.RtglError):
            ctx.set_option("shade_pass", v)
    assert ctx.get_option("shade_pass") == 1
    assert ctx.get_option("shade_pass_launches") == 0
    with pytest.raises(rt.host.RtglError):
        ctx.set_option("shade_pass_launches", 0)
    ctx.close()


@pytest.mark.parametrize("name", MESH_CASES)
def test_mesh_cases_binned_and_plain(name, rt, cases):
    case = cases[name]
    for waves in (1, 2):
        for sort_min in (0, None):
            options = (("scan_waves", waves),) + ((("sort_min_rays", sort_min),) if sort_min is not None else ())
            what = f"{name}, scan_waves {waves}, sort_min_rays {sort_min}"
            for r in both_arms(rt, case, options, what):
                assert_golden(r[0], case[3], what)


@pytest.mark.parametrize("name", OTHER_CASES)
def test_ragged_shrinking_no_launch_and_samples(name, rt, cases):
    case = cases[name]
    for r in both_arms(rt, case, (), name):
        assert_golden(r[0], case[3], name)
    if name == "zero_bounces_three_samples":
        assert shade_launches(case[2], len(case[2]), 0) == 0


def test_queue_zero_ends_inside_a_block(rt, cases, oracle):
    """72 x 40 = 2,880 slots = 11.25 blocks; against the oracle"""
    meta, scene, frames, _ = cases["mesh_env_dof"]
    W, H = 72, 40
    assert (W * H) % 256 != 0 and W % 8 == 0 and H % 8 == 0
    case = (dict(meta, width=W, height=H), scene, frames, None)
    want = gc.initial_image(meta["init"], W, H).copy()
    for p in frames:
        oracle.render(scene, p, want, threads=8)
    for sort_min in (0, None):
        options = (("sort_min_rays", sort_min),) if sort_min is not None else ()
        for r in both_arms(rt, case, options, f"72x40, sort_min_rays {sort_min}"):
            assert np.array_equal(r[0].view(np.uint32), want.view(np.uint32)), f"72x40, sort_min_rays {sort_min}: differs from the oracle"


def test_frame_batch_of_two(rt, cases):
    """n0 = 2 x n0_frame; the frame index rides in the top bits of the pixel word"""
    case = cases["mesh_env_dof"]
    assert len(case[2]) == 2
    for sort_min in (0, None):
        options = (("frame_batch", 2),) + ((("sort_min_rays", sort_min),) if sort_min is not None else ())
        for r in both_arms(rt, case, options, f"frame_batch 2, sort_min_rays {sort_min}", sets=1, sync=False):
            assert r[2] == 0
            assert_golden(r[0], case[3], "frame_batch 2")


@pytest.mark.parametrize("sort_min", [0, None])
def test_first_hit_planes_and_counters(sort_min, rt, cases):
    """the kAov and kCount instances; the work counters do not depend on the form of the launch"""
    case = cases["mesh_env_dof"]
    options = (("aov", 15),) + ((("sort_min_rays", sort_min),) if sort_min is not None else ())
    off, on = both_arms(rt, case, options, f"aov 15 + counters, sort_min_rays {sort_min}", counters=True)
    for r in (off, on):
        assert_golden(r[0], case[3], "aov 15 + counters")
    for k in ("paths", "segments", "env_lookups"):
        assert off[3][k] == on[3][k] and on[3][k] > 0, f"{k}: {off[3][k]} (shade_pass 0) against {on[3][k]} (shade_pass 1)"
    plain = both_arms(rt, case, options[1:], f"counters, sort_min_rays {sort_min}", counters=True)
    for k in ("paths", "segments", "env_lookups"):
        assert plain[0][3][k] == plain[1][3][k] == on[3][k], k


def test_estimate_of_another_scene(rt, cases):
    """The ray counts of a finished frame size the next frames' grids, and they outlive upload_scene.  First scene: a cube map and
    nothing else, so every camera ray leaves at bounce 0 and the estimate for every later bounce is its floor, 2,048 rays = 8 blocks.
    Then mesh_env_dof on the same context, its frames submitted back to back: its queues behind the camera bounce are longer than
    that (checked below from its work counters), so a one-pass grid from the estimate would leave rays unshaded.  The grid comes from
    n0 and the image is the golden one; the stride form does not care."""
    meta, scene, frames, expected = cases["mesh_env_dof"]
    W, H = meta["width"], meta["height"]
    empty_meta, empty_scene, _, _ = cases["env_noise_cube"]
    assert (empty_meta["width"], empty_meta["height"]) == (W, H)
    n0, bounces = W * H, int(frames[0].max_bounce)
    # the inputs do what the test needs: the first scene leaves counts of 0 behind the camera bounce, so the estimate is 0 + 0 + 2,048 rays
    # and a grid from it covers slots 0 .. 2,047.  `segments` is the sum of the queue lengths over the bounces and the queues only get
    # shorter, so bounce 1 of mesh_env_dof holds at least (segments - n0) / (bounces - 1) rays: more than 2,048
    segments = render(rt, cases["mesh_env_dof"], (), counters=True)[3]["segments"] / len(frames)
    assert (segments - n0) / (bounces - 1) > 2048, f"{segments} segments per frame of {n0} pixels"
    first = gc.frame_sequence(rt.scenes, frames[0].replace(frames=1, reset_flag=0), 3)
    for arm in (0, 1):
        ctx = rt.host.Context(W, H)
        ctx.set_option("kernel", 4)
        ctx.set_option("shade_pass", arm)
        ctx.upload_scene(empty_scene)
        for p in first:
            ctx.render(p)                                   # synchronous: the counts of a frame are there when the next one is enqueued
        before = ctx.get_option("shade_pass_launches")
        ctx.upload_scene(scene)
        ctx.write_image(gc.initial_image(meta["init"], W, H))
        for p in frames:
            ctx.render(p, sync=False)
        img = ctx.read_image()
        launches = ctx.get_option("shade_pass_launches") - before
        lean = ctx.get_option("camera_lean_frames")
        ctx.close()
        assert launches == (len(frames) * bounces - lean if arm else 0), f"shade_pass {arm}: {launches} one-pass launches"
        assert_golden(img, expected, f"stale estimate, shade_pass {arm}")
