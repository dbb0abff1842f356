"""Option "camera_lean" (rtgl_amd.hip, launch_wavefront; rt_wavefront.hpp, generate_rays_kernel and shade_camera_kernel): on a frame
whose camera-ray bounce is culled from keep bits an earlier frame left (`d_keep0`), ray generation stores only what the scan reads
-- `a`, `b`, the hit key -- and the shade launch of bounce 0 rebuilds every camera ray from its slot instead of loading it.  The ray is a pure function of the uniforms and the slot, rebuilt with ray
generation's own instructions, so the image is the one the full queue gives, bit for bit, and the reference shader's (tests/golden/).

`camera_lean_frames` (read-only) counts the frames of a context that took the lean form: every test here checks it, so that a
fallback cannot pass for the lean path or the other way round.  (Skipping the granules whose row of keep bits is clear was built and
measured, and left out with its buffer, kernel and read-only option: DESIGN.md 9 item 6.  The test that both kinds of granule occur
went with it.)

Cases (tests/golden_cases.py), two frames each -- frame 1 builds the bits, frame 2 is lean: depth of field on and off, two meshes, 60
coincident triangles per ray, no cube map, a moved camera, a wide aperture.  Each with one and two scan waves per SIMD, and with the
binning instance of the shade kernel (`sort_min_rays` 0) and the plain one (the default at these sizes).  The fallbacks: several
samples per pixel, no bounces, no triangles (and a ragged size), a batch of two frames, the first-hit planes.
"""
import os

import numpy as np
import pytest

import golden_cases as gc
from test_oracle_golden import GOLDEN_DIR, load_case

pytestmark = pytest.mark.gpu

LEAN_CASES = ["mesh_env_dof", "mesh_two_meshes_overlap", "mesh_stacked_duplicates", "env_disabled_background", "camera_moved", "dof_wide_c5"]
FALLBACK_CASES = ["mesh_three_samples", "zero_bounces_three_samples", "c1_ragged_70x53"]


@pytest.fixture(scope="module")
def cases(rt):
    """name -> (meta, scene, frames, expected image); loaded once, never written to"""
    out = {}
    for name in LEAN_CASES + FALLBACK_CASES:
        meta, scene, frames, expected = load_case(os.path.join(GOLDEN_DIR, name + ".npz"), rt)
        expected.setflags(write=False)
        out[name] = (meta, scene, frames, expected)
    return out


def render(rt, case, options, sync=True, **tiling):
    """-> (image, camera_lean_frames); sync=False: the frames are submitted back to back (a context that batches holds a frame back
    only until something else is asked of it)"""
    meta, scene, frames, _ = case
    W, H = meta["width"], meta["height"]
    ctx = rt.host.Context(W, H, **tiling)
    ctx.set_option("kernel", 4)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.upload_scene(scene)
    if not tiling:
        ctx.write_image(gc.initial_image(meta["init"], W, H))
    for p in frames:
        ctx.render(p, sync=sync)
    img = ctx.read_image()
    lean_frames = ctx.get_option("camera_lean_frames")
    ctx.close()
    return img, lean_frames


def assert_golden(img, expected, what):
    neq = (img.view(np.uint32) != expected.view(np.uint32)).any(axis=2)
    assert not neq.any(), f"{what}: {int(neq.sum())} of {neq.size} pixels differ from the reference shader's output, first at {np.argwhere(neq)[:4].tolist()}"


def test_option_round_trip(rt):
    ctx = rt.host.Context(16, 16)
    assert ctx.get_option("camera_lean") == 1
    for v in (0, 1):
        ctx.set_option("camera_lean", v)
        assert ctx.get_option("camera_lean") == v
    with pytest.raises(rt.host.RtglError):
        ctx.set_option("camera_lean", 2)
    assert ctx.get_option("camera_lean_frames") == 0
    ctx.close()


@pytest.mark.parametrize("name", LEAN_CASES)
def test_second_frame_is_lean_and_golden(name, rt, cases):
    case = cases[name]
    assert len(case[2]) == 2
    first = None
    for waves in (1, 2):
        for sort_min in (0, None):
            base = (("scan_waves", waves),) + ((("sort_min_rays", sort_min),) if sort_min is not None else ())
            for lean in (0, 1):
                what = f"{name}, scan_waves {waves}, sort_min_rays {sort_min}, camera_lean {lean}"
                img, lean_frames = render(rt, case, base + (("camera_lean", lean),))
                assert lean_frames == lean, f"{what}: {lean_frames} lean frames"
                if first is None:
                    first = img
                assert np.array_equal(img.view(np.uint32), first.view(np.uint32)), f"{what}: differs from the first render"
                assert_golden(img, case[3], what)


@pytest.mark.parametrize("name", FALLBACK_CASES)
def test_frames_the_lean_form_does_not_cover(name, rt, cases):
    """several samples per pixel; no bounces (the megakernel); no triangles"""
    img, lean_frames = render(rt, cases[name], (("camera_lean", 1),))
    assert lean_frames == 0
    assert_golden(img, cases[name][3], name)


def test_frame_batch_of_two_is_not_lean(rt, cases):
    case = cases["mesh_stacked_duplicates"]
    assert len(case[2]) == 2
    img, lean_frames = render(rt, case, (("camera_lean", 1), ("frame_batch", 2)), sync=False)      # both frames in one set of launches
    assert lean_frames == 0
    assert_golden(img, case[3], "frame_batch 2")


def test_first_hit_planes_are_not_lean(rt, cases):
    case = cases["mesh_env_dof"]
    img, lean_frames = render(rt, case, (("camera_lean", 1), ("aov", 15)))
    assert lean_frames == 0
    assert_golden(img, case[3], "aov 15")


def test_one_context_against_the_oracle_after_every_frame(rt, oracle):
    """Frames that reuse the bits (lean) and frames that rebuild them (as before) in one context: three frames standing, a moved camera,
    depth of field off, a new mesh, an aperture no bound covers.  The image after every frame is the oracle's, the lean frames are
    exactly the frames that reuse bits, and the final image does not depend on the option."""
    sc = rt.scenes
    W, H = 296, 184
    scene_a, scene_b = sc.scene_mesh(36, 18, env_size=16), sc.scene_mesh(20, 28, env_size=16)
    base = sc.params_c2().replace(max_bounce=4)
    stand = dict(camera_aperture=0.5, camera_focal_length=38.0)
    moved = dict(camera_aperture=0.5, camera_focal_length=38.0, camera_position=(2.0, 1.0, -33.0))
    wide = dict(camera_aperture=12.0, camera_focal_length=10.0)                  # aperture above focal / 4: no bits are kept
    # (step, does the frame reuse the bits of the one before)
    steps = [(stand, False), (stand, True), (stand, True), (moved, False), (moved, True), (dict(use_dof=0), False), (dict(use_dof=0), True),
             ("scene_b", None), (dict(camera_aperture=0.001), False), (dict(camera_aperture=0.001), True), (wide, False), (wide, False)]

    def run(lean, check):
        ctx = rt.host.Context(W, H)
        ctx.set_option("camera_lean", lean)
        ctx.upload_scene(scene_a)
        scene = scene_a
        img_o = np.zeros((H, W, 4), np.float32)
        g = sc.GlibcRand(3)
        f = reused = 0
        for step, reuses in steps:
            if step == "scene_b":
                ctx.upload_scene(scene_b); scene = scene_b
                continue
            f += 1
            reused += int(reuses)
            p = base.replace(frames=f, random=g.rand(), **step)
            ctx.render(p)
            assert ctx.get_option("camera_lean_frames") == (reused if lean else 0), f"frame {f} ({step})"
            if check:
                oracle.render(scene, p, img_o, threads=8)
                got = ctx.read_image()
                assert (got.view(np.uint32) == img_o.view(np.uint32)).all(), f"frame {f} ({step}) differs from the oracle"
        img = ctx.read_image()
        ctx.close()
        return img

    a = run(1, True)
    b = run(0, False)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_a_rank_of_two(rt, cases):
    """a tile of a striped image: the slot -> pixel mapping goes through the rank's rows"""
    meta, scene, frames, _ = cases["mesh_env_dof"]
    case = (dict(meta, width=96, height=64), scene, frames, None)
    on, lean_on = render(rt, case, (("camera_lean", 1),), rank=1, world=2, strip_rows=8)
    off, lean_off = render(rt, case, (("camera_lean", 0),), rank=1, world=2, strip_rows=8)
    assert (lean_on, lean_off) == (1, 0)
    assert on.any()
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
