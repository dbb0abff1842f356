"""Option "narrow_fused" (rt_scan.hpp, scan_solo_kernel): a scan wave that has run out of items tests the records of its own candidate
region itself, and narrow_phase_kernel is not launched.  The merge is an atomicMin on a (t, visit index) key, so neither the order of
the exact tests nor who runs them can show: with the option on and off the image is the same, bit for bit, it is the reference
shader's (tests/golden/), and the tallies of the counting instances are the same.

Scenes (tests/golden_cases.py): `mesh_stacked_duplicates` (60 coincident candidates per ray: full regions, and overflow as soon as a
region is capped), `c1_ragged_70x53` (a ray count that is no multiple of 64 or 128) and `mesh_7k_bounce8` (late bounces whose regions
are nearly empty).  Every case runs one and two waves per SIMD and the four work distributions -- "scan_dynamic" 1 static turns,
2 dynamic claims, 3 planned intervals, 4 turns + a claimed tail (include/rtgl_amd.h) -- under `cull` 2, so that the claiming and planned
forms have their item lists and plans on every bounce.  The tallies are compared under `cull` 1 instead: behind the camera-ray bounce the
order of a queue is that of shade's compaction, which differs from run to run, and with it the granules, their keep bits and
`culled_tests` (and `candidates`, since a culled tile's pairs never reach the broad phase); with only the camera rays culled all four
tallies are fixed, as tests/test_gpu_scan_setup_split.py relies on.

RTGL_DEBUG_CAND_CAP caps a wave's region (read when a context sets up its wave buffers: every render here makes a fresh context).
The drain takes 64 x 4 records per turn, four per lane: caps of 1, 63, 64 and 65 put the last record on the first lane, on the last
lane of the first quarter, and on the first lane of the second; what did not fit was tested inside flush() and must not be tested
again (twice would not show in the image -- the merge is idempotent -- but a record skipped at an edge does).
"""
import os

import numpy as np
import pytest

import golden_cases as gc
from test_oracle_golden import GOLDEN_DIR, load_case

pytestmark = pytest.mark.gpu

SCENES = ["mesh_stacked_duplicates", "c1_ragged_70x53", "mesh_7k_bounce8"]
WAVES = [1, 2]
DISTS = [1, 2, 3, 4]
CAPS = [None, 1, 63, 64, 65]
TALLIES = ("candidates", "segments", "triangle_tests", "culled_tests")


@pytest.fixture(scope="module")
def cases(rt):
    """name -> (meta, scene, frames, expected image); loaded once, never written to"""
    out = {}
    for name in SCENES:
        meta, scene, frames, expected = load_case(os.path.join(GOLDEN_DIR, name + ".npz"), rt)
        expected.setflags(write=False)
        out[name] = (meta, scene, frames, expected)
    return out


def render(rt, case, options, counters=False):
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
    for p in frames:
        ctx.render(p)
    img = ctx.read_image()
    cnt = ctx.counters() if counters else None
    ctx.close()
    return img, ({k: cnt[k] for k in TALLIES} if counters else None)


def set_cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("RTGL_DEBUG_CAND_CAP", raising=False)
    else:
        monkeypatch.setenv("RTGL_DEBUG_CAND_CAP", str(cap))


def assert_golden(img, expected, what):
    neq = (img.view(np.uint32) != expected.view(np.uint32)).any(axis=2)
    assert not neq.any(), f"{what}: {int(neq.sum())} of {neq.size} pixels differ from the reference shader's output, first at {np.argwhere(neq)[:4].tolist()}"


def test_option_round_trip(rt):
    ctx = rt.host.Context(16, 16)
    for v in (0, 1):
        ctx.set_option("narrow_fused", v)
        assert ctx.get_option("narrow_fused") == v
    with pytest.raises(rt.host.RtglError):
        ctx.set_option("narrow_fused", 2)
    ctx.close()


@pytest.mark.parametrize("cap", CAPS, ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("name", SCENES)
def test_fused_and_separate_give_the_reference_image(name, cap, rt, cases, monkeypatch):
    """the shipping instances: 2 x 4 of them, each with the drain and with the separate launch"""
    set_cap(monkeypatch, cap)
    case = cases[name]
    for waves in WAVES:
        for dist in DISTS:
            base = (("scan_waves", waves), ("scan_dynamic", dist), ("cull", 2))
            what = f"{name}, region cap {cap}, scan_waves {waves}, scan_dynamic {dist}"
            separate, _ = render(rt, case, base + (("narrow_fused", 0),))
            fused, _ = render(rt, case, base + (("narrow_fused", 1),))
            assert np.array_equal(fused.view(np.uint32), separate.view(np.uint32)), f"{what}: fused differs from separate"
            assert_golden(separate, case[3], what + ", separate")
            assert_golden(fused, case[3], what + ", fused")


@pytest.mark.parametrize("cap", [None, 65], ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("name", SCENES)
def test_counting_instances_drain_too(name, cap, rt, cases, monkeypatch):
    """`counters` 1 selects the counting instances: same image, and the four tallies do not depend on who runs the exact tests"""
    set_cap(monkeypatch, cap)
    case = cases[name]
    for waves in WAVES:
        for dist in DISTS:
            base = (("scan_waves", waves), ("scan_dynamic", dist), ("cull", 1))
            what = f"{name}, region cap {cap}, scan_waves {waves}, scan_dynamic {dist}, counters"
            separate, cnt_s = render(rt, case, base + (("narrow_fused", 0),), counters=True)
            fused, cnt_f = render(rt, case, base + (("narrow_fused", 1),), counters=True)
            print(what, cnt_f)
            assert cnt_f == cnt_s, f"{what}: tallies fused {cnt_f}, separate {cnt_s}"
            assert np.array_equal(fused.view(np.uint32), separate.view(np.uint32)), f"{what}: fused differs from separate"
            assert_golden(fused, case[3], what + ", fused")


@pytest.mark.parametrize("name", SCENES)
def test_default_distribution_with_binned_queues(name, rt, cases):
    """library defaults but every queue binned (`sort_min_rays` 0): the camera-ray bounce in static turns, the binned bounces in
    the hybrid form, packet culling's gather in front of the scan"""
    case = cases[name]
    base = (("cull", 3), ("sort_min_rays", 0))
    separate, _ = render(rt, case, base + (("narrow_fused", 0),))
    fused, _ = render(rt, case, base + (("narrow_fused", 1),))
    assert np.array_equal(fused.view(np.uint32), separate.view(np.uint32))
    assert_golden(fused, case[3], f"{name}, binned queues, fused")


def test_frame_batch_of_two(rt, cases):
    """two frames traced in one set of launches (queues twice as long, one frame's rays behind the other's)"""
    case = cases["mesh_stacked_duplicates"]
    assert len(case[2]) == 2
    separate, _ = render(rt, case, (("frame_batch", 2), ("narrow_fused", 0)))
    fused, _ = render(rt, case, (("frame_batch", 2), ("narrow_fused", 1)))
    assert np.array_equal(fused, separate)
    assert_golden(fused, case[3], "frame_batch 2, fused")
