"""The tail drain of the scan by pairs (rt_scan.hpp, drain_region; rt_drain_pairs.hpp): a wave expands the records of its candidate region
into (ray slot, storage position) pairs in its LDS queue and tests 64 x 4 of them per turn.  narrow_phase_kernel (`narrow_fused` 0) is
the untouched second implementation of the same tests, and the merge is an atomicMin on a (t, visit index) key: with the option on and
off the image is the same, bit for bit, and it is the reference shader's (tests/golden/); the tallies of the counting instances agree.

Scenes (tests/golden_cases.py):
  * `mesh_stacked_duplicates`: 30 copies of one quad, 60 coincident triangles that every ray through the quad survives the broad phase
    for -- full masks, records that carry bits into the next turn, and overflow as soon as a region is capped;
  * `c1_ragged_70x53`: a ray count that is no multiple of 64 or 128;
  * `mesh_7k_bounce8`: late bounces whose regions are nearly empty -- a single short turn, most lanes without a pair;
  * `meshrec_single_triangles_134`: 134 one-triangle mesh records over 400 triangles -- the last tile's padding rows lie behind the
    last triangle, and masks name positions there (the `pos < n_tri_visits` guard and the clamped loads).
Every case runs one and two waves per SIMD and the four work distributions (`scan_dynamic` 1 .. 4) under `cull` 2, as
tests/test_gpu_narrow_fused.py does and for its reasons; the tallies are compared under `cull` 1.

RTGL_DEBUG_CAND_CAP caps a wave's region at that many RECORDS (read when a context sets up its wave buffers: every render here makes a
fresh context); what does not fit is tested inside flush() and must not reach the drain.  1, 63, 64 and 65 are the edges of the record
window's first batch (one record per lane).  The pair list has edges of its own, and the stacked scene reaches them.  Its 60 coincident
triangles are 30 copies each of two triangles: copies have the same bounds, so whatever order the tiles are stored in keeps them
together, and a record covers five consecutive storage positions -- a ray through the quad leaves about twelve records of mask 31, five
pairs each (a run of copies that does not start on a multiple of five splits one of them in two), against a handful of one- and
two-bit records from the grid behind the quad.  The regions of the waves that scan those tiles are runs of full masks, and a region of
C of them holds 5 C pairs, in turns of 256:
  * C = 52: 260 pairs; record 51 holds pairs 255 .. 259: one goes into the first turn, four stay in its mask for the second;
  * C = 141: 705 = 2 x 256 + 193 pairs; the last one is entry 192 of the third turn: lane 0 of the turn's last quarter;
  * C = 256: 1,280 = 5 x 256 pairs; the last one is entry 255 of the fifth turn: lane 63 of the last quarter, and no sixth turn;
  * C = 205: 1,025 = 4 x 256 + 1 pairs; the last one is the first and only pair of a fifth turn.
(5 C = 193, 0, 1 mod 256 <=> C = 141, 0, 205 mod 256, since 5 x 205 = 1 mod 256.)  Regions that mix in shorter masks hit other entries:
the caps move the edges through the population, they do not need every region to look the same.
"""
import os

import numpy as np
import pytest

import golden_cases as gc
from test_oracle_golden import GOLDEN_DIR, load_case

pytestmark = pytest.mark.gpu

SCENES = ["mesh_stacked_duplicates", "c1_ragged_70x53", "mesh_7k_bounce8", "meshrec_single_triangles_134"]
WAVES = [1, 2]
DISTS = [1, 2, 3, 4]
CAPS = [None, 1, 63, 64, 65]
STACKED_CAPS = [52, 141, 205, 256]
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


def check_shipping(rt, case, name, cap):
    for waves in WAVES:
        for dist in DISTS:
            base = (("scan_waves", waves), ("scan_dynamic", dist), ("cull", 2))
            what = f"{name}, region cap {cap}, scan_waves {waves}, scan_dynamic {dist}"
            separate, _ = render(rt, case, base + (("narrow_fused", 0),))
            fused, _ = render(rt, case, base + (("narrow_fused", 1),))
            assert np.array_equal(fused.view(np.uint32), separate.view(np.uint32)), f"{what}: drained by pairs differs from narrow_phase_kernel"
            assert_golden(separate, case[3], what + ", narrow_phase_kernel")
            assert_golden(fused, case[3], what + ", drained by pairs")


@pytest.mark.parametrize("cap", CAPS, ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("name", SCENES)
def test_pairs_and_narrow_phase_give_the_reference_image(name, cap, rt, cases, monkeypatch):
    """the shipping instances: 2 x 4 of them, each with the drain and with the separate launch"""
    set_cap(monkeypatch, cap)
    check_shipping(rt, cases[name], name, cap)


@pytest.mark.parametrize("cap", STACKED_CAPS, ids=lambda c: f"cap{c}")
def test_stacked_scene_at_the_edges_of_the_pair_list(cap, rt, cases, monkeypatch):
    """runs of full masks, capped where the last pair falls on the first / last lane of a turn's last quarter, on the next turn's first
    entry, and where a record straddles two turns (module docstring)"""
    set_cap(monkeypatch, cap)
    check_shipping(rt, cases["mesh_stacked_duplicates"], "mesh_stacked_duplicates", cap)


@pytest.mark.parametrize("cap", [None, 65], ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("name", SCENES)
def test_counting_instances_drain_by_pairs_too(name, cap, rt, cases, monkeypatch):
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
            assert cnt_f == cnt_s, f"{what}: tallies drained by pairs {cnt_f}, narrow_phase_kernel {cnt_s}"
            assert np.array_equal(fused.view(np.uint32), separate.view(np.uint32)), f"{what}: drained by pairs differs from narrow_phase_kernel"
            assert_golden(fused, case[3], what + ", drained by pairs")
