"""The scan's item set-up (rt_scan.hpp, scan_solo_kernel: ray fetch, prepared rays, B operands and thresholds per segment) seen through
the counting instances of the kernel (`counters` 1), which no other test launches at shapes this small.

Scene, sizes and bounces are those of tests/test_gpu_scan_setup.py: 8 x 8 (64 rays: one granule, the two upper sets empty), 24 x 8 (a
full granule + 64) and 40 x 24 (seven granules and a half); compaction leaves every later queue ragged inside a set.  Image and final RNG
states are compared with the oracle bit for bit.  The counters say more than the image does: `candidates` is the number of (ray,
triangle) pairs that passed the bf16 broad phase, so it moves as soon as one operand word or one threshold changes -- the exact test
downstream would hide a threshold that became looser.  With `cull` 0 and 1 no queue is binned, the order of every queue is that of the
compaction, and the four tallies must agree across one and two waves per SIMD and across the four work distributions; they must also be
what tests/golden/scan_setup_counters.json holds: the values of the build before the set-up was reworked, recorded on an MI355X.
"""
import json
import os

import numpy as np
import pytest

import golden_cases as gc

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (24, 8), (40, 24)]
WAVES = [1, 2]
DISTS = [1, 2, 3, 4]          # scan_dynamic: static turns, dynamic claims, planned intervals, turns + a claimed tail
CULLS = [0, 1]                # not binned: queue order is that of the compaction
BOUNCES = 4
TALLIES = ("candidates", "culled_tests", "triangle_tests", "segments")
COUNTERS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_setup_counters.json")


def the_scene(rt):
    return gc.scene_two_meshes(rt.scenes)


def the_params(rt):
    sc = rt.scenes
    return sc.params_c2().replace(max_bounce=BOUNCES, frames=1, random=sc.GlibcRand(0).rand())


def case_key(W, H, cull):
    return f"{W}x{H}/cull{cull}"


def render(rt, W, H, options):
    """(image, final RNG states, the four tallies) of one frame with the counting instances"""
    ctx = rt.host.Context(W, H)
    ctx.set_option("kernel", 4)
    ctx.set_option("rng_state", 1)
    ctx.set_option("counters", 1)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.upload_scene(the_scene(rt))
    ctx.render(the_params(rt))
    img, seeds, cnt = ctx.read_image(), ctx.read_rng_state(), ctx.counters()
    ctx.close()
    return img, seeds, {k: cnt[k] for k in TALLIES}


@pytest.fixture(scope="module")
def expected(rt, oracle):
    """(width, height) -> (image, final RNG states) of the oracle; computed once, never written to"""
    out = {}
    scene, p = the_scene(rt), the_params(rt)
    for W, H in SIZES:
        img = np.zeros((H, W, 4), np.float32)
        _, seeds = oracle.render(scene, p, img, threads=4, want_seeds=True)
        img.setflags(write=False)
        seeds.setflags(write=False)
        out[(W, H)] = (img, seeds)
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(COUNTERS_FILE) as f:
        return json.load(f)["cases"]


def assert_same(got, want, what):
    img, seeds = got
    want_img, want_seeds = want
    neq = (img.view(np.uint32) != want_img.view(np.uint32)).any(axis=2)
    assert not neq.any(), f"{what}: {int(neq.sum())} of {neq.size} pixels differ from the oracle, first at {np.argwhere(neq)[:4].tolist()}"
    assert (seeds.reshape(want_seeds.shape) == want_seeds).all(), f"{what}: final PCG4D states differ"


@pytest.mark.parametrize("cull", CULLS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_counting_instances_agree_with_each_other_and_with_the_record(size, cull, rt, expected, recorded):
    """the eight counting instances: same image, same RNG states, same tallies, and the tallies of the recorded build"""
    W, H = size
    want = recorded[case_key(W, H, cull)]
    for waves in WAVES:
        for dist in DISTS:
            what = f"{W}x{H}, cull {cull}, scan_waves {waves}, scan_dynamic {dist}"
            img, seeds, cnt = render(rt, W, H, (("cull", cull), ("scan_waves", waves), ("scan_dynamic", dist)))
            print(what, cnt)
            assert_same((img, seeds), expected[size], what)
            assert cnt == want, f"{what}: tallies {cnt}, recorded {want}"


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_counting_instances_with_chunks_that_span_groups(size, waves, rt, expected):
    """every queue binned, groups of 4 quads under chunks of 3: an item has up to two segments, each with a set-up of its own"""
    W, H = size
    img, seeds, _ = render(rt, W, H, (("mf_group_quads", 4), ("scan_waves", waves), ("cull", 3), ("sort_min_rays", 0)))
    assert_same((img, seeds), expected[size], f"{W}x{H}, groups of 4 quads, scan_waves {waves}")


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_counting_instances_with_several_whole_groups_per_item(size, waves, rt, expected):
    """every queue binned, groups of 2 quads under chunks of 4: chunks that start inside a group, two segments per item"""
    W, H = size
    img, seeds, _ = render(rt, W, H, (("mf_group_quads", 2), ("mf_chunk_quads", 4), ("scan_waves", waves), ("cull", 3), ("sort_min_rays", 0)))
    assert_same((img, seeds), expected[size], f"{W}x{H}, groups of 2 quads, chunks of 4, scan_waves {waves}")
