"""The scan's item set-up (rt_scan.hpp, scan_solo_kernel: fetch_rays and the group record) at the boundary between full and ragged
granules.  A granule is 128 consecutive slots of a bounce's ray queue, four sets of 32.  A full granule's rays are fetched by eight
unguarded loads in one round trip; only the queue's last granule, when it is ragged, takes the guarded loads set by set.  Which
granules are full changes from bounce to bounce: compaction leaves the later queues with counts that are no multiple of 32.

Images: 8 x 8 (64 rays: one granule, two of its sets empty), 24 x 8 (192 rays: a full granule + 64) and 40 x 24 (960 rays: seven
granules and a half), 4 bounces, over a 460-visit mesh (two overlapping ranges: 12 quads of 40).  Launches this small cut the chunks
down to 3 quads, so with groups of 4 quads a chunk spans two groups and an item has two segments, each with its own group record;
with groups of 2 and chunks of 4 every item has two whole groups.  Image and final RNG states are compared with the oracle bit for bit.
"""
import numpy as np
import pytest

import golden_cases as gc

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (24, 8), (40, 24)]
WAVES = [1, 2]
DISTS = [1, 2, 3, 4]          # scan_dynamic: static turns, dynamic claims, planned intervals, turns + a claimed tail
BOUNCES = 4


def the_scene(rt):
    return gc.scene_two_meshes(rt.scenes)


def the_params(rt):
    sc = rt.scenes
    return sc.params_c2().replace(max_bounce=BOUNCES, frames=1, random=sc.GlibcRand(0).rand())


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


def render(rt, W, H, options):
    ctx = rt.host.Context(W, H)
    ctx.set_option("kernel", 4)
    ctx.set_option("rng_state", 1)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.upload_scene(the_scene(rt))
    ctx.render(the_params(rt))
    img, seeds = ctx.read_image(), ctx.read_rng_state()
    ctx.close()
    return img, seeds


def assert_same(got, want, what):
    img, seeds = got
    want_img, want_seeds = want
    neq = (img.view(np.uint32) != want_img.view(np.uint32)).any(axis=2)
    assert not neq.any(), f"{what}: {int(neq.sum())} of {neq.size} pixels differ from the oracle, first at {np.argwhere(neq)[:4].tolist()}"
    assert (seeds.reshape(want_seeds.shape) == want_seeds).all(), f"{what}: final PCG4D states differ"


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_scan_variant_on_full_and_ragged_granules(size, waves, dist, rt, expected):
    """one and two waves per SIMD x the four work distributions: the eight shipping instances of the kernel"""
    W, H = size
    got = render(rt, W, H, (("scan_waves", waves), ("scan_dynamic", dist)))
    assert_same(got, expected[size], f"{W}x{H}, scan_waves {waves}, scan_dynamic {dist}")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_binned_culled_queues_with_ragged_tails(size, rt, expected):
    """every queue binned and culled: the rays of a granule come from the sorted queue, the last granule of every bounce is ragged"""
    W, H = size
    got = render(rt, W, H, (("cull", 3), ("sort_min_rays", 0)))
    assert_same(got, expected[size], f"{W}x{H}, every queue binned")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_chunks_that_span_groups(size, rt, expected):
    """groups of 4 quads under chunks of 3: an item has up to two segments, the rays are fetched and the group record read per segment"""
    W, H = size
    got = render(rt, W, H, (("mf_group_quads", 4),))
    assert_same(got, expected[size], f"{W}x{H}, groups of 4 quads")


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_several_whole_groups_per_item(size, waves, rt, expected):
    """groups of 2 quads under chunks of 4, every queue binned: two segments in every item that keeps tiles of both groups"""
    W, H = size
    got = render(rt, W, H, (("mf_group_quads", 2), ("mf_chunk_quads", 4), ("scan_waves", waves), ("cull", 3), ("sort_min_rays", 0)))
    assert_same(got, expected[size], f"{W}x{H}, groups of 2 quads, chunks of 4, scan_waves {waves}")
