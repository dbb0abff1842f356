// scan_launch_check.cpp -- the launch policy of the kernel-4 scan (raytracer.glsl_amd/csrc/rt_scan_launch.hpp), on the host alone.
//   (a) Anchors: sixteen launches whose figures were worked out from the arithmetic as it stood inside rtgl_amd.hip before it moved into
//       the header, by an independent restatement.  A mismatch means that the move changed what a launch does.
//   (b) A sweep over devices, meshes, options and queue lengths: every launch fits the capacity computed from the same mesh and options
//       (the buffers ensure_wave_buffers allocates are indexed by what launch() returns; a violation is an out-of-bounds write on the GPU).
// Exit status 0: all of it held.  (tests/test_scan_launch.py builds this with the address and undefined-behaviour sanitizers.)
#include "../../raytracer.glsl_amd/csrc/rt_scan_launch.hpp"

#include <cstdio>

namespace sl = rt_scan_launch;
static int g_failures = 0;

struct Anchor {
    const char *name;
    uint32_t n_cus, n_groups, group_quads, n_tri_visits, mf_chunk_quads; int scan_waves, scan_dynamic, cull; uint64_t items_per_wave;
    uint32_t n0, est, bounce; bool binned;
    // expected
    uint32_t real_quads, W, chunk_quads, chunks; int cull_on, dist; uint32_t blocks; size_t lds; uint32_t cull_blocks, regions, sched_stride, keep_words; size_t keep;
    size_t items_head, items_need, plan_off_tot, plan_off_base, plan_need;      // the layouts, in bytes, of the launches that use one (0: not checked)
};
static const Anchor kAnchors[] = {
    {"C2 camera", 256, 8, 32, 10000, 32, 0, 0, 3, 3, 2073600, 2073600, 0, false, 250, 2, 32, 8, 1, 0, 256, 135168, 4050, 2048, 256, 32, 518912, 0, 0, 0, 0, 0},
    {"C2 binned", 256, 8, 32, 10000, 32, 0, 0, 3, 3, 2073600, 1500000, 1, true, 250, 2, 32, 8, 1, 3, 256, 135168, 2930, 2048, 256, 32, 518912, 0, 0, 0, 0, 0},
    {"C2 late", 256, 8, 32, 10000, 32, 0, 0, 3, 3, 2073600, 60000, 5, false, 250, 2, 16, 16, 0, 0, 256, 98304, 118, 2048, 256, 32, 518912, 0, 0, 0, 0, 0},
    {"C2 planned", 256, 8, 32, 10000, 32, 0, 3, 3, 3, 2073600, 1500000, 1, true, 250, 2, 32, 8, 1, 2, 256, 135168, 2930, 2048, 256, 32, 518912, 0, 0, 518656, 518912, 518984},
    {"C2 one wave", 256, 8, 32, 10000, 32, 1, 2, 2, 3, 2073600, 300000, 3, false, 250, 1, 32, 8, 1, 1, 256, 135168, 586, 2048, 256, 32, 518912, 1024, 519456, 0, 0, 0},
    {"rank of eight", 256, 8, 32, 10000, 32, 0, 0, 3, 3, 259200, 259200, 0, false, 250, 2, 32, 8, 1, 0, 256, 135168, 507, 2048, 256, 32, 65312, 0, 0, 0, 0, 0},
    {"C4 camera", 256, 79, 32, 100000, 32, 0, 0, 3, 3, 2073600, 2073600, 0, false, 2500, 2, 32, 79, 1, 1, 256, 135168, 4050, 2048, 256, 313, 5075608, 1024, 5120540, 0, 0, 0},
    {"C4 late, cull 0", 256, 79, 32, 100000, 32, 0, 0, 0, 3, 2073600, 40000, 6, false, 2500, 2, 32, 79, 0, 1, 256, 135168, 79, 2048, 256, 313, 5075608, 0, 0, 0, 0, 0},
    {"two meshes 8x8", 256, 3, 4, 460, 32, 0, 0, 3, 3, 64, 64, 0, false, 12, 2, 3, 4, 1, 0, 4, 98304, 1, 2048, 256, 2, 32, 0, 0, 0, 0, 0},
    {"two meshes 40x24", 256, 3, 4, 460, 32, 2, 4, 3, 3, 960, 777, 2, true, 12, 2, 3, 4, 1, 3, 4, 98304, 2, 2048, 256, 2, 46, 0, 0, 0, 0, 0},
    {"groups of 2, chunks of 4", 256, 6, 2, 460, 4, 1, 1, 3, 3, 960, 960, 0, false, 12, 1, 4, 3, 1, 0, 6, 98304, 2, 2048, 256, 2, 46, 0, 0, 0, 0, 0},
    {"more chunks than CUs", 256, 280, 1, 11200, 1, 0, 0, 3, 3, 192, 192, 0, false, 280, 2, 1, 280, 1, 0, 280, 98304, 1, 2240, 280, 35, 595, 0, 0, 0, 0, 0},
    {"more chunks than CUs, claims", 256, 280, 1, 11200, 1, 0, 2, 2, 3, 192, 100, 1, false, 280, 2, 1, 280, 1, 1, 35, 98304, 1, 2240, 280, 35, 595, 1280, 3520, 0, 0, 0},
    {"104 CUs", 104, 8, 32, 10000, 32, 0, 0, 3, 3, 2073600, 60000, 5, false, 250, 2, 32, 8, 0, 0, 104, 135168, 118, 832, 104, 32, 518912, 0, 0, 0, 0, 0},
    {"empty queue", 256, 8, 32, 10000, 32, 0, 0, 3, 3, 2073600, 0, 7, false, 250, 2, 4, 63, 0, 0, 63, 98304, 1, 2048, 256, 32, 518912, 0, 0, 0, 0, 0},
    {"padding quads", 256, 2, 32, 100, 32, 0, 0, 1, 1, 4096, 4096, 0, false, 3, 2, 3, 1, 1, 0, 4, 98304, 8, 2048, 256, 1, 48, 0, 0, 0, 0, 0},
};

#define EXPECT_EQ(got, want) do { if ((unsigned long long)(got) != (unsigned long long)(want)) { ++g_failures; \
    std::fprintf(stderr, "%s: %s = %llu, expected %llu\n", a.name, #got, (unsigned long long)(got), (unsigned long long)(want)); } } while (0)

static void anchors()
{
    for (const Anchor &a : kAnchors) {
        const sl::Setup s = {a.n_cus, sl::real_quads(a.n_groups, a.group_quads, a.n_tri_visits), a.mf_chunk_quads, a.scan_waves, a.scan_dynamic, a.cull};
        const sl::Capacity c = sl::capacity(s);
        const sl::Launch L = sl::launch(s, a.items_per_wave, a.n0, a.est, a.bounce, a.binned);
        EXPECT_EQ(s.real_quads, a.real_quads); EXPECT_EQ(L.W, a.W); EXPECT_EQ(L.waves, 4 * a.W); EXPECT_EQ(L.chunk_quads, a.chunk_quads); EXPECT_EQ(L.chunks, a.chunks);
        EXPECT_EQ(L.cull, a.cull_on); EXPECT_EQ(L.dist, a.dist); EXPECT_EQ(L.blocks, a.blocks); EXPECT_EQ(L.lds, a.lds); EXPECT_EQ(L.cull_blocks, a.cull_blocks);
        EXPECT_EQ(c.regions, a.regions); EXPECT_EQ(c.sched_stride, a.sched_stride); EXPECT_EQ(c.keep_words, a.keep_words); EXPECT_EQ(c.keep_count(a.n0), a.keep);
        EXPECT_EQ(L.items_grid_y, a.chunks);
        if (a.items_need) { EXPECT_EQ(L.cull && L.dist == 1, 1); EXPECT_EQ(L.items_head, a.items_head); EXPECT_EQ(L.items_need, a.items_need); }
        if (a.plan_need) { EXPECT_EQ(L.cull && L.dist == 2, 1); EXPECT_EQ(L.plan_off_tot, a.plan_off_tot); EXPECT_EQ(L.plan_off_base, a.plan_off_base); EXPECT_EQ(L.plan_need, a.plan_need); }
        EXPECT_EQ(L.stride, a.n0 / 128 + 1);
        EXPECT_EQ(sl::uses_claim_counters(L.dist), a.dist == 1 || a.dist == 3);
    }
}

#define HOLDS(cond) do { if (!(cond)) { if (++g_failures <= 20) std::fprintf(stderr, "CUs %u, quads %u, mf_chunk_quads %u, scan_waves %d, scan_dynamic %d, cull %d, estimate %u, bounce %u, binned %d: %s\n", \
    s.n_cus, s.real_quads, s.mf_chunk_quads, s.scan_waves, s.scan_dynamic, s.cull, est, bounce, (int)binned, #cond); } } while (0)

static unsigned long long sweep()
{
    static const uint32_t kCus[] = {1, 2, 7, 64, 104, 256, 304}, kMoreQuads[] = {250, 255, 256, 257, 1023, 1024, 2500, 8191, 8192, 8193, 100000};
    static const uint32_t kChunkQuads[] = {1, 3, 4, 5, 8, 31, 32}, kEst[] = {0, 1, 64, 127, 128, 129, 960, 20000, 2073600, 16588800};
    static const struct { uint32_t bounce; bool binned; } kBounce[] = {{0, false}, {1, false}, {1, true}};
    uint32_t quads[69 + sizeof kMoreQuads / sizeof kMoreQuads[0]], n_quads = 0;
    for (uint32_t q = 1; q <= 69; ++q) quads[n_quads++] = q;
    for (uint32_t q : kMoreQuads) quads[n_quads++] = q;
    unsigned long long cases = 0;
    for (uint32_t n_cus : kCus) for (uint32_t qi = 0; qi < n_quads; ++qi) for (uint32_t mf : kChunkQuads)
    for (int scan_waves = 0; scan_waves <= 2; ++scan_waves) for (int scan_dynamic = 0; scan_dynamic <= 4; ++scan_dynamic) for (int cull = 0; cull <= 3; ++cull) {
        const sl::Setup s = {n_cus, quads[qi], mf, scan_waves, scan_dynamic, cull};
        const sl::Capacity c = sl::capacity(s);
        for (uint32_t est : kEst) for (const auto &b : kBounce) {
            const uint32_t bounce = b.bounce; const bool binned = b.binned;
            const sl::Launch L = sl::launch(s, 3, est, est, bounce, binned);
            ++cases;
            HOLDS(L.chunks <= c.sched_stride);
            HOLDS((unsigned long long)L.blocks * 4 * L.W <= c.regions);
            HOLDS(L.waves == 4 * L.W);
            HOLDS(L.chunk_quads >= 1 && L.chunk_quads <= 32);
            HOLDS((unsigned long long)L.chunks * L.chunk_quads >= s.real_quads);
            HOLDS(L.blocks >= 1);
            HOLDS(L.lds <= 160 * 1024);
            HOLDS((L.dist != 0 && L.dist != 3) || L.blocks % L.chunks == 0);
            HOLDS(L.dist >= 0 && L.dist <= 3);
        }
    }
    return cases;
}

int main()
{
    anchors();
    const unsigned long long cases = sweep();
    if (cases != 7056000ull) { ++g_failures; std::fprintf(stderr, "the sweep ran %llu cases, not 7056000\n", cases); }
    if (g_failures) { std::fprintf(stderr, "scan_launch_check: %d expectation(s) failed\n", g_failures); return 1; }
    std::printf("scan_launch_check ok: %d anchors, %llu swept launches\n", (int)(sizeof kAnchors / sizeof kAnchors[0]), cases);
    return 0;
}
