// shade_launch_check.cpp -- the rule that picks the form of a shade launch (raytracer.glsl_amd/csrc/rt_shade_launch.hpp), on the host alone.
// The one-pass shade_kernel gives block b the slots 256 b .. 256 b + 255 and nothing else, so a grid that does not reach the queue's
// last slot loses rays.  The host knows one exact bound on a queue's length: n0, the slots of queue 0.
//   (a) A one-pass grid covers n0, and is not a block longer than that, for the sizes listed below.
//   (b) The rule never hands the one-pass form a grid taken from the estimate: for every estimate, also one far below or above the queue,
//       a one-pass launch has the grid of (a); and the stride form -- correct with any grid -- keeps the grid of the estimate.
//   (c) "shade_pass" = 0 takes the stride form everywhere.
// Exit status 0: all of it held.  (tests/test_shade_launch.py builds this with the address and undefined-behaviour sanitizers.)
#include "../../raytracer.glsl_amd/csrc/rt_shade_launch.hpp"

#include <cstdio>

namespace sh = rt_shade_launch;
static int g_failures = 0;

#define EXPECT(cond, ...) do { if (!(cond)) { ++g_failures; std::fprintf(stderr, "%s: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } while (0)

int main()
{
    // 70 x 53 is not a multiple of 256; 1920 x 1080; a batch of sixteen 3840 x 2160 frames
    const uint32_t sizes[] = {0u, 1u, 255u, 256u, 257u, 3710u, 2073600u, 16u * 8294400u};
    unsigned one_pass_seen = 0, stride_seen = 0;
    for (const uint32_t n0 : sizes) {
        // (a)
        const uint64_t blocks = sh::blocks_for(n0);
        EXPECT(blocks * sh::kBlockRays >= n0, "n0 %u: %llu blocks", n0, (unsigned long long)blocks);
        EXPECT(blocks == 0 || (blocks - 1) * sh::kBlockRays < n0, "n0 %u: %llu blocks, the last one behind the queue", n0, (unsigned long long)blocks);
        // (b), (c): estimates from nothing to n0, and -- what estimate_rays never returns, but the rule must not depend on that -- above it
        const uint32_t ests[] = {0u, 1u, 255u, 256u, 2048u, n0 / 1000u, n0 / 10u, n0 / 2u, n0 - (n0 ? 1u : 0u), n0, n0 + 1u, n0 + 2048u, 0xFFFFFFFFu};
        for (const uint32_t est : ests)
            for (int bins = 0; bins < 2; ++bins) {
                const sh::Launch on = sh::launch(1, n0, est, bins != 0), off = sh::launch(0, n0, est, bins != 0);
                if (on.one_pass) {
                    ++one_pass_seen;
                    EXPECT(on.blocks == blocks, "n0 %u est %u bins %d: one pass with %u blocks, n0 needs %llu", n0, est, bins, on.blocks, (unsigned long long)blocks);
                    EXPECT((uint64_t)on.blocks * sh::kBlockRays >= n0, "n0 %u est %u bins %d: one pass, %u blocks do not cover queue 0", n0, est, bins, on.blocks);
                } else {
                    ++stride_seen;
                    EXPECT(on.blocks == sh::blocks_for(est), "n0 %u est %u bins %d: stride form with %u blocks", n0, est, bins, on.blocks);
                }
                EXPECT(!off.one_pass, "n0 %u est %u bins %d: shade_pass 0 took one pass", n0, est, bins);
                EXPECT(off.blocks == sh::blocks_for(est), "n0 %u est %u bins %d: shade_pass 0 with %u blocks", n0, est, bins, off.blocks);
            }
        // a queue expected to hold less than one ray per kMaxBlocksPerFull slots stays with the stride form unless the launch bins
        if (n0 >= 2u * sh::kMaxBlocksPerFull) {
            EXPECT(!sh::launch(1, n0, n0 / sh::kMaxBlocksPerFull - 1u, false).one_pass, "n0 %u: one pass for a queue expected all but empty", n0);
            EXPECT(sh::launch(1, n0, n0 / sh::kMaxBlocksPerFull + 1u, false).one_pass, "n0 %u: the stride form for a queue of n0 / %u", n0, sh::kMaxBlocksPerFull);
        }
        // a launch that bins a full queue is the case the one-pass form was built for
        EXPECT(sh::launch(1, n0, n0, true).one_pass, "n0 %u: a binning launch of a full queue did not take one pass", n0);
    }
    EXPECT(one_pass_seen > 0 && stride_seen > 0, "the sweep saw %u one-pass and %u stride launches", one_pass_seen, stride_seen);
    if (g_failures) { std::fprintf(stderr, "%d expectation(s) failed\n", g_failures); return 1; }
    std::printf("shade launch rule: %u one-pass and %u stride launches checked\n", one_pass_seen, stride_seen);
    return 0;
}
