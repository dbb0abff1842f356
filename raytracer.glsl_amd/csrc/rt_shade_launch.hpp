// Which form of the shade launch a bounce takes (rt_wavefront.hpp: shade_kernel makes one pass, shade_stride_kernel grid-stride passes)
// and with how many blocks, as plain host C++: no HIP in this header, so that the host compiler can build it alone
// (tests/cpp/shade_launch_check.cpp).  Arithmetic only: nothing here allocates, reads the environment or launches.
#pragma once
#include <cstdint>

namespace rt_shade_launch {

constexpr uint32_t kBlockRays = 256;      // (rtgl_amd.hip launches both kernels with 256 threads, one per slot)

inline uint32_t blocks_for(uint32_t rays) { return (uint32_t)(((uint64_t)rays + kBlockRays - 1u) / kBlockRays); }

struct Launch {
    bool one_pass;        // shade_kernel (true) or shade_stride_kernel
    uint32_t blocks;
};

// n0: the slots of queue 0 (B x n0_frame in a batch) -- the one exact bound the host has on a queue: counts[b + 1] <= counts[b] <= n0.
// est: the rays expected in this bounce's queue (estimate_rays: a guess from an earlier frame, possibly of another scene, so NOT a bound).
// bins: this launch bins its survivors, which it does where the next queue is expected to hold at least "sort_min_rays" rays.
// shade_pass: the option of that name -- 0 the stride form everywhere, 1 the rule.
//
// The one-pass form must see a block for every slot that can hold a ray, so its grid comes from n0 and from nothing else.  The stride
// form is correct with any grid >= 1 and takes the estimate's, as it always did.
//
// The rule: one pass where the launch bins, and wherever at least one block in kMaxBlocksPerFull is expected to find rays.  Blocks that
// find none are free as far as they were measured: on the last bounces of C2 (8,100 blocks for queues of 35k to 200k rays, 85 to 98 %
// of them empty) the one-pass launches took 8.0 to 16.0 us where the stride form took 8.5 to 16.6 us (profiles/shade_pass_c2/ab.txt).
// A queue of 1 / 59 of n0 was the emptiest in that measurement; beyond it (a late bounce of a large batch) the stride form stays, whose
// cost does not depend on n0.
constexpr uint32_t kMaxBlocksPerFull = 64;
inline Launch launch(int shade_pass, uint32_t n0, uint32_t est, bool bins)
{
    if (shade_pass != 0 && (bins || (uint64_t)est * kMaxBlocksPerFull >= n0)) return {true, blocks_for(n0)};
    return {false, blocks_for(est)};
}

}      // namespace rt_shade_launch
