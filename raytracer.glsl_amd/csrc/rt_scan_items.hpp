// Which items a wave of the kernel-4 scan (rt_scan.hpp, scan_solo_kernel) takes of a chunk, as index arithmetic that the host compiler can
// build alone (tests/cpp/scan_items_check.cpp): no HIP in this header; under hipcc the functions are marked for both sides and the kernel
// calls them -- it keeps no second copy.
//   * the hybrid distribution: of every hdiv granules hdiv - 1 are taken in fixed turns, the hdiv-th is claimed from the chunk's counter
//     (the tail).  Turn k and tail index k name granules by DIFFERENT mappings (turn_granule, tail_granule); together they name every granule
//     of [0, n_gran) exactly once.  A wave that leaves its turns for the tail changes numbering: whatever it holds about "item k" in the
//     turn numbering -- the record read ahead, the rays on their way -- says nothing about item k of the tail.
//   * the batch a claim takes, for the dynamic and the hybrid form;
//   * which chunk a block starts on, how many blocks start there and the block's rank among them.
#pragma once
#include <cstdint>
#include <algorithm>

#if defined(__HIPCC__)
#define RT_ITEMS_FN __host__ __device__ inline
#else
#define RT_ITEMS_FN inline
#endif

namespace rt_scan_items {

constexpr uint32_t kNone = 0xFFFFFFFFu;      // no item: the record read ahead, the rays in flight
constexpr uint32_t kXcds = 8u;
constexpr uint32_t kHybridDivMin = 1u, kHybridDivMax = 64u, kHybridDivDefault = 3u;      // what RTGL_AMD_HYBRID_DIV accepts

RT_ITEMS_FN bool hybrid_div_accepted(long v) { return v >= (long)kHybridDivMin && v <= (long)kHybridDivMax; }

// hybrid: every hdiv-th granule is claimed (1: all of them), the hturn = hdiv - 1 before it are taken in turns
RT_ITEMS_FN uint32_t hdiv_of(uint32_t hybrid_div) { return std::max(hybrid_div, 1u); }
RT_ITEMS_FN uint32_t hturn_of(uint32_t hdiv) { return std::max(hdiv - 1u, 1u); }
RT_ITEMS_FN uint32_t n_tail(uint32_t n_gran, uint32_t hdiv) { return n_gran / hdiv; }
RT_ITEMS_FN uint32_t n_turns(uint32_t n_gran, uint32_t hdiv) { return n_gran - n_tail(n_gran, hdiv); }
// the granule of turn k < n_turns and of tail index k < n_tail
RT_ITEMS_FN uint32_t turn_granule(uint32_t k, uint32_t hdiv) { const uint32_t hturn = hturn_of(hdiv); return (k / hturn) * hdiv + k % hturn; }
RT_ITEMS_FN uint32_t tail_granule(uint32_t k, uint32_t hdiv) { return hdiv * k + (hdiv - 1u); }
RT_ITEMS_FN uint32_t hybrid_granule(bool tail, uint32_t k, uint32_t hdiv) { return tail ? tail_granule(k, hdiv) : turn_granule(k, hdiv); }

// Items a claim takes of the `rem` that the claiming wave believes unclaimed.  Dynamic: a quarter of an even share, 1..16; hybrid: half of
// an even share, 1..4 (the tail is short).
RT_ITEMS_FN uint32_t claim_batch_dynamic(uint32_t rem, uint32_t blocks_here, uint32_t waves) { return std::min(std::max(rem / (4u * std::max(blocks_here, 1u) * waves), 1u), 16u); }
RT_ITEMS_FN uint32_t claim_batch_hybrid(uint32_t rem, uint32_t blocks_here, uint32_t waves) { return std::min(std::max(rem / (2u * std::max(blocks_here, 1u) * waves), 1u), 4u); }

// Blocks on chunks.  By XCD (enough blocks): eight consecutive blocks share a chunk; plain: chunk = block mod chunks.
RT_ITEMS_FN bool by_xcd(uint32_t grid, uint32_t n_chunks) { return grid >= kXcds * n_chunks; }
RT_ITEMS_FN uint32_t first_chunk(uint32_t grid, uint32_t block, uint32_t n_chunks) { return by_xcd(grid, n_chunks) ? (block / kXcds) % n_chunks : block % n_chunks; }
// the blocks that start on chunk c
RT_ITEMS_FN uint32_t blocks_on(uint32_t grid, uint32_t c, uint32_t n_chunks)
{
    if (by_xcd(grid, n_chunks)) {
        const uint32_t rest = grid % (kXcds * n_chunks);
        return (grid / (kXcds * n_chunks)) * kXcds + std::min(kXcds, rest > kXcds * c ? rest - kXcds * c : 0u);
    }
    return (grid - c + n_chunks - 1u) / n_chunks;
}
// the rank of a block among the blocks that start on its first chunk
RT_ITEMS_FN uint32_t rank_on(uint32_t grid, uint32_t block, uint32_t n_chunks) { return by_xcd(grid, n_chunks) ? (block / (kXcds * n_chunks)) * kXcds + block % kXcds : block / n_chunks; }

}  // namespace rt_scan_items
