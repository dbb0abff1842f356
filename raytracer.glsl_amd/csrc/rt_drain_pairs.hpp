// How the tail drain of a scan wave (rt_scan.hpp, drain_region) turns the records of its candidate region into (ray slot, storage position)
// pairs, as index arithmetic that the host compiler can build alone (tests/cpp/drain_pairs_check.cpp): no HIP in this header; under hipcc
// the functions are marked for both sides and the kernel calls them -- it keeps no second copy.
//
// A record is (ray slot, first storage position, 5-bit mask); every set bit of the mask is one exact test.  The wave holds a WINDOW of
// 64 x kFly consecutive records in registers -- batch j of a window is one record per lane, record j x 64 + lane of the window -- and
// builds, per TURN, a list of up to kTurnPairs pairs in its LDS queue, which the lanes then test kFly at a time:
//   * the batches are expanded in order, a batch's records in lane order, a record's bits from the lowest up: pair number
//     `fill` + (set bits of the batch's earlier lanes) + (set bits of the record below this one) of the turn;
//   * a pair whose number reaches kTurnPairs does not go into this turn's list: its bit stays in the record's mask, and the record (all of
//     its bits, some, or none) is taken up again by the next turn, which starts with the same window;
//   * a window whose masks are all empty is replaced by the next one (whose records were loaded a turn ahead) IN the turn, so that a
//     turn is short of kTurnPairs pairs only when the region has no more: the turns of a region are ceil(pairs / kTurnPairs), carries
//     force none;
//   * the list lives in entries [0, kTurnPairs) of the wave's queue; a lane with nothing to write writes to the queue's scratch entry.
#pragma once
#include <cstdint>
#include <algorithm>

#if defined(__HIPCC__)
#define RT_DRAIN_FN __host__ __device__ inline
#else
#define RT_DRAIN_FN inline
#endif

namespace rt_drain_pairs {

constexpr uint32_t kLanes = 64u;
constexpr uint32_t kFly = 4u;                          // pairs a lane tests per turn = batches of a window
constexpr uint32_t kTurnPairs = kLanes * kFly;         // pairs of a full turn
constexpr uint32_t kWindow = kLanes * kFly;            // records of a window
constexpr uint32_t kMaskBits = 5u;                     // triangles a record can mark

// record `j x 64 + lane` of the window that starts at `base`, and the record the lane loads for it (behind the region's end: the last
// record, whose mask the lane then takes as empty)
RT_DRAIN_FN uint32_t window_record(uint32_t base, uint32_t j, uint32_t lane) { return base + j * kLanes + lane; }
RT_DRAIN_FN uint32_t load_record(uint32_t base, uint32_t j, uint32_t lane, uint32_t n_rec) { return std::min(window_record(base, j, lane), n_rec - 1u); }
RT_DRAIN_FN bool record_in_region(uint32_t base, uint32_t j, uint32_t lane, uint32_t n_rec) { return n_rec - base > j * kLanes + lane; }      // (base < n_rec)
// is there a window behind the one at `base`
RT_DRAIN_FN bool window_behind(uint32_t base, uint32_t n_rec) { return n_rec - base > kWindow; }

// Set bits of a batch's earlier lanes / of the whole batch, from the counts of the three ballots "bit b of this lane's popcount is set":
// c_b = lanes below this one (or all lanes) in ballot b.
RT_DRAIN_FN uint32_t bits_from_ballots(uint32_t c0, uint32_t c1, uint32_t c2) { return c0 + 2u * c1 + 4u * c2; }
// the number a record's lowest remaining bit gets in the turn
RT_DRAIN_FN uint32_t first_pair(uint32_t fill, uint32_t bits_below) { return fill + bits_below; }
// does pair number `at` go into this turn's list
RT_DRAIN_FN bool pair_fits(uint32_t at) { return at < kTurnPairs; }
// where a lane writes: the pair's entry, or the scratch entry (`put` false: the record has no bit left, or the list is full)
RT_DRAIN_FN uint32_t list_entry(bool put, uint32_t at, uint32_t scratch_entry) { return put ? at : scratch_entry; }
// the list's length behind a batch that holds `batch_bits` set bits
RT_DRAIN_FN uint32_t fill_behind(uint32_t fill, uint32_t batch_bits) { return std::min(fill + batch_bits, kTurnPairs); }
RT_DRAIN_FN bool turn_full(uint32_t fill) { return fill >= kTurnPairs; }
// the entry lane `lane` reads for its q-th test of a turn of `fill` > 0 pairs, and whether that is a pair of its own (a lane without one
// reads the list's last pair and drops the result)
RT_DRAIN_FN bool lane_has_pair(uint32_t lane, uint32_t q, uint32_t fill) { return q * kLanes + lane < fill; }
RT_DRAIN_FN uint32_t lane_entry(uint32_t lane, uint32_t q, uint32_t fill) { return std::min(q * kLanes + lane, fill - 1u); }
// turns a region of `pairs` set bits takes
RT_DRAIN_FN uint64_t turns_of(uint64_t pairs) { return (pairs + kTurnPairs - 1u) / kTurnPairs; }

}  // namespace rt_drain_pairs
