// The pair expansion of the scan's tail drain (raytracer.glsl_amd/csrc/rt_drain_pairs.hpp), checked by the host compiler alone.
// A model of drain_region (rt_scan.hpp) over one wave of 64 lanes -- the window of 64 x 4 records in "registers", the three ballots
// of a batch, the list in a queue of exactly SoloCfg::kQueue entries on the heap (the sanitizer sees any index beyond it), the four
// reads per lane -- with the header's functions in the places where the kernel calls them.  For regions of 0 .. 1,300 records and the
// mask populations below:
//   * every (record, set bit) is tested exactly once, by a lane that owns the pair, and in record order;
//   * no list index reaches kQueue, the scratch entry is never read, at most four pairs per lane and turn;
//   * the loop ends, after exactly ceil(pairs / 256) turns (carries force none: a used-up window is replaced inside the turn);
//   * a window is only replaced when every one of its bits has gone into a list.
// A mutant of the model that forgets what a record carries over (built here, from the header's pieces) is caught.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "../../raytracer.glsl_amd/csrc/rt_drain_pairs.hpp"

namespace dp = rt_drain_pairs;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

struct Rng {
    uint64_t s;
    uint32_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return (uint32_t)((z ^ (z >> 31)) >> 32); }
    uint32_t below(uint32_t n) { return (uint32_t)(((uint64_t)next() * n) >> 32); }
};

constexpr uint32_t kQueue = 2u * 64u + 192u + 1u;      // SoloCfg::kQueue (tests/test_drain_pairs.py holds the two together)
constexpr uint32_t kScratch = kQueue - 1u;
constexpr uint32_t L = dp::kLanes, K = dp::kFly;

struct Pair { uint32_t rec, bit; };
struct Outcome { uint64_t turns = 0, tests = 0; bool ended = true, ok = true; };

// lanes of `m` below `lane` (the device's mbcnt)
static uint32_t below(uint64_t m, uint32_t lane) { return (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull)); }

// The wave.  mask[i] = the 5-bit mask of record i; a pair is written to the list as (record, bit) where the kernel writes (slot, position).
// forget_carry: the mutant -- a record that was only partly taken loses the rest.
static Outcome run_wave(const std::vector<uint32_t> &mask, bool forget_carry, bool quiet)
{
    Outcome out;
    const uint32_t n_rec = (uint32_t)mask.size();
    if (n_rec == 0u) return out;                        // (the kernel does not enter the drain)
    uint64_t pairs = 0;
    for (uint32_t m : mask) pairs += (uint32_t)__builtin_popcount(m);
    std::vector<uint32_t> tested((size_t)n_rec * dp::kMaskBits, 0u);
    std::unique_ptr<Pair[]> list(new Pair[kQueue]);
    for (uint32_t i = 0; i < kQueue; ++i) list[i] = Pair{0xFFFFFFFFu, 0xFFu};           // (nothing written yet: no record)
#define WCHECK(c, ...) do { if (!(c)) { out.ok = false; if (!quiet) CHECK(false, __VA_ARGS__); } } while (0)
    uint32_t rec_of[K][L], um[K][L], nxt[K][L];
    auto load_window = [&](uint32_t at) {
        for (uint32_t j = 0; j < K; ++j) for (uint32_t l = 0; l < L; ++l) {
            const uint32_t i = dp::load_record(at, j, l, n_rec);
            WCHECK(i < n_rec, "load of record %u of %u", i, n_rec);
            nxt[j][l] = i < n_rec ? i : 0u;
        }
    };
    auto take_window = [&](uint32_t at) {
        for (uint32_t j = 0; j < K; ++j) for (uint32_t l = 0; l < L; ++l) {
            rec_of[j][l] = nxt[j][l];
            const bool in = dp::record_in_region(at, j, l, n_rec);
            WCHECK(in == ((uint64_t)at + j * L + l < n_rec), "record_in_region(%u, %u, %u, %u)", at, j, l, n_rec);
            WCHECK(!in || nxt[j][l] == dp::window_record(at, j, l), "window %u batch %u lane %u holds record %u", at, j, l, nxt[j][l]);
            um[j][l] = in ? mask[nxt[j][l]] : 0u;
        }
    };
    uint32_t base = 0u;
    load_window(0u); take_window(0u);
    load_window(dp::kWindow);
    uint32_t last_rec = 0u, last_bit = 0u; bool any_tested = false;
    const uint64_t turn_limit = pairs / dp::kTurnPairs + 8u;
    for (;;) {
        if (out.turns > turn_limit) { out.ended = false; break; }
        uint32_t fill = 0u;
        for (;;) {
            for (uint32_t j = 0; j < K; ++j) {
                uint64_t b0 = 0, b1 = 0, b2 = 0;
                for (uint32_t l = 0; l < L; ++l) {
                    const uint32_t pc = (uint32_t)__builtin_popcount(um[j][l]);
                    b0 |= (uint64_t)(pc & 1u) << l; b1 |= (uint64_t)((pc >> 1) & 1u) << l; b2 |= (uint64_t)((pc >> 2) & 1u) << l;
                }
                const uint32_t batch_bits = dp::bits_from_ballots((uint32_t)__builtin_popcountll(b0), (uint32_t)__builtin_popcountll(b1), (uint32_t)__builtin_popcountll(b2));
                if (batch_bits == 0u || dp::turn_full(fill)) continue;
                const uint32_t deepest = b2 ? dp::kMaskBits : (b1 ? 3u : 1u);
                for (uint32_t l = 0; l < L; ++l) {
                    uint32_t at = dp::first_pair(fill, dp::bits_from_ballots(below(b0, l), below(b1, l), below(b2, l)));
                    bool took = false;
                    for (uint32_t k = 0; k < dp::kMaskBits; ++k) {
                        if (k >= deepest) { WCHECK(um[j][l] == 0u || !dp::pair_fits(at), "batch %u lane %u: bits left behind the deepest mask", j, l); break; }
                        const bool put = um[j][l] != 0u && dp::pair_fits(at);
                        const uint32_t bit = um[j][l] ? (uint32_t)__builtin_ctz(um[j][l]) : 0u;
                        const uint32_t entry = dp::list_entry(put, at, kScratch);
                        WCHECK(entry < kQueue, "list index %u", entry);
                        WCHECK(!put || entry < dp::kTurnPairs, "pair written to entry %u", entry);
                        if (entry < kQueue) list[entry] = Pair{rec_of[j][l], bit};
                        if (put) { um[j][l] &= um[j][l] - 1u; ++at; took = true; }
                    }
                    if (forget_carry && took) um[j][l] = 0u;
                }
                fill = dp::fill_behind(fill, batch_bits);
                WCHECK(fill <= dp::kTurnPairs, "fill %u", fill);
            }
            if (dp::turn_full(fill) || !dp::window_behind(base, n_rec)) break;
            for (uint32_t j = 0; j < K; ++j) for (uint32_t l = 0; l < L; ++l) WCHECK(um[j][l] == 0u, "window %u replaced with bits %#x of batch %u lane %u untested", base, um[j][l], j, l);
            base += dp::kWindow;
            WCHECK(base < n_rec, "window %u of %u records", base, n_rec);
            take_window(base); load_window(base + dp::kWindow);
        }
        if (fill == 0u) break;
        ++out.turns;
        // the tests: which list entry each (lane, q) reads; the pairs in list order
        std::vector<uint32_t> owners(dp::kTurnPairs, 0u);
        for (uint32_t l = 0; l < L; ++l) {
            uint32_t own = 0u;
            for (uint32_t q = 0; q < K; ++q) {
                const uint32_t entry = dp::lane_entry(l, q, fill);
                WCHECK(entry < fill, "lane %u test %u reads entry %u of a list of %u", l, q, entry, fill);
                if (dp::lane_has_pair(l, q, fill) && entry < fill) { owners[entry]++; ++own; }
            }
            WCHECK(own <= K, "lane %u owns %u pairs", l, own);
        }
        for (uint32_t e = 0; e < fill; ++e) {
            WCHECK(owners[e] == 1u, "entry %u of a list of %u is tested %u times", e, fill, owners[e]);
            const Pair p = list[e];
            WCHECK(p.rec < n_rec && p.bit < dp::kMaskBits && ((mask[p.rec < n_rec ? p.rec : 0u] >> p.bit) & 1u), "entry %u: record %u bit %u is no pair", e, p.rec, p.bit);
            if (p.rec >= n_rec || p.bit >= dp::kMaskBits) continue;
            tested[(size_t)p.rec * dp::kMaskBits + p.bit]++; ++out.tests;
            WCHECK(!any_tested || p.rec > last_rec || (p.rec == last_rec && p.bit > last_bit), "record %u bit %u behind record %u bit %u", p.rec, p.bit, last_rec, last_bit);
            last_rec = p.rec; last_bit = p.bit; any_tested = true;
        }
        if (!dp::turn_full(fill)) break;
    }
    WCHECK(out.ended, "%u records: the loop did not end within %llu turns", n_rec, (unsigned long long)turn_limit);
    for (uint32_t i = 0; i < n_rec; ++i)
        for (uint32_t b = 0; b < dp::kMaskBits; ++b)
            WCHECK(tested[(size_t)i * dp::kMaskBits + b] == ((mask[i] >> b) & 1u), "record %u of %u bit %u (mask %#x): tested %u times", i, n_rec, b, mask[i], tested[(size_t)i * dp::kMaskBits + b]);
    WCHECK(out.turns == dp::turns_of(pairs), "%u records, %llu pairs: %llu turns, expected %llu", n_rec, (unsigned long long)pairs, (unsigned long long)out.turns, (unsigned long long)dp::turns_of(pairs));
#undef WCHECK
    return out;
}

int main()
{
    Rng rng{20240607ull};
    uint64_t regions = 0, mutant_shapes = 0, mutant_caught = 0, turns = 0;
    auto run = [&](const std::vector<uint32_t> &mask) { const Outcome o = run_wave(mask, false, false); ++regions; turns += o.turns; };
    for (uint32_t n = 0; n <= 1300u; ++n) {
        std::vector<uint32_t> m(n);
        for (auto &x : m) x = 31u;                                   // every mask full: five turns' worth per window, every record but few carries
        run(m);
        for (auto &x : m) x = 1u << rng.below(dp::kMaskBits);        // single bits: a turn is a window
        run(m);
        for (auto &x : m) x = 1u + rng.below(31u);                   // random, none empty (what flush() writes)
        run(m);
        for (auto &x : m) x = rng.below(4u) ? 0u : rng.below(32u);   // random and mostly empty (no such record is written; the loop must not depend on it)
        run(m);
        for (auto &x : m) x = 1u << rng.below(dp::kMaskBits);        // one full mask among single bits
        if (n) m[rng.below(n)] = 31u;
        run(m);
        // a full mask that straddles the end of a turn: among single bits, the record whose five pairs are numbers 256 t - r .. 256 t - r + 4
        for (uint32_t t = 1; t * dp::kTurnPairs <= n; ++t)
            for (uint32_t r = 1; r < dp::kMaskBits; ++r) {
                for (auto &x : m) x = 1u << rng.below(dp::kMaskBits);
                const uint32_t at = t * dp::kTurnPairs - r - 4u * (t - 1u);       // (the t - 1 straddlers before it add four pairs each)
                for (uint32_t u = 1; u <= t; ++u) { const uint32_t i = u * dp::kTurnPairs - r - 4u * (u - 1u); if (i < n) m[i] = 31u; }
                if (at >= n) continue;
                run(m);
                const Outcome mut = run_wave(m, true, true);
                ++mutant_shapes; if (!mut.ok) ++mutant_caught;
            }
    }
    CHECK(mutant_shapes > 0 && mutant_caught == mutant_shapes, "the model that forgets a record's carry passed on %llu of %llu straddling shapes", (unsigned long long)(mutant_shapes - mutant_caught), (unsigned long long)mutant_shapes);
    CHECK(dp::turns_of(0) == 0 && dp::turns_of(1) == 1 && dp::turns_of(256) == 1 && dp::turns_of(257) == 2, "turns_of");
    printf("%s: %llu regions, %llu turns, mutant caught on %llu of %llu shapes, %d failures\n", g_fail ? "FAILED" : "ok", (unsigned long long)regions, (unsigned long long)turns,
           (unsigned long long)mutant_caught, (unsigned long long)mutant_shapes, g_fail);
    return g_fail ? 1 : 0;
}
