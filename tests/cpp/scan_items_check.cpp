// The item schedule of the kernel-4 scan (raytracer.glsl_amd/csrc/rt_scan_items.hpp), checked by the host compiler alone.
//   (a) partition: turns + tail name every granule exactly once, for every divisor; every chunk's blocks get the ranks 0 .. blocks - 1;
//       a tail mapping of hdiv * k (a mutant, built here from the header's pieces) is caught.
//   (b) a model of the wave loop of scan_solo_kernel -- k, hi, step, tail, the record read ahead, ray_k, advance(), the empty-keep
//       `continue` -- over the waves of one chunk with the claim counter as a plain integer, interleaved in seeded random orders and two
//       adversarial ones, for all four distributions: every item is visited exactly once, a reused record names the granule item_of
//       would compute at that moment, and so do the rays that are taken as fetched.
//   (c) with -DSCAN_ITEMS_PARENT_RULE the model keeps the record and ray_k across the switch from turns to tail, as the kernel did before:
//       the program then reports per hybrid_div whether (b) is violated ("parent-rule hybrid_div 2: VIOLATION ..." / "... 3: clean"),
//       prints the first witness and exits 0; tests/test_scan_items.py asserts the outcomes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../raytracer.glsl_amd/csrc/rt_scan_items.hpp"

namespace si = rt_scan_items;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

struct Rng {
    uint64_t s;
    uint32_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return (uint32_t)((z ^ (z >> 31)) >> 32); }
    uint32_t below(uint32_t n) { return (uint32_t)(((uint64_t)next() * n) >> 32); }
};

// ---- (a) ------------------------------------------------------------------------------------------------------------------------------
template <class TailFn>
static bool partition_ok(uint32_t n_gran, uint32_t hybrid_div, TailFn tail_fn)
{
    const uint32_t hdiv = si::hdiv_of(hybrid_div), nt = si::n_tail(n_gran, hdiv), nk = si::n_turns(n_gran, hdiv);
    if (nt + nk != n_gran) return false;
    std::vector<uint32_t> seen(n_gran, 0u);
    for (uint32_t k = 0; k < nk; ++k) { const uint32_t g = si::turn_granule(k, hdiv); if (g >= n_gran) return false; seen[g]++; }
    for (uint32_t k = 0; k < nt; ++k) { const uint32_t g = tail_fn(k, hdiv); if (g >= n_gran) return false; seen[g]++; }
    for (uint32_t g = 0; g < n_gran; ++g) if (seen[g] != 1u) return false;
    return true;
}

[[maybe_unused]] static void check_partition()
{
    uint32_t mutant_caught = 0, mutant_shapes = 0;
    for (uint32_t n_gran = 0; n_gran <= 300; ++n_gran)
        for (uint32_t hd = 0; hd <= 64; ++hd) {      // (0 never reaches the kernel -- the variable refuses it -- and reads as 1)
            CHECK(partition_ok(n_gran, hd, [](uint32_t k, uint32_t hdiv) { return si::tail_granule(k, hdiv); }), "partition n_gran %u hybrid_div %u", n_gran, hd);
            if (hd >= 2 && n_gran >= hd) { ++mutant_shapes; if (!partition_ok(n_gran, hd, [](uint32_t k, uint32_t hdiv) { return hdiv * k; })) ++mutant_caught; }
        }
    CHECK(mutant_shapes > 0 && mutant_caught == mutant_shapes, "the tail mapping hdiv * k passed the partition check on %u of %u shapes", mutant_shapes - mutant_caught, mutant_shapes);
    for (long v = -2; v <= 70; ++v) CHECK(si::hybrid_div_accepted(v) == (v >= 1 && v <= 64), "hybrid_div_accepted(%ld)", v);

    std::vector<uint32_t> ranks, count;
    auto blocks_ranks = [&](uint32_t grid, uint32_t chunks) {
        count.assign(chunks, 0u); ranks.assign((size_t)chunks * grid, 0u);
        for (uint32_t b = 0; b < grid; ++b) {
            const uint32_t c = si::first_chunk(grid, b, chunks), r = si::rank_on(grid, b, chunks);
            CHECK(c < chunks, "grid %u chunks %u block %u: chunk %u", grid, chunks, b, c);
            if (c >= chunks) continue;
            CHECK(r < si::blocks_on(grid, c, chunks), "grid %u chunks %u block %u: rank %u of %u", grid, chunks, b, r, si::blocks_on(grid, c, chunks));
            if (r < grid) ranks[(size_t)c * grid + r]++;
            count[c]++;
        }
        uint32_t sum = 0;
        for (uint32_t c = 0; c < chunks; ++c) {
            const uint32_t n = si::blocks_on(grid, c, chunks);
            sum += n;
            CHECK(count[c] == n, "grid %u chunks %u chunk %u: %u blocks start there, blocks_on says %u", grid, chunks, c, count[c], n);
            for (uint32_t r = 0; r < n && r < grid; ++r) CHECK(ranks[(size_t)c * grid + r] == 1u, "grid %u chunks %u chunk %u: rank %u taken %u times", grid, chunks, c, r, ranks[(size_t)c * grid + r]);
        }
        CHECK(sum == grid, "grid %u chunks %u: blocks_on sums to %u", grid, chunks, sum);
    };
    for (uint32_t grid = 1; grid <= 600; ++grid)
        for (uint32_t chunks = 1; chunks <= 300; ++chunks) blocks_ranks(grid, chunks);
    blocks_ranks(280, 280); blocks_ranks(256, 280); blocks_ranks(560, 280);      // (more chunks than CUs: one block per chunk, or fewer blocks than chunks)
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------------------
enum { kStatic = 0, kDynamic = 1, kPlanned = 2, kHybrid = 3 };

struct Shape { int dist; uint32_t n_gran, waves, blocks, hybrid_div; bool cull; };      // waves per block (4 or 8); blocks that start on the chunk

struct Chunk {                              // what the waves of one chunk share
    Shape s;
    std::vector<uint8_t> keep;              // per granule: some tile must be scanned
    std::vector<uint32_t> items;            // dynamic + cull: the granules with a non-empty row
    uint32_t counter = 0;                   // the chunk's claim counter
    std::vector<uint32_t> visits, scans;    // per granule
};

// the first violation of each kind: a reused record that names another granule, rays taken as fetched that are another granule's (one wave
// per SIMD only: the kernel keeps ray_k for W == 1), a granule not visited or scanned exactly once
enum Kind { kRecord = 0, kRays = 1, kCount = 2, kKinds = 3 };
struct Violation {
    bool has[kKinds] = {false, false, false}; std::string text[kKinds];
    bool any() const { return has[0] || has[1] || has[2]; }
    const std::string &first() const { return has[0] ? text[0] : has[1] ? text[1] : text[2]; }
    void merge(const Violation &o) { for (int i = 0; i < kKinds; ++i) if (!has[i] && o.has[i]) { has[i] = true; text[i] = o.text[i]; } }
};

struct Wave {
    // the loop's state, named as in the kernel
    uint32_t k = 0, hi = 0, step = 0; bool tail = false;
    uint32_t rec_k = si::kNone, rec_g = 0; bool rec_keep = false;
    uint32_t ray_k = si::kNone, ray_g = 0;      // ray_g: the granule whose rays are in nxt_a / nxt_b
    uint32_t rank = 0, wave = 0;                // block's rank on the chunk, wave in the block
    bool started = false, done = false;
    uint32_t turns = 0;

    uint32_t n_claimable(const Chunk &c) const { const Shape &s = c.s; return s.dist == kHybrid ? si::n_tail(s.n_gran, si::hdiv_of(s.hybrid_div)) : n_items(c); }
    static uint32_t n_items(const Chunk &c) { return (c.s.cull && c.s.dist == kDynamic) ? (uint32_t)c.items.size() : c.s.n_gran; }
    void claim(Chunk &c, uint32_t seen, uint32_t &lo, uint32_t &end)
    {
        const uint32_t nc = n_claimable(c), rem = nc > seen ? nc - seen : 0u;
        const uint32_t n = c.s.dist == kHybrid ? si::claim_batch_hybrid(rem, c.s.blocks, c.s.waves) : si::claim_batch_dynamic(rem, c.s.blocks, c.s.waves);
        const uint32_t at = c.counter; c.counter += n;
        lo = std::min(at, nc); end = std::min(at + n, nc);
    }
    void item_of(const Chunk &c, uint32_t kk, uint32_t &g, bool &bits) const
    {
        const Shape &s = c.s;
        g = s.dist == kHybrid ? si::hybrid_granule(tail, kk, si::hdiv_of(s.hybrid_div)) : kk; bits = true;
        if (s.cull) { if (s.dist == kDynamic) g = c.items[kk]; bits = c.keep[g] != 0; }
    }
    void start(Chunk &c)
    {
        const Shape &s = c.s;
        if (s.dist == kDynamic) { step = 1; claim(c, 0u, k, hi); }
        else if (s.dist == kPlanned) {      // unit costs: the block's part (a, e] of the chunk's granules, a share per wave
            const uint32_t a = (uint32_t)(((uint64_t)s.n_gran * rank) / s.blocks), e = (uint32_t)(((uint64_t)s.n_gran * (rank + 1u)) / s.blocks);
            const uint32_t w_lo = a + (uint32_t)(((uint64_t)(e - a) * wave) / s.waves), w_hi = a + (uint32_t)(((uint64_t)(e - a) * (wave + 1u)) / s.waves);
            step = 1; k = std::min(w_lo, s.n_gran); hi = std::min(w_hi, s.n_gran);
        } else {
            step = s.blocks * s.waves; k = rank * s.waves + wave; hi = s.dist == kHybrid ? si::n_turns(s.n_gran, si::hdiv_of(s.hybrid_div)) : n_items(c);
            if (s.dist == kHybrid && k >= hi) { tail = true; step = 1; claim(c, 0u, k, hi); }      // (nothing read ahead yet)
        }
        started = true; done = !(k < hi);
    }
    void advance(Chunk &c)
    {
        const Shape &s = c.s;
        k += step;
        if (s.dist == kDynamic && k >= hi) claim(c, hi, k, hi);
        if (s.dist == kHybrid && k >= hi) {
            if (tail) claim(c, hi, k, hi);
            else {
                tail = true; step = 1;
#ifndef SCAN_ITEMS_PARENT_RULE
                rec_k = si::kNone; ray_k = si::kNone;      // the rule of rt_scan.hpp: a record is valid only in the numbering it was read in
#endif
                claim(c, 0u, k, hi);
            }
        }
    }
    // one pass of `while (k < hi)`
    void iterate(Chunk &c, Violation &v)
    {
        auto complain = [&](Kind kind, const char *what, uint32_t have, uint32_t want) {
            if (v.has[kind]) return;
            char buf[256];
            snprintf(buf, sizeof buf, "%s: dist %d n_gran %u waves %u blocks %u hybrid_div %u cull %d; block %u wave %u %s index %u after %u turns holds granule %u, item_of gives %u",
                     what, c.s.dist, c.s.n_gran, c.s.waves, c.s.blocks, c.s.hybrid_div, (int)c.s.cull, rank, wave, tail ? "tail" : "turn", k, turns, have, want);
            v.has[kind] = true; v.text[kind] = buf;
        };
        uint32_t g, now_g; bool keep, now_keep;
        item_of(c, k, now_g, now_keep);
        if (rec_k == k) { g = rec_g; keep = rec_keep; if (g != now_g) complain(kRecord, "reused record", g, now_g); } else { g = now_g; keep = now_keep; }
        if (!tail) ++turns;
        const uint32_t succ = k + step < hi ? k + step : si::kNone;
        if (succ != si::kNone) { item_of(c, succ, rec_g, rec_keep); rec_k = succ; }
        if (g < c.s.n_gran) c.visits[g]++;
        if (!keep) {
            if (succ != si::kNone && rec_keep) { ray_g = rec_g; ray_k = succ; }
            advance(c); done = !(k < hi);
            return;
        }
        if (ray_k != k) ray_g = g;                          // fetch_rays(g)
        else if (c.s.waves == 4u && ray_g != now_g) complain(kRays, "rays taken as fetched", ray_g, now_g);
        if (g < c.s.n_gran) c.scans[g]++;                     // prepare_ray(nxt_a, nxt_b) + the scan
        if (succ != si::kNone && rec_keep) { ray_g = rec_g; ray_k = succ; }
        advance(c); done = !(k < hi);
    }
};

enum Order { kRandom, kOneTurnFirst, kOneTurnLast };

// the waves of the chunk run to the end in one interleaving; returns the first violation
static Violation run(const Shape &s, Order order, uint64_t seed)
{
    Rng rng{seed};
    static Chunk c; static std::vector<Wave> w; static std::vector<uint32_t> live, idx;      // (kept across runs: no allocation per interleaving)
    c.s = s; c.counter = 0; c.items.clear();
    c.keep.assign(s.n_gran, 1);
    if (s.cull) for (uint32_t g = 0; g < s.n_gran; ++g) c.keep[g] = rng.below(3) != 0;      // a third of the rows empty
    for (uint32_t g = 0; g < s.n_gran; ++g) if (c.keep[g]) c.items.push_back(g);
    c.visits.assign(s.n_gran, 0u); c.scans.assign(s.n_gran, 0u);
    w.assign((size_t)s.blocks * s.waves, Wave());
    for (uint32_t b = 0; b < s.blocks; ++b) for (uint32_t i = 0; i < s.waves; ++i) { Wave &x = w[(size_t)b * s.waves + i]; x.rank = b; x.wave = i; }
    Violation v;
    auto step_wave = [&](Wave &x) { if (!x.started) x.start(c); else if (!x.done) x.iterate(c, v); };
    if (order == kRandom) {
        live.resize(w.size());
        for (uint32_t i = 0; i < live.size(); ++i) live[i] = i;
        // (a burst of 1-4 passes per pick: plain alternation would hardly ever let one wave run ahead of another's last turn)
        while (!live.empty()) {
            const uint32_t at = rng.below((uint32_t)live.size()); Wave &x = w[live[at]];
            for (uint32_t n = 1u + rng.below(4); n && !(x.started && x.done); --n) step_wave(x);
            if (x.started && x.done) { live[at] = live.back(); live.pop_back(); }
        }
    } else {
        // fixed turns of the wave with first index k0: ceil((hi - k0) / step).  "One turn first": the waves with at most one turn run to
        // their end one after the other, then the others by turn count; "last": the reverse.
        const uint32_t hi = s.dist == kHybrid ? si::n_turns(s.n_gran, si::hdiv_of(s.hybrid_div)) : s.n_gran, stride = s.blocks * s.waves;
        idx.resize(w.size());
        for (uint32_t i = 0; i < idx.size(); ++i) idx[i] = i;
        auto turns_of = [&](uint32_t i) { return i < hi ? (hi - i + stride - 1u) / stride : 0u; };
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return order == kOneTurnFirst ? turns_of(a) < turns_of(b) : turns_of(a) > turns_of(b); });
        for (uint32_t i : idx) { Wave &x = w[i]; while (!(x.started && x.done)) step_wave(x); }
    }
    {
        for (uint32_t g = 0; g < s.n_gran && !v.has[kCount]; ++g) {
            const uint32_t want_visits = (s.cull && s.dist == kDynamic) ? (uint32_t)c.keep[g] : 1u, want_scans = c.keep[g];
            if (c.visits[g] != want_visits || c.scans[g] != want_scans) {
                char buf[256];
                snprintf(buf, sizeof buf, "granule %u visited %u times (want %u), scanned %u times (want %u): dist %d n_gran %u waves %u blocks %u hybrid_div %u cull %d order %d seed %llu",
                         g, c.visits[g], want_visits, c.scans[g], want_scans, s.dist, s.n_gran, s.waves, s.blocks, s.hybrid_div, (int)s.cull, (int)order, (unsigned long long)seed);
                v.has[kCount] = true; v.text[kCount] = buf;
            }
        }
    }
    return v;
}

constexpr uint32_t kOrders = 200;
static const uint32_t kSteps[] = {4, 8, 16, 32, 64};
static const uint32_t kDivs[] = {1, 2, 3, 4, 7, 64};

// every order of one shape; the first violation of each kind (all_kinds: go on until a record and a rays violation are both found)
static Violation run_shape(const Shape &s, uint64_t &seed, bool all_kinds = false)
{
    Violation v;
    auto enough = [&]() { return all_kinds ? (v.has[kRecord] && v.has[kRays]) : v.any(); };
    for (int o = 0; o < 2 && !enough(); ++o) v.merge(run(s, o ? kOneTurnLast : kOneTurnFirst, ++seed));
    for (uint32_t i = 0; i < kOrders && !enough(); ++i) v.merge(run(s, kRandom, ++seed));
    return v;
}

// step = waves per block x blocks on the chunk: four waves (one per SIMD) or eight (two); where both fit, the shapes alternate
static Shape shape_of(int dist, uint32_t n_gran, uint32_t step, uint32_t hybrid_div, bool cull)
{
    const uint32_t waves = (step == 4u || (n_gran & 2u)) ? 4u : 8u;
    return {dist, n_gran, waves, step / waves, hybrid_div, cull};
}

int main()
{
#ifndef SCAN_ITEMS_PARENT_RULE
    check_partition();
    // the witness of the defect, by name: hybrid_div 2, one block of four waves, 12 granules
    { uint64_t seed = 1000; const Violation v = run_shape(shape_of(kHybrid, 12, 4, 2, false), seed); CHECK(!v.any(), "%s", v.first().c_str()); }
    uint64_t seed = 0; uint64_t runs = 0;
    for (uint32_t n_gran = 1; n_gran <= 200; ++n_gran)
        for (uint32_t step : kSteps) {
            const bool cull = (n_gran + step / 4u) % 2u != 0u;     // culled and unculled launches alternate over the shapes
            for (int dist : {kStatic, kDynamic, kPlanned}) { const Violation v = run_shape(shape_of(dist, n_gran, step, 3, cull), seed); CHECK(!v.any(), "%s", v.first().c_str()); runs += kOrders + 2; }
            for (uint32_t hd : kDivs) { const Violation v = run_shape(shape_of(kHybrid, n_gran, step, hd, cull), seed); CHECK(!v.any(), "%s", v.first().c_str()); runs += kOrders + 2; }
        }
    printf("%s: %llu interleavings, %d failures\n", g_fail ? "FAILED" : "ok", (unsigned long long)runs, g_fail);
    return g_fail ? 1 : 0;
#else
    // (c): the parent's rule, over the same shapes and orders.  Per divisor and kind: "parent-rule hybrid_div D record|rays: VIOLATION in N
    // shapes; first: ..." or "...: clean"
    static const char *const names[] = {"record", "rays"};
    for (uint32_t hd : kDivs) {
        uint64_t seed = 0; Violation first; uint32_t bad[2] = {0, 0};
        for (uint32_t n_gran = 1; n_gran <= 200; ++n_gran)
            for (uint32_t step : kSteps) {
                const bool cull = (n_gran + step / 4u) % 2u != 0u;
                const Violation v = run_shape(shape_of(kHybrid, n_gran, step, hd, cull), seed, true);
                first.merge(v);
                for (int kind = 0; kind < 2; ++kind) if (v.has[kind]) ++bad[kind];
            }
        for (int kind = 0; kind < 2; ++kind) {
            if (bad[kind]) printf("parent-rule hybrid_div %u %s: VIOLATION in %u shapes; first: %s\n", hd, names[kind], bad[kind], first.text[kind].c_str());
            else printf("parent-rule hybrid_div %u %s: clean\n", hd, names[kind]);
        }
    }
    return 0;
#endif
}
