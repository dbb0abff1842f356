// buffer_ledger_check.cpp -- the device-buffer ledger (raytracer.glsl_amd/csrc/rt_buffers.hpp) against a counting allocator over malloc / free
// that can be told to fail its n-th allocation.  One fixed script of operations runs clean (the total after every step is checked against the
// figures below) and then once per n = 1..N with the n-th allocation failing, on to its end.  After EVERY step:
//   * a capacity field is non-zero only while its pointer is a live block of at least that many units;
//   * the slot of a failed operation is null (and its capacity 0);
//   * the ledger's total is the sum of the live blocks, and every live block is held by exactly one slot;
//   * nothing was freed that was not live (no double free); at the end nothing is live.
// One more run has every free report an error (after freeing): the code comes back, the entry is gone and the slot is null all the same.
// Exit status 0: all of it held.  (tests/test_buffer_ledger.py builds this with the address and undefined-behaviour sanitizers.)
#include "../../raytracer.glsl_amd/csrc/rt_buffers.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>

static std::map<void *, size_t> g_live;       // block -> bytes
static int g_allocs = 0, g_fail_at = 0, g_bad_frees = 0, g_failures = 0, g_free_rc = 0;

static int fake_alloc(void **p, size_t bytes)
{
    if (++g_allocs == g_fail_at) return 2;     // (an allocator's "out of memory")
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return 1;
    g_live[*p] = bytes;
    return 0;
}
static int fake_free(void *p)
{
    if (!g_live.erase(p)) { ++g_bad_frees; return 0; }      // not (or no longer) live: counted, and NOT handed to free()
    free(p);
    return g_free_rc;
}

#define EXPECT(cond) do { if (!(cond)) { ++g_failures; std::fprintf(stderr, "fail_at %d, step %d: %s\n", g_fail_at, step, #cond); } } while (0)

enum Kind { kAllocate, kEnsure, kGrowD, kGrowE, kRelease, kReleaseAll };
struct Op { Kind kind; int slot; size_t need, bytes, clean_total; };
// slots 0..2: a, b, c (plain); 3: d, grown in units of 4 bytes with a size_t capacity; 4: e, units of 8 bytes with a 32-bit capacity
static const Op kScript[] = {
    {kAllocate, 0, 0, 100, 100}, {kAllocate, 1, 0, 200, 300}, {kAllocate, 0, 0, 50, 250},      // (the third: into a live slot)
    {kEnsure, 2, 0, 64, 314}, {kEnsure, 2, 0, 999, 314},                                       // (the second: nothing)
    {kGrowD, 3, 10, 40, 354}, {kGrowD, 3, 5, 20, 354}, {kGrowD, 3, 20, 80, 394},               // (sufficient in between)
    {kRelease, 1, 0, 0, 194}, {kRelease, 1, 0, 0, 194}, {kEnsure, 1, 0, 300, 494},
    {kGrowE, 4, 3, 24, 518}, {kAllocate, 2, 0, 10, 464}, {kGrowE, 4, 3, 24, 464}, {kGrowE, 4, 9, 72, 512},
    {kRelease, 0, 0, 0, 462}, {kGrowD, 3, 21, 84, 466}, {kEnsure, 0, 0, 8, 474},
    {kReleaseAll, 0, 0, 0, 0}, {kEnsure, 0, 0, 16, 16}, {kReleaseAll, 0, 0, 0, 0},
};
static const int kSteps = (int)(sizeof kScript / sizeof kScript[0]), kAllocsClean = 13;

static void run(int fail_at)
{
    g_allocs = 0; g_fail_at = fail_at;
    void *slot[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap_d = 0; uint32_t cap_e = 0;
    int step = 0;
    {
        rt_buffers::Ledger ledger(fake_alloc, fake_free);
        for (; step < kSteps; ++step) {
            const Op &op = kScript[step];
            const int allocs_before = g_allocs;
            const size_t live_before = g_live.size();
            int rc = 0;
            switch (op.kind) {
            case kAllocate: rc = ledger.allocate(&slot[op.slot], op.bytes); break;
            case kEnsure: rc = ledger.ensure(&slot[op.slot], op.bytes); break;
            case kGrowD: rc = ledger.grow(&slot[3], cap_d, op.need, op.bytes); break;
            case kGrowE: rc = ledger.grow(&slot[4], cap_e, (uint32_t)op.need, op.bytes); break;
            case kRelease: rc = ledger.release(&slot[op.slot]); break;
            case kReleaseAll: ledger.release_all(); cap_d = 0; cap_e = 0; break;      // (capacities are the caller's: it drops them with the buffers)
            }
            const bool failed = g_allocs == g_fail_at && allocs_before != g_allocs;
            if (g_free_rc) {      // the free's code, from the operations that freed; an allocate whose free failed allocates nothing
                const bool freed = g_live.size() < live_before;
                EXPECT(rc == (freed && op.kind != kReleaseAll ? g_free_rc : 0));
                if (rc) { EXPECT(slot[op.slot] == nullptr); EXPECT(g_allocs == allocs_before); }
                if (rc && op.kind == kGrowD) EXPECT(cap_d == 0);
                if (rc && op.kind == kGrowE) EXPECT(cap_e == 0);
            } else
            EXPECT((rc != 0) == failed);
            if (failed) { EXPECT(rc == 2); EXPECT(slot[op.slot] == nullptr); }
            if (failed && op.kind == kGrowD) EXPECT(cap_d == 0);
            if (failed && op.kind == kGrowE) EXPECT(cap_e == 0);
            if (!failed && !rc && (op.kind == kAllocate || op.kind == kEnsure || op.kind == kGrowD || op.kind == kGrowE)) EXPECT(slot[op.slot] != nullptr);
            if (op.kind == kRelease) EXPECT(slot[op.slot] == nullptr);
            // the capacity invariant
            if (cap_d) EXPECT(slot[3] && g_live.count(slot[3]) && g_live[slot[3]] >= cap_d * 4);
            if (cap_e) EXPECT(slot[4] && g_live.count(slot[4]) && g_live[slot[4]] >= (size_t)cap_e * 8);
            // the total is the sum of the live blocks; every live block sits in exactly one slot, every slot is null or live
            size_t sum = 0, held = 0;
            for (const auto &kv : g_live) sum += kv.second;
            for (int k = 0; k < 5; ++k) if (slot[k]) { EXPECT(g_live.count(slot[k]) == 1); ++held; for (int j = 0; j < k; ++j) EXPECT(slot[j] != slot[k]); }
            EXPECT(ledger.total_bytes() == sum);
            EXPECT(held == g_live.size());
            EXPECT(g_bad_frees == 0);
            if (fail_at == 0 && !g_free_rc) EXPECT(ledger.total_bytes() == op.clean_total);
        }
        if (fail_at == 0 && !g_free_rc) EXPECT(g_allocs == kAllocsClean);
        EXPECT(ledger.ensure(&slot[1], 32) == 0 || g_allocs == g_fail_at);      // one block left for the destructor
    }
    EXPECT(g_live.empty());                            // nothing left live, by the last release_all and the destructor
    EXPECT(slot[1] == nullptr);
    EXPECT(g_bad_frees == 0);
    for (const auto &kv : g_live) free(kv.first);
    g_live.clear();
}

int main()
{
    for (int n = 0; n <= kAllocsClean + 1; ++n) run(n);      // 0: no failure; kAllocsClean + 1: the closing ensure fails
    g_free_rc = 7;
    run(0);
    g_free_rc = 0;
    if (g_failures) { std::fprintf(stderr, "buffer_ledger_check: %d expectation(s) failed\n", g_failures); return 1; }
    std::printf("buffer_ledger_check ok: %d steps x %d runs\n", kSteps, kAllocsClean + 3);
    return 0;
}
