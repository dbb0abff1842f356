// How a launch of the kernel-4 scan (rt_scan.hpp) is cut into chunks, blocks and work items, and how large the buffers are that it
// indexes, as plain host C++: no HIP in this header, so that the host compiler can build it alone (tests/cpp/scan_launch_check.cpp).
// Arithmetic only: nothing here allocates, reads the environment or launches.  capacity() is what ensure_wave_buffers sizes from the mesh
// and the options, launch() what one bounce does with its queue; launch.blocks x launch.waves <= capacity.regions (a candidate region per
// scan wave) and launch.chunks <= capacity.sched_stride (a work counter and an item count per chunk) tie the two.
#pragma once
#include <cstdint>
#include <cstddef>
#include <algorithm>

namespace rt_scan_launch {

constexpr uint32_t kQuadTris = 40, kQuadTiles = 4, kRaysPerWave = 128;      // (rtgl_amd.hip ties them to rt_mfma.hpp and SoloCfg)

// the quads that hold triangles (the last group may end in padding quads)
inline uint32_t real_quads(uint32_t n_groups, uint32_t group_quads, uint32_t n_tri_visits) { return std::min(n_groups * group_quads, (n_tri_visits + kQuadTris - 1) / kQuadTris); }

struct Setup { uint32_t n_cus, real_quads, mf_chunk_quads; int scan_waves, scan_dynamic, cull; };      // device, mesh and the options of those names

// kernel 4 launches at most max(CUs, chunks) blocks (8 waves with two waves per SIMD); each wave owns one region of the candidate buffer
struct Capacity {
    uint32_t chunks, regions, sched_stride, keep_words;      // chunks at the full chunk size; work counters per bounce; words per granule: one bit per tile
    size_t keep_count(uint32_t n0) const { return ((size_t)n0 / 128 + 16) * keep_words; }      // one bit per (granule of 128 rays, tile); + 16 granules read ahead of the last one
};
inline Capacity capacity(const Setup &s)
{
    const uint32_t chunk_quads = std::min(s.mf_chunk_quads, std::max(s.real_quads, 1u)), chunks = (s.real_quads + chunk_quads - 1) / chunk_quads;
    const uint32_t stride = std::max<uint32_t>(s.n_cus, chunks);
    return {chunks, stride * 8u, stride, std::max(1u, (s.real_quads * kQuadTiles + 31u) / 32u)};
}

// work distribution of the scan (rt_scan.hpp): "scan_dynamic" 0 = by the mesh (hybrid; dynamic from 1,024 quads = 41k triangles on: few
// blocks per chunk), 1 = static turns, 2 = dynamic claims, 3 = planned (equal-cost intervals of the item line, no atomics), 4 = hybrid
// (turns + a claimed tail).  Returns the kernel's kDist: 0 static, 1 dynamic, 2 planned, 3 hybrid.  This is the choice for the MESH: a launch
// may still take fixed turns (Launch::dist), but whether a frame's claim counters are cleared is decided by this value.
inline int mesh_dist(const Setup &s) { return s.scan_dynamic ? s.scan_dynamic - 1 : (s.real_quads >= 1024u ? 1 : 3); }
inline bool uses_claim_counters(int dist) { return dist == 1 || dist == 3; }

// packet culling pays where the 128 rays of a granule are coherent: the camera rays, and every queue that was binned (option "cull":
// 0 never, 1 bounce 0, 2 every bounce as the queues come, 3 (default) bounce 0 and the binned bounces)
inline bool culls(const Setup &s, uint32_t bounce, bool binned) { return s.cull == 2 || (s.cull >= 1 && bounce == 0) || (s.cull == 3 && binned); }

struct Launch {
    uint32_t W, waves, est_gran, chunk_quads, chunks, blocks;      // waves per SIMD and per block; granules of 128 rays expected in the queue
    int cull, dist; size_t lds;                                    // packet culling runs; the kernel's kDist; dynamic shared memory of the scan
    uint32_t cull_blocks, items_grid_x, items_grid_y;              // grids of packet_cull_kernel and cull_items_kernel
    // bytes.  Work items (cull && dist == 1): [one count per chunk][chunks x (granules of the whole image) entries]; planned (cull &&
    // dist == 2): cost prefix sums per chunk [chunks x stride u32][chunks totals u32][chunks + 1 starts u64]
    uint32_t stride; size_t items_head, items_need, plan_off_tot, plan_off_base, plan_need;
};

// n0: the slots of the queue; est: the rays expected in it; binned: the queue was binned
inline Launch launch(const Setup &s, uint64_t items_per_wave, uint32_t n0, uint32_t est, uint32_t bounce, bool binned)
{
    Launch L = {};
    // Two waves per SIMD run the steady stream 1.5x faster (47 against 70 cycles per product).  Until the item loop moved into scalar
    // registers small launches were better off with one wave per SIMD (half as many rays per block); measured since: two waves win or tie
    // everywhere (C2 3.394 against 3.434 ms, a rank of eight 0.686 against 0.713 ms).  "scan_waves" = 0 / 2: two, 1: one.
    L.W = s.scan_waves == 1 ? 1u : 2u; L.waves = 4u * L.W;
    L.est_gran = (est + kRaysPerWave - 1u) / kRaysPerWave;
    // A launch has (granules x chunks) work items for its waves, claimed dynamically (rt_scan.hpp).  Late bounces (and every bounce of a
    // rank that owns an eighth of the image) have few granules: cut the triangle range finer, down to 4 quads per chunk, until there are
    // three items per wave (each item pays its ray and group set-up again, ~20 % at 8 quads, so only as far as needed -- thresholds of 1, 2,
    // 4, 8 items per wave measured: 2-4 are best for a rank of four or eight, none matters at N = 1; never more chunks than CUs)
    uint32_t chunk_quads = std::min(s.mf_chunk_quads, std::max(s.real_quads, 1u));
    while (chunk_quads > 4u && (uint64_t)L.est_gran * ((s.real_quads + chunk_quads - 1) / chunk_quads) < items_per_wave * s.n_cus * L.waves
           && (s.real_quads + chunk_quads / 2 - 1) / (chunk_quads / 2) <= s.n_cus)
        chunk_quads /= 2u;
    const uint32_t chunks = (s.real_quads + chunk_quads - 1) / chunk_quads;
    L.chunk_quads = chunk_quads; L.chunks = L.items_grid_y = chunks;
    L.cull = culls(s, bounce, binned);
    // (auto: the camera-ray bounce of a small mesh keeps its fixed turns -- almost every item is empty there and a claimed tail only adds
    // round trips: 74 us against 168 on C2; the binned bounces take the hybrid form: 660 -> 589, 553 -> 499 us)
    // (unculled launches have items of equal cost: fixed turns are balanced there and a claimed tail only adds round trips)
    L.dist = (s.scan_dynamic == 0 && (bounce == 0 || !L.cull) && mesh_dist(s) == 3) ? 0 : mesh_dist(s);
    // one block per CU (forced by the LDS request); fewer when there is not an item per wave.  Static: the same number of blocks on every chunk.
    L.blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)L.est_gran * chunks + L.waves - 1) / L.waves, (uint64_t)s.n_cus));
    if (L.dist == 0 || L.dist == 3) L.blocks = std::max(1u, std::min((L.est_gran + L.waves - 1u) / L.waves, std::max(1u, s.n_cus / chunks))) * chunks;
    L.lds = std::max<size_t>(((size_t)chunk_quads * kQuadTiles + 4) * 1024, 96 * 1024);   // + the four rows read two trips ahead behind the last tile; > half of the CU's LDS with the static queue: one block per CU
    L.cull_blocks = std::max(1u, std::min((L.est_gran + 3u) / 4u, 8192u));
    L.items_grid_x = std::max(1u, std::min((L.est_gran + 255u) / 256u, 1024u));
    L.stride = n0 / kRaysPerWave + 1u;
    L.items_head = ((size_t)capacity(s).sched_stride * sizeof(uint32_t) + 255) & ~(size_t)255;
    L.items_need = L.items_head + (size_t)chunks * L.stride * sizeof(uint32_t);
    L.plan_off_tot = (((size_t)chunks * L.stride * sizeof(uint32_t)) + 255) & ~(size_t)255;
    L.plan_off_base = (L.plan_off_tot + (size_t)chunks * sizeof(uint32_t) + 255) & ~(size_t)255;
    L.plan_need = L.plan_off_base + ((size_t)chunks + 1) * sizeof(unsigned long long);
    return L;
}

}  // namespace rt_scan_launch
