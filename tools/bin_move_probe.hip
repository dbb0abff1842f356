// bin_move_probe.hip -- ray binning's move (rt_wavefront.hpp): scatter the staged rays to their slots, or gather them from there?
//
// The shade kernel of a binned bounce leaves the next bounce's rays in a staging queue, and the move puts each ray at its slot
// `to = first[key] + rank` of the next queue.  Within a wave the destinations are effectively random.  Three ways to move
// ~2.5 M records of 68 B through a random permutation, each timed from the state a shade launch leaves (staging just written
// through, then the destination's previous contents written through as well):
//   (a) scatter   one launch: read staging coalesced, five write-through stores per ray to the SoA destination at `to`
//                 (a, b, c, rng 16 B each, pixel 4 B) -- sort_scatter_kernel
//   (b) gather    place: one 4-B write-through store src[to] = slot per ray; then gather: per destination slot read src, load the five
//                 SoA staging streams at it and store them coalesced (write-through)
//   (c) gather    the same from AoS staging: one 64-B record (a, b, c, rng) per ray plus the 4-B pixel stream
// The gather is timed on its own here; in the pipeline it is fused into packet_cull_kernel's load of the granule.
// Build: hipcc -O3 --offload-arch=gfx950 tools/bin_move_probe.hip -o tools/bin_move_probe ; run: tools/bin_move_probe [n] [reps]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

typedef uint32_t u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st4(uint4 *p, uint4 v) { const u4v w = {v.x, v.y, v.z, v.w}; asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" :: "v"(p), "v"(w) : "memory"); }
__device__ __forceinline__ void st1(uint32_t *p, uint32_t x) { asm volatile("global_store_dword %0, %1, off sc0 sc1" :: "v"(p), "v"(x) : "memory"); }

struct Soa { uint4 *a, *b, *c, *g; uint32_t *px; };

// what a shade launch leaves: staging written through, coalesced
__global__ void __launch_bounds__(256) fill_soa(Soa s, uint32_t n, uint32_t tag)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    st4(s.a + i, make_uint4(i, tag, 1u, 2u)); st4(s.b + i, make_uint4(i, tag, 3u, 4u)); st4(s.c + i, make_uint4(i, tag, 5u, 6u));
    st4(s.g + i, make_uint4(i, tag, 7u, 8u)); st1(s.px + i, i ^ tag);
}
__global__ void __launch_bounds__(256) fill_aos(uint4 *rec, uint32_t *px, uint32_t n, uint32_t tag)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) st4(rec + 4u * i + k, make_uint4(i, tag, 2u * k + 1u, 2u * k + 2u));
    st1(px + i, i ^ tag);
}

// (a) today's move
__global__ void __launch_bounds__(256) move_scatter(Soa st, Soa q, const uint32_t *to_of, uint32_t n)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t to = to_of[i];
        const uint4 a = st.a[i], b = st.b[i], c = st.c[i], g = st.g[i];
        const uint32_t p = st.px[i];
        if (to >= n) continue;
        st4(q.a + to, a); st4(q.b + to, b); st4(q.c + to, c); st4(q.g + to, g); st1(q.px + to, p);
    }
}
// (b), (c): the index scatter
__global__ void __launch_bounds__(256) place(uint32_t *src, const uint32_t *to_of, uint32_t n)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t to = to_of[i];
        if (to < n) st1(src + to, i);
    }
}
__global__ void __launch_bounds__(256) gather_soa(Soa st, Soa q, const uint32_t *src, uint32_t n)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t s = src[j];
    if (s >= n) return;
    const uint4 a = st.a[s], b = st.b[s], c = st.c[s], g = st.g[s];
    const uint32_t p = st.px[s];
    st4(q.a + j, a); st4(q.b + j, b); st4(q.c + j, c); st4(q.g + j, g); st1(q.px + j, p);
}
__global__ void __launch_bounds__(256) gather_aos(const uint4 *rec, const uint32_t *spx, Soa q, const uint32_t *src, uint32_t n)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t s = src[j];
    if (s >= n) return;
    const uint4 a = rec[4u * s], b = rec[4u * s + 1u], c = rec[4u * s + 2u], g = rec[4u * s + 3u];
    const uint32_t p = spx[s];
    st4(q.a + j, a); st4(q.b + j, b); st4(q.c + j, c); st4(q.g + j, g); st1(q.px + j, p);
}

static double median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char **argv)
{
    const uint32_t n = argc > 1 ? (uint32_t)atoi(argv[1]) : 2500000u;
    const int reps = argc > 2 ? atoi(argv[2]) : 30;
    std::vector<uint32_t> perm(n);
    for (uint32_t i = 0; i < n; ++i) perm[i] = i;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (uint32_t i = n - 1; i > 0; --i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; std::swap(perm[i], perm[(uint32_t)(x % (i + 1u))]); }
    auto alloc_soa = [&](Soa &s) -> hipError_t {
        hipError_t e;
        if ((e = hipMalloc((void **)&s.a, (size_t)n * 16)) || (e = hipMalloc((void **)&s.b, (size_t)n * 16)) || (e = hipMalloc((void **)&s.c, (size_t)n * 16))
            || (e = hipMalloc((void **)&s.g, (size_t)n * 16)) || (e = hipMalloc((void **)&s.px, (size_t)n * 4))) return e;
        return hipSuccess;
    };
    Soa st, q;
    CHECK(alloc_soa(st)); CHECK(alloc_soa(q));
    uint4 *rec; uint32_t *to_of, *src;
    CHECK(hipMalloc((void **)&rec, (size_t)n * 64));
    CHECK(hipMalloc((void **)&to_of, (size_t)n * 4));
    CHECK(hipMalloc((void **)&src, (size_t)n * 4));
    CHECK(hipMemcpy(to_of, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1, e2;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1)); CHECK(hipEventCreate(&e2));
    const dim3 grid((n + 255u) / 256u), sgrid(std::min((n + 255u) / 256u, 16384u));
    std::vector<float> ta, tb_place, tb_gather, tc_place, tc_gather;
    for (int r = 0; r < reps + 3; ++r) {
        float m0, m1;
        // (a)
        hipLaunchKernelGGL(fill_soa, grid, dim3(256), 0, 0, q, n, 0xA000u + r);
        hipLaunchKernelGGL(fill_soa, grid, dim3(256), 0, 0, st, n, 0xB000u + r);
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(move_scatter, sgrid, dim3(256), 0, 0, st, q, to_of, n);
        CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&m0, e0, e1));
        if (r >= 3) ta.push_back(m0);
        // (b)
        hipLaunchKernelGGL(fill_soa, grid, dim3(256), 0, 0, q, n, 0xC000u + r);
        hipLaunchKernelGGL(fill_soa, grid, dim3(256), 0, 0, st, n, 0xD000u + r);
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(place, sgrid, dim3(256), 0, 0, src, to_of, n);
        CHECK(hipEventRecord(e1));
        hipLaunchKernelGGL(gather_soa, grid, dim3(256), 0, 0, st, q, src, n);
        CHECK(hipEventRecord(e2)); CHECK(hipEventSynchronize(e2));
        CHECK(hipEventElapsedTime(&m0, e0, e1)); CHECK(hipEventElapsedTime(&m1, e1, e2));
        if (r >= 3) { tb_place.push_back(m0); tb_gather.push_back(m1); }
        // (c)
        hipLaunchKernelGGL(fill_soa, grid, dim3(256), 0, 0, q, n, 0xE000u + r);
        hipLaunchKernelGGL(fill_aos, grid, dim3(256), 0, 0, rec, st.px, n, 0xF000u + r);
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(place, sgrid, dim3(256), 0, 0, src, to_of, n);
        CHECK(hipEventRecord(e1));
        hipLaunchKernelGGL(gather_aos, grid, dim3(256), 0, 0, rec, st.px, q, src, n);
        CHECK(hipEventRecord(e2)); CHECK(hipEventSynchronize(e2));
        CHECK(hipEventElapsedTime(&m0, e0, e1)); CHECK(hipEventElapsedTime(&m1, e1, e2));
        if (r >= 3) { tc_place.push_back(m0); tc_gather.push_back(m1); }
    }
    CHECK(hipGetLastError());
    // the moves are the same permutation: spot-check the last (c) result against the record tags
    std::vector<uint4> qa(n);
    CHECK(hipMemcpy(qa.data(), q.a, (size_t)n * 16, hipMemcpyDeviceToHost));
    uint32_t bad = 0;
    for (uint32_t i = 0; i < n; ++i) if (qa[perm[i]].x != i) ++bad;
    const double mb = (double)n * 68.0 / 1e6;
    std::printf("n = %u records of 68 B (%.1f MB), random permutation, %d reps, medians (ms); wrong records after (c): %u\n", n, mb, reps, bad);
    const double a = median(ta), bp = median(tb_place), bg = median(tb_gather), cp = median(tc_place), cg = median(tc_gather);
    std::printf("(a) scatter, 5 SoA streams             : %.4f ms  (%.2f TB/s of ray bytes moved)\n", a, mb / a / 1e3);
    std::printf("(b) place %.4f + gather SoA %.4f      = %.4f ms  (%.2fx of (a))\n", bp, bg, bp + bg, (bp + bg) / a);
    std::printf("(c) place %.4f + gather AoS+px %.4f   = %.4f ms  (%.2fx of (a))\n", cp, cg, cp + cg, (cp + cg) / a);
    std::printf("min / max: (a) %.4f / %.4f  (b) gather %.4f / %.4f  (c) gather %.4f / %.4f  place %.4f / %.4f\n",
                *std::min_element(ta.begin(), ta.end()), *std::max_element(ta.begin(), ta.end()),
                *std::min_element(tb_gather.begin(), tb_gather.end()), *std::max_element(tb_gather.begin(), tb_gather.end()),
                *std::min_element(tc_gather.begin(), tc_gather.end()), *std::max_element(tc_gather.begin(), tc_gather.end()),
                *std::min_element(tb_place.begin(), tb_place.end()), *std::max_element(tb_place.begin(), tb_place.end()));
    return bad ? 2 : 0;
}
