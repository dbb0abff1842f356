// rt_adaptive.hpp -- adaptive sampling: masked frames over the tiles that are still noisy.  The contract is in include/rtgl_amd.h
// ("adaptive sampling"), the derivation and the figures in DESIGN.md 5.11, the host half (mask rule, block list) in rt_adaptive_plan.hpp.
// No reference counterpart.
//
// A masked frame is the ordinary per-bounce pipeline behind generate_rays_masked_kernel, whose queue 0 holds the 8 x 8 blocks of a list
// instead of all of them; the pipeline traces into a sample buffer as a one-frame image (reset_flag = 1, frames = 0), and
// adaptive_merge_kernel folds that buffer into the image with the count of each tile.  adaptive_tiles_kernel is error_tiles_kernel with a
// snapshot count per tile.  A tile has one owner in both: no global atomics.  The float arithmetic is defined operation by operation
// (rt_error.hpp) so that tests/adaptive_mirror.py gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.hpp"
#include "rt_wavefront.hpp"
#include "rt_error.hpp"

#pragma clang fp contract(off)

namespace rt {

// generate_rays_kernel's full (not lean), sample-0, single-frame form with the block indirection: slot idx of queue 0 is pixel
// (in & 7, in >> 3) of block list[idx >> 6], in = idx & 63; n0 = 64 x the list's length.  The chores of that kernel for the ray counts,
// the scan's work counters and the count of bounce 0 are done here in the same way.  Seed and camera ray come from the absolute pixel
// coordinates (camera_slot_ray), so a pixel's sample does not depend on the list.  Untiled contexts only: local row = global row.
__global__ void __launch_bounds__(256) generate_rays_masked_kernel(FrameParams P, ImageView im, WaveBuffers wb, const uint32_t *__restrict__ list, uint32_t n0, Counters *counters,
                                                                   uint32_t n_counts, uint32_t n_sched)
{
    if (blockIdx.x == 0 && threadIdx.x < n_counts && threadIdx.x > 0u) store_through(wb.counts + threadIdx.x, 0u);
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx < n_sched) store_through(wb.sched + idx, 0u);
    if (idx >= n0) return;
    if (idx == 0u) {
        store_through(wb.counts, n0);
        if (counters) store_through(&counters->paths, (unsigned long long)n0);      // (the host has zeroed the counters; nothing else of a frame adds to this one)
    }
    const uint32_t blocks_x = (uint32_t)im.disp_w >> 3;
    const uint32_t blk = list[idx >> 6], in = idx & 63u;
    const int px = (int)((blk % blocks_x) * 8u + (in & 7u)), py = (int)((blk / blocks_x) * 8u + (in >> 3));
    PathState s;
    s.pixel = (uint32_t)py * (uint32_t)im.width + (uint32_t)px;
    camera_slot_ray(P, im, px, py, s);
    s.thr = mk(1.0f, 1.0f, 1.0f); s.rad = mk(0.0f, 0.0f, 0.0f);
    store_ray(wb.q[0], idx, s, true);
    if (wb.best[0]) store_through(wb.best[0] + idx, 0xFFFFFFFFFFFFFFFFull);
}

struct AdaptiveMergeArgs {
    float4 *image;
    const float4 *samples;                // the one-frame image the masked frame traced
    uint32_t *n;                          // samples per tile
    const uint32_t *tiles;                // the active tiles, one block each
    int32_t width, fw, fh, tx;
};

// One block per active tile, thread = row-major index of the tile: a row of 16 lanes loads 256 contiguous bytes of either buffer.
// v = (x + prev k) / (k + 1), accumulate_pixel's operations with frames = k = the tile's count, which thread 0 then raises.
__global__ void __launch_bounds__(256) adaptive_merge_kernel(AdaptiveMergeArgs a)
{
    const int tid = (int)threadIdx.x;
    const uint32_t t = a.tiles[blockIdx.x];
    const int x = (int)(t % (uint32_t)a.tx) * kErrTile + (tid & 15), y = (int)(t / (uint32_t)a.tx) * kErrTile + (tid >> 4);
    const uint32_t k = error_load(a.n + t);
    __syncthreads();                                                   // (every thread has the count before thread 0 replaces it)
    if (x < a.fw && y < a.fh) {
        const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
        const float4 s = a.samples[i], prev = a.image[i];
        const float fk = (float)k, fk1 = (float)(k + 1u);
        store_through(a.image + i, (s.x + prev.x * fk) / fk1, (s.y + prev.y * fk) / fk1, (s.z + prev.z * fk) / fk1, 1.0f);      // (read by the next call and the caller: rt_wavefront.hpp, store_through)
    }
    if (tid == 0) store_through(a.n + t, k + 1u);
}

struct AdaptiveTilesArgs {
    const float4 *image;
    float *snapshot;                      // one float per pixel: lum of the image when the tile's snapshot was taken
    uint4 *records;                       // tx x ty records of two uint4: {sum, mse, count, converged}, {n, m, 0, 0}
    const uint32_t *n;                    // samples per tile
    uint32_t *m;                          // samples per tile when its snapshot was taken (0: none)
    int32_t width, fw, fh;
    float floor_, threshold;
};

// One block per tile, laid out like error_tiles_kernel and with its tree.  A tile whose count has not moved since its snapshot keeps
// record and snapshot (n == m: the block leaves at once); without a snapshot (m == 0) one is taken and the record is not valid.
__global__ void __launch_bounds__(256) adaptive_tiles_kernel(AdaptiveTilesArgs a)
{
    __shared__ float ps[4];
    __shared__ uint32_t pc[4];
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * kErrTile + (tid & 15), y = (int)blockIdx.y * kErrTile + (tid >> 4);
    const size_t t = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const uint32_t n = error_load(a.n + t), m = error_load(a.m + t);
    if (n == m) return;                                                // (uniform)
    float e = 0.0f;                                                    // (positions outside the footprint and pixels that do not count: +0)
    bool counts = false;
    if (x < a.fw && y < a.fh) {
        const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
        const float4 px = a.image[i];
        const float Ln = error_lum(px.x, px.y, px.z);
        if (m) {
            const float Lm = __uint_as_float(error_load(reinterpret_cast<const uint32_t *>(a.snapshot + i)));
            const float d = Ln - Lm;
            const float den = ((Ln > 0.0f) ? Ln : 0.0f) + a.floor_;
            const float q = d / den;
            const float qq = q * q;
            counts = (qq - qq == 0.0f);
            e = counts ? qq : 0.0f;
        }
        store_through(reinterpret_cast<uint32_t *>(a.snapshot + i), __float_as_uint(Ln));
    }
    const float s = error_wave_tree(e);
    const uint32_t cnt = (uint32_t)__popcll(__ballot(counts));
    if ((tid & 63) == 0) { ps[tid >> 6] = s; pc[tid >> 6] = cnt; }
    __syncthreads();                                                   // (and every thread has m before thread 0 replaces it)
    if (tid != 0) return;
    const float sum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
    const uint32_t count = (pc[0] + pc[1]) + (pc[2] + pc[3]);
    uint4 *rec = a.records + 2u * t;
    if (count) {
        const float c = (float)m / (float)(n - m);
        const float mse = (sum / (float)count) * c;
        store_through(rec, __float_as_uint(sum), __float_as_uint(mse), count, (mse <= a.threshold * a.threshold) ? 1u : 0u);
    } else store_through(rec, 0u, 0u, 0u, 0u);
    store_through(rec + 1, n, n, 0u, 0u);
    store_through(a.m + t, n);
}

}  // namespace rt
