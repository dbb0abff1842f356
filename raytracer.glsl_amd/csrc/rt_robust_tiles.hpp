// rt_robust_tiles.hpp -- a robust adaptive session: masked frames folded into K bucket means with a sample count per 16 x 16 tile, the
// estimate of the tiles whose count has moved, and a resolve that takes each pixel's N from its tile.  The contract is in
// include/rtgl_amd.h ("robust adaptive sampling"), the derivation and the figures in DESIGN.md 5.16, the host half (validation, counts,
// sizes) in rt_robust_tiles_plan.hpp; shapes, mask rule, lists and summary are rt_adaptive_plan.hpp's.  No reference counterpart.
//
// All three kernels are one block of 256 per tile, thread = row-major index of the tile, so that a row of 16 lanes moves 256 contiguous
// bytes of a plane; a tile has one owner: no global atomics.  The fold moves 48 B per active pixel.  The arithmetic is RESTATED from
// robust_accumulate_kernel, robust_resolve_kernel and spread_tiles_kernel, not shared with them: those headers stay what they are.  The
// float arithmetic is defined operation by operation (rt_error.hpp) so that tests/robust_adaptive_mirror.py gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.hpp"
#include "rt_wavefront.hpp"
#include "rt_error.hpp"

#pragma clang fp contract(off)

namespace rt {

struct TileBucketsFoldArgs {
    const float4 *source;                 // the sample buffer of a masked frame, or the accumulation image
    float4 *buckets;                      // K planes of `plane` pixels, bucket-major
    size_t plane;
    uint32_t *n;                          // samples per tile
    const uint32_t *tiles;                // the active tiles, one block each
    uint32_t K;
    int32_t width, fw, fh, tx;
};

// b' = (x + b k) / (k + 1) per component, w like a colour, with j = n mod K and k = n div K of the block's tile: both wave-uniform.
// Thread 0 then raises the count.
__global__ void __launch_bounds__(256) tile_buckets_fold_kernel(TileBucketsFoldArgs a)
{
    const int tid = (int)threadIdx.x;
    const uint32_t t = a.tiles[blockIdx.x];
    const int x = (int)(t % (uint32_t)a.tx) * kErrTile + (tid & 15), y = (int)(t / (uint32_t)a.tx) * kErrTile + (tid >> 4);
    const uint32_t n = error_load(a.n + t);
    __syncthreads();                                                   // (every thread has the count before thread 0 replaces it)
    const uint32_t j = n % a.K, k = n / a.K;
    if (x < a.fw && y < a.fh) {
        const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
        float4 *bucket = a.buckets + (size_t)j * a.plane;
        const float4 s = a.source[i], b = bucket[i];
        const float fk = (float)k, fk1 = (float)(k + 1u);
        store_through(bucket + i, (s.x + b.x * fk) / fk1, (s.y + b.y * fk) / fk1, (s.z + b.z * fk) / fk1, (s.w + b.w * fk) / fk1);      // (read by the next fold of this bucket, the update and the resolve: rt_wavefront.hpp, store_through)
    }
    if (tid == 0) store_through(a.n + t, n + 1u);
}

struct TileBucketsResolveArgs {
    const float4 *buckets;                // K planes of `plane` pixels, bucket-major
    float4 *out;                          // kDest 0: the output plane {r, g, b, G}; kDest 1: the accumulation image {r, g, b, w}
    size_t plane;
    const uint32_t *n;                    // samples per tile
    int32_t width, height, fw, fh;
    float gain;
};

__device__ __forceinline__ bool tile_buckets_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
// min(max(v, lo), hi) as two selections (the keys are never a NaN; a zero keeps the sign it came with)
__device__ __forceinline__ float tile_buckets_clamp(float v, float lo, float hi) { const float w = (v < lo) ? lo : v; return (w > hi) ? hi : w; }

// One block per tile of the tx x ty grid, every pixel of the image: N = n[t] is uniform per block, so that the n_j are scalars.  A pixel
// outside the footprint or of a tile without a sample gets +0 in all four components.  Otherwise steps 1-9 of rtgl_robust_resolve with
// that N: the K loads first, then everything on registers, every loop with constant bounds and unrolled, no array indexed at run time.
template <int K, int kDest>
__global__ void __launch_bounds__(256) tile_buckets_resolve_kernel(TileBucketsResolveArgs a)
{
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * kErrTile + (tid & 15), y = (int)blockIdx.y * kErrTile + (tid >> 4);
    if (x >= a.width || y >= a.height) return;
    const uint32_t N = error_load(a.n + ((size_t)blockIdx.y * gridDim.x + blockIdx.x));
    const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
    if (N == 0u || x >= a.fw || y >= a.fh) { store_through(a.out + i, 0.0f, 0.0f, 0.0f, 0.0f); return; }
    float4 b[K];
#pragma unroll
    for (int j = 0; j < K; ++j) b[j] = a.buckets[(size_t)j * a.plane + i];
    float key[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float l = error_lum(b[j].x, b[j].y, b[j].z);
        key[j] = tile_buckets_finite(l) ? l : __uint_as_float(0x7F800000u);
    }
    int rank[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        int r = 0;
#pragma unroll
        for (int m = 0; m < K; ++m)
            if (m != j) r += (key[m] < key[j] || (key[m] == key[j] && m < j)) ? 1 : 0;
        rank[j] = r;
    }
    float S = 0.0f, A = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        S = S + key[j];
        A = A + (float)(2 * rank[j] - (K - 1)) * key[j];
    }
    float G;
    if (!tile_buckets_finite(S)) G = 1.0f;
    else if (!(S > 0.0f)) G = 0.0f;
    else G = A / ((float)K * S);
    if (!(G <= 1.0f)) G = 1.0f;
    if (!(G >= 0.0f)) G = 0.0f;
    const float u = (G * a.gain) * (float)(K / 2);
    constexpr int cap = (K - 1) / 2;
    int t = (u >= (float)cap) ? cap : (int)u;
    if (N < (uint32_t)K) t = 0;                                        // (uniform)
    const uint32_t q = N / (uint32_t)K, rem = N % (uint32_t)K;
    float W = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f, cw = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t nj = q + ((uint32_t)j < rem ? 1u : 0u);
        if (nj > 0u && t <= rank[j] && rank[j] <= K - 1 - t) {
            const float fn = (float)nj;
            W = W + fn;
            cx = cx + fn * b[j].x; cy = cy + fn * b[j].y; cz = cz + fn * b[j].z; cw = cw + fn * b[j].w;
        }
    }
    store_through(a.out + i, cx / W, cy / W, cz / W, kDest ? cw / W : G);      // (read by the caller and by whatever takes the image next)
}

struct TileBucketsEstimateArgs {
    const float4 *buckets;                // K planes of `plane` pixels, bucket-major
    uint4 *records;                       // tx x ty records of two uint4: {sum, mse, count, converged}, {n, m, 0, 0}
    const uint32_t *n;                    // samples per tile
    uint32_t *m;                          // samples per tile when its record was made
    size_t plane;
    int32_t width, fw, fh;
    float gain, floor_, threshold;
};

// One block per tile.  A tile whose count has not moved since its record was made keeps it (n == m: the block leaves at once, having read
// two words).  With fewer samples than buckets the record is {0, 0, 0, 0, n, n}: not valid.  Otherwise steps 1-9 of
// rtgl_robust_error_estimate per footprint pixel (n >= K, so t is not zeroed), the tile's sum by error_wave_tree and 32 bytes of LDS.
template <int K>
__global__ void __launch_bounds__(256) tile_buckets_estimate_kernel(TileBucketsEstimateArgs a)
{
    __shared__ float ps[4];
    __shared__ uint32_t pc[4];
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * kErrTile + (tid & 15), y = (int)blockIdx.y * kErrTile + (tid >> 4);
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const uint32_t n = error_load(a.n + tile), m = error_load(a.m + tile);
    if (n == m) return;                                                // (uniform)
    float e = 0.0f;                                                    // (positions outside the footprint and pixels that do not count: +0)
    bool counts = false;
    if (n >= (uint32_t)K && x < a.fw && y < a.fh) {
        const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
        float4 b[K];
#pragma unroll
        for (int j = 0; j < K; ++j) b[j] = a.buckets[(size_t)j * a.plane + i];
        float key[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float l = error_lum(b[j].x, b[j].y, b[j].z);
            key[j] = tile_buckets_finite(l) ? l : __uint_as_float(0x7F800000u);
        }
        int rank[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            int r = 0;
#pragma unroll
            for (int q = 0; q < K; ++q)
                if (q != j) r += (key[q] < key[j] || (key[q] == key[j] && q < j)) ? 1 : 0;
            rank[j] = r;
        }
        float S = 0.0f, A = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            S = S + key[j];
            A = A + (float)(2 * rank[j] - (K - 1)) * key[j];
        }
        float G;
        if (!tile_buckets_finite(S)) G = 1.0f;
        else if (!(S > 0.0f)) G = 0.0f;
        else G = A / ((float)K * S);
        if (!(G <= 1.0f)) G = 1.0f;
        if (!(G >= 0.0f)) G = 0.0f;
        const float u = (G * a.gain) * (float)(K / 2);
        constexpr int cap = (K - 1) / 2;
        const int t = (u >= (float)cap) ? cap : (int)u;
        float lo = 0.0f, hi = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            lo = (rank[j] == t) ? key[j] : lo;
            hi = (rank[j] == K - 1 - t) ? key[j] : hi;
        }
        float M = 0.0f, T = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            M = M + tile_buckets_clamp(key[j], lo, hi);
            if (t <= rank[j] && rank[j] <= K - 1 - t) T = T + key[j];
        }
        const float mw = M / (float)K;
        float D = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float d = tile_buckets_clamp(key[j], lo, hi) - mw;
            D = D + d * d;
        }
        const int h = K - 2 * t;
        const float mu = T / (float)h;
        const float v = D / (float)(h * (h - 1));
        const float den = ((mu > 0.0f) ? mu : 0.0f) + a.floor_;
        const float q = v / (den * den);
        counts = (q - q == 0.0f);                                      // (finite: a NaN or an infinity anywhere on the way ends here)
        e = counts ? q : 0.0f;
    }
    const float s = error_wave_tree(e);
    const uint32_t cnt = (uint32_t)__popcll(__ballot(counts));
    if ((tid & 63) == 0) { ps[tid >> 6] = s; pc[tid >> 6] = cnt; }
    __syncthreads();                                                   // (and every thread has m before thread 0 replaces it)
    if (tid != 0) return;
    const float sum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
    const uint32_t count = (pc[0] + pc[1]) + (pc[2] + pc[3]);
    uint4 *rec = a.records + 2u * tile;
    if (count) {
        const float mse = sum / (float)count;
        store_through(rec, __float_as_uint(sum), __float_as_uint(mse), count, (mse <= a.threshold * a.threshold) ? 1u : 0u);      // (read by the caller)
    } else store_through(rec, 0u, 0u, 0u, 0u);
    store_through(rec + 1, n, n, 0u, 0u);
    store_through(a.m + tile, n);
}

}  // namespace rt
