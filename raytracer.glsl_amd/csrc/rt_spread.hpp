// rt_spread.hpp -- rtgl_robust_error_estimate: the noise level of the picture a robust session's resolve makes, per 16 x 16 tile, from the
// spread of the K bucket means (Yuen's standard error of a trimmed mean over the winsorized luminances).  The contract is in
// include/rtgl_amd.h ("robust error estimate"), the derivation and the figures in DESIGN.md 5.13, the host half (validation, counts, sizes)
// in rt_spread_plan.hpp.  No reference counterpart.
//
// The shape is error_tiles_kernel's (rt_error.hpp): one block of 256 per tile, thread t = row-major index t, a row of 16 lanes reads 256
// contiguous bytes of each plane; the tile's sum by error_wave_tree and 32 bytes of LDS, one owner per tile, no global atomics.  The whole
// picture is error_solve_kernel's, launched unchanged behind this one.  One pass: 16 K bytes read per footprint pixel (12 K where the
// loads are narrowed to the three colours), 16 written per tile.  The float arithmetic is defined operation by operation (rt_error.hpp) so
// that tests/robust_error_mirror.py gives the same bits; the keys, ranks, G and t are restated from robust_resolve_kernel, not shared.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.hpp"
#include "rt_wavefront.hpp"
#include "rt_error.hpp"

#pragma clang fp contract(off)

namespace rt {

struct SpreadTilesArgs {
    const float4 *buckets;                // K planes of `plane` pixels, bucket-major
    uint4 *tiles;                         // tx x ty records {sum, mse, count, converged}
    size_t plane;
    int32_t width, fw, fh;                // the planes' row length; the footprint (width / 8 * 8, height / 8 * 8)
    float gain, floor_, threshold;
};

__device__ __forceinline__ bool spread_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
// min(max(v, lo), hi) as two selections (the keys are never a NaN; a zero keeps the sign it came with)
__device__ __forceinline__ float spread_clamp(float v, float lo, float hi) { const float w = (v < lo) ? lo : v; return (w > hi) ? hi : w; }

// Steps 1-9 of the header for one pixel, then the tile's record.  The K loads first, then everything on registers: every loop over the
// buckets has constant bounds and is unrolled, lo and hi are picked by compares, so that no array is indexed at run time.
template <int K>
__global__ void __launch_bounds__(256) spread_tiles_kernel(SpreadTilesArgs a)
{
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * kErrTile + (tid & 15), y = (int)blockIdx.y * kErrTile + (tid >> 4);
    const bool inside = x < a.fw && y < a.fh;
    float e = 0.0f;                                                    // (positions outside the footprint and pixels that do not count: +0)
    bool counts = false;
    if (inside) {
        const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
        float4 b[K];
#pragma unroll
        for (int j = 0; j < K; ++j) b[j] = a.buckets[(size_t)j * a.plane + i];
        float key[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float l = error_lum(b[j].x, b[j].y, b[j].z);
            key[j] = spread_finite(l) ? l : __uint_as_float(0x7F800000u);
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
        if (!spread_finite(S)) G = 1.0f;
        else if (!(S > 0.0f)) G = 0.0f;
        else G = A / ((float)K * S);
        if (!(G <= 1.0f)) G = 1.0f;
        if (!(G >= 0.0f)) G = 0.0f;
        const float u = (G * a.gain) * (float)(K / 2);
        constexpr int cap = (K - 1) / 2;
        const int t = (u >= (float)cap) ? cap : (int)u;                // (N >= K: the host refuses the call otherwise)
        float lo = 0.0f, hi = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            lo = (rank[j] == t) ? key[j] : lo;
            hi = (rank[j] == K - 1 - t) ? key[j] : hi;
        }
        float M = 0.0f, T = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            M = M + spread_clamp(key[j], lo, hi);
            if (t <= rank[j] && rank[j] <= K - 1 - t) T = T + key[j];
        }
        const float mw = M / (float)K;
        float D = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const float d = spread_clamp(key[j], lo, hi) - mw;
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
    __shared__ float ps[4];
    __shared__ uint32_t pc[4];
    const float s = error_wave_tree(e);
    const uint32_t n = (uint32_t)__popcll(__ballot(counts));
    if ((tid & 63) == 0) { ps[tid >> 6] = s; pc[tid >> 6] = n; }
    __syncthreads();
    if (tid == 0) {
        uint4 *rec = a.tiles + ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        const float sum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
        const uint32_t count = (pc[0] + pc[1]) + (pc[2] + pc[3]);
        if (count) {
            const float mse = sum / (float)count;
            store_through(rec, __float_as_uint(sum), __float_as_uint(mse), count, (mse <= a.threshold * a.threshold) ? 1u : 0u);      // (read by error_solve_kernel and by the caller)
        } else store_through(rec, 0u, 0u, 0u, 0u);
    }
}

}  // namespace rt
