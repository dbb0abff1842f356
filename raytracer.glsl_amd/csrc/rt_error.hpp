// rt_error.hpp -- rtgl_error_estimate: the noise level of the accumulation image, per 16 x 16 tile and for the whole picture, and the stop
// rule on top of it.  The contract is in include/rtgl_amd.h ("error estimate"), the derivation in DESIGN.md 5.10.  No reference counterpart:
// the reference renders until somebody saves the picture.
//
// The image at two moments m < n of one accumulation differs by a known multiple of the noise: E[(I_n - I_m)^2] = sigma^2 (n - m) / (n m),
// so the squared relative difference of the luminance to a snapshot taken earlier, averaged over a tile and scaled by m / (n - m), is the
// relative MSE of the image as it stands.  One streaming pass: 16 bytes of image and 4 of snapshot read, 4 written per pixel.
//
// The float arithmetic is defined operation by operation like the denoisers' (binary32, one rounding each, no contraction, correctly
// rounded divide) and the sums are taken in ONE order, a balanced pairwise tree over the 256 row-major indices of a tile, so that the numpy
// restatement (tests/error_mirror.py) gives the same bits.  A tile has one owner: no global atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "rt_device.hpp"
#include "rt_wavefront.hpp"

#pragma clang fp contract(off)

namespace rt {

constexpr int kErrTile = 16;                                           // a tile is 16 x 16 pixels = one block, thread t = row-major index t
constexpr int kErrSummaryWords = 16;                                   // rtgl_error_summary, 64 bytes

__device__ __forceinline__ float error_lum(float r, float g, float b) { return (0.25f * r + 0.5f * g) + 0.25f * b; }
__device__ __forceinline__ uint32_t error_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Levels 1..6 of the tree inside a wave, which holds the row-major indices 64 w .. 64 w + 63 of the tile: neighbours, pairs of
// neighbours, the two quads of a half row, the two halves of a row of 16 lanes (four DPP steps; after each, the lanes of a group all hold
// the group's sum, a + b being b + a bit for bit), then the four rows as (r0 + r1) + (r2 + r3) through scalar registers.  ALL 64 lanes must
// be active.
__device__ __forceinline__ float error_wave_tree(float x)
{
    auto dpp = [](float v, auto ctrl) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xf, 0xf, false)); };
    x = x + dpp(x, std::integral_constant<int, 0xB1>{});               // quad_perm [1,0,3,2]
    x = x + dpp(x, std::integral_constant<int, 0x4E>{});               // quad_perm [2,3,0,1]
    x = x + dpp(x, std::integral_constant<int, 0x141>{});              // row_half_mirror
    x = x + dpp(x, std::integral_constant<int, 0x140>{});              // row_mirror
    auto rl = [&](int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l)); };
    return (rl(0) + rl(16)) + (rl(32) + rl(48));
}

struct ErrorTilesArgs {
    const float4 *image;
    float *snapshot;                      // one float per pixel: the raw lum of the image when the snapshot was taken
    uint4 *tiles;                         // tx x ty records {sum, mse, count, converged}
    int32_t width, fw, fh;                // the image's row length; the footprint (width / 8 * 8, height / 8 * 8)
    float g_n, g_m, c, floor_, threshold;
};

// One block per tile, a wave per 4 rows x 16 columns: a row of 16 lanes loads 256 contiguous bytes of the image.  kEstimate: the tile's
// record from the image and the snapshot; otherwise the record is zeroed (a call without a usable snapshot).  kKeep: the snapshot is left as
// it is; otherwise it becomes the current image's lum.  Levels 7 and 8 of the tree combine the four waves through LDS (32 bytes).
template <bool kEstimate, bool kKeep>
__global__ void __launch_bounds__(256) error_tiles_kernel(ErrorTilesArgs a)
{
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * kErrTile + (tid & 15), y = (int)blockIdx.y * kErrTile + (tid >> 4);
    const bool inside = x < a.fw && y < a.fh;
    float e = 0.0f;                                                    // (positions outside the footprint and pixels that do not count: +0)
    bool counts = false;
    if (inside) {
        const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
        const float4 px = a.image[i];
        const float L = error_lum(px.x, px.y, px.z);
        if constexpr (kEstimate) {
            const float S = __uint_as_float(error_load(reinterpret_cast<const uint32_t *>(a.snapshot + i)));
            const float Ln = L * a.g_n, Lm = S * a.g_m;
            const float d = Ln - Lm;
            const float den = ((Ln > 0.0f) ? Ln : 0.0f) + a.floor_;
            const float q = d / den;
            const float qq = q * q;
            counts = (qq - qq == 0.0f);                                // (finite: a NaN or an infinity anywhere on the way ends here)
            e = counts ? qq : 0.0f;
        }
        if constexpr (!kKeep) store_through(reinterpret_cast<uint32_t *>(a.snapshot + i), __float_as_uint(L));   // (read by the next call: rt_wavefront.hpp, store_through)
    }
    uint4 *rec = a.tiles + ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
    if constexpr (kEstimate) {
        __shared__ float ps[4];
        __shared__ uint32_t pc[4];
        const float s = error_wave_tree(e);
        const uint32_t n = (uint32_t)__popcll(__ballot(counts));
        if ((tid & 63) == 0) { ps[tid >> 6] = s; pc[tid >> 6] = n; }
        __syncthreads();
        if (tid == 0) {
            const float sum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
            const uint32_t count = (pc[0] + pc[1]) + (pc[2] + pc[3]);
            if (count) {
                const float mse = (sum / (float)count) * a.c;
                store_through(rec, __float_as_uint(sum), __float_as_uint(mse), count, (mse <= a.threshold * a.threshold) ? 1u : 0u);
            } else store_through(rec, 0u, 0u, 0u, 0u);
        }
    } else if (tid == 0) store_through(rec, 0u, 0u, 0u, 0u);
}

struct ErrorSolveArgs {
    const uint4 *tiles;
    uint32_t *summary;                    // kErrSummaryWords words (rtgl_error_summary)
    uint32_t n_tiles, valid;              // valid 0: the call took a snapshot only; the summary is zeroed
    int32_t frames_now, frames_snapshot;
    uint32_t footprint, quantile_permille;
    float c;
};

// One block of 256.  Lane t adds the tile sums t, t + 256, ... in ascending order from +0, the same 256-leaf tree combines the lanes; the
// integers (counts, valid and converged tiles) and the maximum (of non-negative floats that are never a NaN: their bits order like the
// values) go through LDS integer operations, whose results do not depend on order.
__global__ void __launch_bounds__(256) error_solve_kernel(ErrorSolveArgs a)
{
    __shared__ float ps[4];
    __shared__ unsigned long long sN;
    __shared__ uint32_t sValid, sConv, sMax;
    const int tid = (int)threadIdx.x;
    uint4 *out = reinterpret_cast<uint4 *>(a.summary);
    if (!a.valid) {                                                    // (uniform)
        if (tid < 4) store_through(out + tid, 0u, 0u, 0u, 0u);
        return;
    }
    if (tid == 0) { sN = 0ull; sValid = 0u; sConv = 0u; sMax = 0u; }
    __syncthreads();
    float s = 0.0f, mx = 0.0f;
    unsigned long long N = 0ull;
    uint32_t nv = 0u, nc = 0u;
    // eight records per trip, all 32 words requested before the first is used: one block reads thousands of records, and a load per
    // add would make the call a chain of memory round trips.  A record past the end is read from the last one and contributes +0 and
    // count 0, which changes no bit (the sums are never -0).
    constexpr uint32_t kAhead = 8u;
    for (uint32_t base = (uint32_t)tid; base < a.n_tiles; base += 256u * kAhead) {
        uint32_t w[kAhead][4];
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) {
            const uint32_t k = base + 256u * j;
            const uint32_t *r = reinterpret_cast<const uint32_t *>(a.tiles + (k < a.n_tiles ? k : a.n_tiles - 1u));
#pragma unroll
            for (int c = 0; c < 4; ++c) w[j][c] = error_load(r + c);
        }
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) {
            const bool in = base + 256u * j < a.n_tiles;
            const uint32_t count = in ? w[j][2] : 0u;
            s = s + (in ? __uint_as_float(w[j][0]) : 0.0f);
            if (count) {
                const float mse = __uint_as_float(w[j][1]);
                N += count; ++nv; nc += w[j][3];
                mx = (mse > mx) ? mse : mx;
            }
        }
    }
    const float ws = error_wave_tree(s);
    if ((tid & 63) == 0) ps[tid >> 6] = ws;
    if (nv) { atomicAdd(&sN, N); atomicAdd(&sValid, nv); atomicAdd(&sConv, nc); atomicMax(&sMax, __float_as_uint(mx)); }
    __syncthreads();
    if (tid != 0) return;
    const float sum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
    const unsigned long long total = sN;
    const float mse = total ? (sum / (float)total) * a.c : 0.0f;
    const uint32_t conv = (sValid > 0u && (unsigned long long)sConv * 1000ull >= (unsigned long long)sValid * (unsigned long long)a.quantile_permille) ? 1u : 0u;
    store_through(out + 0, 1u, conv, (uint32_t)a.frames_now, (uint32_t)a.frames_snapshot);
    store_through(out + 1, sValid, sConv, a.footprint - (uint32_t)total, __float_as_uint(a.c));
    store_through(out + 2, __float_as_uint(mse), sMax, 0u, 0u);
    store_through(out + 3, 0u, 0u, 0u, 0u);
}

}  // namespace rt
