// rt_robust.hpp -- robust accumulation: the frames dealt round-robin into K bucket means, and a resolve that drops the buckets that
// disagree with the others (median of means with a Gini-adaptive trim).  The contract is in include/rtgl_amd.h ("robust accumulation"),
// the derivation and the figures in DESIGN.md 5.12, the host half (bucket of the next frame, counts, validation, sizes) in
// rt_robust_plan.hpp.  No reference counterpart.
//
// Both kernels stream: one lane per pixel of the context's rows, no neighbourhood, no LDS, no atomics.  The fold reads the image and
// one bucket plane and writes that plane (48 B per pixel); the resolve reads the K planes and writes one (16 K + 16 B per pixel).  The
// float arithmetic is defined operation by operation (rt_error.hpp) so that tests/robust_mirror.py gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.hpp"
#include "rt_wavefront.hpp"
#include "rt_error.hpp"

#pragma clang fp contract(off)

namespace rt {

// b' = (x + b k) / (k + 1) per component, w like a colour: accumulate_pixel's operations in adaptive_merge_kernel's order, with the
// image as it stands for x and k = the samples the bucket holds.  `bucket` is the plane's base and k a kernel argument: both scalars.
__global__ void __launch_bounds__(256) robust_accumulate_kernel(const float4 *__restrict__ image, float4 *__restrict__ bucket, uint32_t k, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 x = image[i], b = bucket[i];
    const float fk = (float)k, fk1 = (float)(k + 1u);
    store_through(bucket + i, (x.x + b.x * fk) / fk1, (x.y + b.y * fk) / fk1, (x.z + b.z * fk) / fk1, (x.w + b.w * fk) / fk1);      // (read by the next fold of this bucket and by the resolve: rt_wavefront.hpp, store_through)
}

struct RobustResolveArgs {
    const float4 *buckets;                // K planes of `plane` pixels, bucket-major
    float4 *out;                          // kDest 0: the output plane {r, g, b, G}; kDest 1: the accumulation image {r, g, b, w}
    size_t plane;
    uint32_t n;                           // pixels of a plane that are the context's rows
    uint32_t frames;                      // N >= 1
    float gain;
};

__device__ __forceinline__ bool robust_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// One lane per pixel; the K loads first, then everything on registers: every loop below has constant bounds and is unrolled, so that no
// array is indexed at run time.  Steps 1-9 of the header, in its order and with its names.
template <int K, int kDest>
__global__ void __launch_bounds__(256) robust_resolve_kernel(RobustResolveArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    float4 b[K];
#pragma unroll
    for (int j = 0; j < K; ++j) b[j] = a.buckets[(size_t)j * a.plane + i];
    float key[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float l = error_lum(b[j].x, b[j].y, b[j].z);
        key[j] = robust_finite(l) ? l : __uint_as_float(0x7F800000u);
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
    if (!robust_finite(S)) G = 1.0f;
    else if (!(S > 0.0f)) G = 0.0f;
    else G = A / ((float)K * S);
    if (!(G <= 1.0f)) G = 1.0f;
    if (!(G >= 0.0f)) G = 0.0f;
    const float u = (G * a.gain) * (float)(K / 2);
    constexpr int cap = (K - 1) / 2;
    int t = (u >= (float)cap) ? cap : (int)u;
    if (a.frames < (uint32_t)K) t = 0;                                 // (uniform)
    const uint32_t q = a.frames / (uint32_t)K, rem = a.frames % (uint32_t)K;
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

}  // namespace rt
