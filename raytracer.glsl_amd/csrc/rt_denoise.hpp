// rt_denoise.hpp -- edge-avoiding a-trous filter over the accumulation image, guided by the first-hit planes (rtgl_denoise; the contract
// is in include/rtgl_amd.h, the reasoning in DESIGN.md 5.4).  No reference counterpart.
//
// The filter is defined operation by operation (binary32, one rounding each, no contraction, correctly rounded divide) so that a numpy
// restatement (tests/denoise_mirror.py) gives the same bits; nothing here may be reassociated, fused or replaced by an approximation.
//
// One filtering kernel, the staged form: a block of four waves takes 64 columns of four rows `step` apart and walks the eight tap rows
// they share through LDS (below).  The direct form -- every lane loading its 25 taps' records from global memory, 75 16-byte loads per
// pixel and pass -- was built first, gave the same bits and was dropped for being slower: both timings are in DESIGN.md 5.4.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.hpp"
#include "rt_wavefront.hpp"

#pragma clang fp contract(off)

namespace rt {

struct AtrousArgs {
    const float4 *src;        // colour of the previous pass (RGBA32F; the accumulation image for the first pass)
    const float4 *albedo;     // first-hit planes; a plane the parameters do not need may be NULL and is never read
    const float4 *normal;
    const float4 *position;
    float4 *dst;
    int32_t width, height;    // all local pixels
    int32_t step;             // 2^L
    int32_t step_log2;        // L
    float inv_color;          // 1 / (sig sig), sig = sigma_color 2^-L
    float inv_normal;         // 1 / (sigma_normal sigma_normal)
    float sigma_position;
    uint32_t use_color, use_normal, use_position;      // 0: the term is switched off (its sigma <= 0) and its factor skipped
};

constexpr float kAtrousAlbedoFloor = 0.0009765625f;     // 2^-10

// (1 - x/4)^4 for x < 4, else 0 (a NaN gives 0): the compact stand-in for exp(-x)
__device__ __forceinline__ float atrous_ew(float x)
{
    float q = (x < 4.0f) ? 1.0f - 0.25f * x : 0.0f;
    q = q * q;
    return q * q;
}
__device__ __forceinline__ float atrous_dot3(float x, float y, float z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ f3 atrous_divisor(const float4 &a)
{
    return mk(a.x > kAtrousAlbedoFloor ? a.x : kAtrousAlbedoFloor, a.y > kAtrousAlbedoFloor ? a.y : kAtrousAlbedoFloor, a.z > kAtrousAlbedoFloor ? a.z : kAtrousAlbedoFloor);
}

// passes = 0: no filtering, only the copy (kDemod = false: the identity, bit for bit) or the demodulation round trip c / d * d
template <bool kDemod>
__global__ void __launch_bounds__(256) atrous_identity_kernel(AtrousArgs a)
{
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= (size_t)a.width * (size_t)a.height) return;
    const float4 v = a.src[p];
    f3 c = mk(v.x, v.y, v.z);
    if (kDemod) { const f3 d = atrous_divisor(a.albedo[p]); c = mk(c.x / d.x, c.y / d.y, c.z / d.z); c = mk(c.x * d.x, c.y * d.y, c.z * d.z); }
    store_through(a.dst + p, c.x, c.y, c.z, v.w);                      // (read by the caller: rt_wavefront.hpp, store_through)
}

// One pass.  kDemod: `src` is the accumulation image and every colour read from it is divided by its pixel's albedo first (the first
// pass of a demodulating call); kRemod: the result is multiplied by the pixel's albedo (its last pass).
// A block takes 64 columns of four rows `step` apart (rows Y0 + k step, one per wave).  Their taps lie in eight tap rows
// Y0 + (m - 2) step, m = 0..7, and the five taps of a row are shifts of one segment of 64 + 4 step pixels.  The block walks the eight
// tap rows: the segment of row m + 1 is loaded from global memory while the waves take their taps of row m from LDS (wave k uses rows
// m = k .. k + 4 as its j = -2 .. 2, so the accumulation order is the contract's); two LDS buffers, one barrier per row.  A block asks
// global memory for 8 (64 + 4 step) pixel records where the direct form asked for 6,400: a twelfth at step 1, a sixth at step 16.
// LDS image of a segment: nine arrays of 64 + 4 step floats (colour after demodulation, normal.xyz, position.xyz); lane l reads word
// l + const of an array: conflict free.  A column outside the image is never staged: its LDS words are stale and the tap that reads
// them is dropped.  kWide: segments of more than 256 pixels (step 64 and 128), up to three records per thread.
template <bool kDemod, bool kRemod, bool kWide>
__global__ void __launch_bounds__(256) atrous_kernel(AtrousArgs a)
{
    extern __shared__ float seg[];                                   // [2][9][wt]
    constexpr int kRecs = kWide ? 3 : 1;
    const int s = a.step, wt = 64 + 4 * s;
    const int tid = (int)threadIdx.x, lane = tid & 63, k = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x0 = (int)blockIdx.x * 64;
    const int chunk = (int)blockIdx.y >> a.step_log2, Y0 = 4 * s * chunk + ((int)blockIdx.y & (s - 1));
    if (Y0 >= a.height) return;                                      // (block-uniform, in front of every barrier)
    const int x = x0 + lane, y = Y0 + k * s;
    const bool live = x < a.width && y < a.height;
    float4 ip4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    f3 d = mk(1.0f, 1.0f, 1.0f), c = mk(0.0f, 0.0f, 0.0f), n = mk(0.0f, 0.0f, 0.0f), pos = mk(0.0f, 0.0f, 0.0f);
    float inv_pos = 0.0f;
    const size_t p = live ? (size_t)y * (size_t)a.width + (size_t)x : 0;
    if (live) {
        ip4 = a.src[p];
        if (kDemod || kRemod) d = atrous_divisor(a.albedo[p]);
        c = mk(ip4.x, ip4.y, ip4.z);
        if (kDemod) c = mk(c.x / d.x, c.y / d.y, c.z / d.z);
        if (a.use_normal) { const float4 v = a.normal[p]; n = mk(v.x, v.y, v.z); }
        if (a.use_position) {
            const float4 v = a.position[p];
            pos = mk(v.x, v.y, v.z);
            const float sp = a.sigma_position * v.w;
            inv_pos = (sp > 0.0f) ? 1.0f / (sp * sp) : 0.0f;
        }
    }
    float4 rc[kRecs], ra[kRecs], rn[kRecs], rp[kRecs];
    auto load_row = [&](int m) {
        const int ty = Y0 + (m - 2) * s;
        if (ty < 0 || ty >= a.height) return;
#pragma unroll
        for (int u = 0; u < kRecs; ++u) {
            const int col = tid + 256 * u, qx = x0 - 2 * s + col;
            if (col < wt && qx >= 0 && qx < a.width) {
                const size_t q = (size_t)ty * (size_t)a.width + (size_t)qx;
                rc[u] = a.src[q];
                if (kDemod) ra[u] = a.albedo[q];
                if (a.use_normal) rn[u] = a.normal[q];
                if (a.use_position) rp[u] = a.position[q];
            }
        }
    };
    auto store_row = [&](int m) {
        const int ty = Y0 + (m - 2) * s;
        if (ty < 0 || ty >= a.height) return;
        float *b = seg + (m & 1) * 9 * wt;
#pragma unroll
        for (int u = 0; u < kRecs; ++u) {
            const int col = tid + 256 * u, qx = x0 - 2 * s + col;
            if (col < wt && qx >= 0 && qx < a.width) {
                f3 t = mk(rc[u].x, rc[u].y, rc[u].z);
                if (kDemod) { const f3 dq = atrous_divisor(ra[u]); t = mk(t.x / dq.x, t.y / dq.y, t.z / dq.z); }
                b[col] = t.x; b[wt + col] = t.y; b[2 * wt + col] = t.z;
                if (a.use_normal) { b[3 * wt + col] = rn[u].x; b[4 * wt + col] = rn[u].y; b[5 * wt + col] = rn[u].z; }
                if (a.use_position) { b[6 * wt + col] = rp[u].x; b[7 * wt + col] = rp[u].y; b[8 * wt + col] = rp[u].z; }
            }
        }
    };
    f3 acc = mk(0.0f, 0.0f, 0.0f);
    float ws = 0.0f;
    load_row(0);
    store_row(0);
    __syncthreads();
#pragma unroll 1
    for (int m = 0; m < 8; ++m) {
        if (m < 7) load_row(m + 1);
        const int j = m - 2 - k, ty = Y0 + (m - 2) * s;
        if (live && j >= -2 && j <= 2 && ty >= 0 && ty < a.height) {
            const float hj = (j == 0) ? 0.375f : ((j == -1 || j == 1) ? 0.25f : 0.0625f);
            const float *b = seg + (m & 1) * 9 * wt + lane + 2 * s;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int o = (i - 2) * s, qx = x + o;
                const float hi = (i == 2) ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f);
                const f3 t = mk(b[o], b[wt + o], b[2 * wt + o]);
                float w = hj * hi;
                if (a.use_color) w = w * atrous_ew(atrous_dot3(t.x - c.x, t.y - c.y, t.z - c.z) * a.inv_color);
                if (a.use_normal) w = w * atrous_ew(atrous_dot3(b[3 * wt + o] - n.x, b[4 * wt + o] - n.y, b[5 * wt + o] - n.z) * a.inv_normal);
                if (a.use_position) w = w * atrous_ew(atrous_dot3(b[6 * wt + o] - pos.x, b[7 * wt + o] - pos.y, b[8 * wt + o] - pos.z) * inv_pos);
                if (qx >= 0 && qx < a.width && w > 0.0f) {
                    acc = mk(acc.x + w * t.x, acc.y + w * t.y, acc.z + w * t.z);
                    ws = ws + w;
                }
            }
        }
        if (m < 7) store_row(m + 1);
        __syncthreads();
    }
    if (!live) return;
    f3 out = c;
    if (ws > 0.0f) out = mk(acc.x / ws, acc.y / ws, acc.z / ws);
    if (kRemod) out = mk(out.x * d.x, out.y * d.y, out.z * d.z);
    store_through(a.dst + p, out.x, out.y, out.z, ip4.w);               // (read by the next pass / the caller: rt_wavefront.hpp, store_through)
}

}  // namespace rt
