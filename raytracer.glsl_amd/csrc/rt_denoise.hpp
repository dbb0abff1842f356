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

// ---- rtgl_denoise_guided: the same filter with a luminance tolerance that follows a per-pixel variance estimate, and a firefly clamp in
// front (the contract is in include/rtgl_amd.h, "variance-guided denoiser"; the reasoning in DESIGN.md 5.5; restated by
// tests/denoise_guided_mirror.py).  Two kernels: guided_prepare_kernel turns the image into records {c1.rgb, v0} (demodulated, clamped
// colour and the spatial variance of its luminance) and guided_kernel filters such records, the variance riding in the fourth component.

struct GuidedArgs {
    const float4 *image;      // the accumulation image (prepare; the last pass takes its alpha from here)
    const float4 *src;        // records {c.rgb, var} of the previous pass or of the prepare kernel (passes)
    const float4 *albedo;     // first-hit planes; a plane the parameters do not need may be NULL and is never read
    const float4 *normal;
    const float4 *position;
    float4 *dst;              // records for the next pass; for the last pass (or prepare with passes = 0) the denoised image
    float4 *variance;         // {mu, v0, var after the last pass, s0}: written by prepare, its third component again by the last pass
    uint32_t *near;           // per pixel, the neighbours (of its 3 x 3) whose geometric weight is > 0: written by prepare, read by the passes
    int32_t width, height;
    int32_t step, step_log2;
    float lum2;               // sigma_lum sigma_lum
    float inv_normal;         // 1 / (sigma_normal sigma_normal)
    float sigma_position;
    float firefly_ratio;
    uint32_t use_clamp, use_normal, use_position;
    uint32_t demodulate;      // prepare: divide by the albedo going in
    uint32_t final_image;     // prepare with passes = 0: dst is the denoised image, {c1 d or c1, I.a}
};

constexpr float kGuidedVarFloor = 9.5367431640625e-07f;        // 2^-20

__device__ __forceinline__ float guided_lum(float r, float g, float b) { return (0.25f * r + 0.5f * g) + 0.25f * b; }

// Tile of 64 columns x 4 rows per block of four waves (wave k: row k, lane: column).  The moments of a pixel take the clamped luminance,
// normal and position of the 7 x 7 pixels about it, and a clamped pixel the luminance, normal and position of the 3 x 3 about it: the block
// stages the 72 x 12 pixels about its tile once (c0, its luminance, normal and position: ten arrays), clamps the 70 x 10 in the middle (c1
// over c0 in place, its luminance into an array of its own) and then every lane walks its 49 taps in LDS, lane l reading word l + const
// of a row: conflict free.  A pixel outside the image is never staged and a tap on it is skipped by its coordinates.  37.4 KB per block.
// It also writes, per pixel, which of its 8 neighbours have a geometric weight > 0 (bit 3 (j + 1) + (i + 1)): the passes blur the
// variance over those only, and the geometry does not change from pass to pass.
constexpr int kPrepW0 = 72, kPrepH0 = 12, kPrepW1 = 70, kPrepH1 = 10;
constexpr int kPrepN0 = kPrepW0 * kPrepH0, kPrepN1 = kPrepW1 * kPrepH1;
constexpr size_t kPrepLdsBytes = (size_t)(10 * kPrepN0 + kPrepN1) * sizeof(float);

// (guided_prepare_tvar_kernel below repeats this body with the temporal select added: a change here belongs there too; with every
// history shorter than 4 the two give the same bits, which tests/test_gpu_temporal_moments.py runs)
__global__ void __launch_bounds__(256) guided_prepare_kernel(GuidedArgs a)
{
    extern __shared__ float seg[];                                   // 10 x [12][72], origin (x0 - 4, y0 - 4); then [10][70], origin (x0 - 3, y0 - 3)
    float *c0r = seg, *c0g = seg + kPrepN0, *c0b = seg + 2 * kPrepN0, *l0 = seg + 3 * kPrepN0, *gn = seg + 4 * kPrepN0, *gp = seg + 7 * kPrepN0;
    float *l1 = seg + 10 * kPrepN0;
    const int tid = (int)threadIdx.x, lane = tid & 63, k = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x0 = (int)blockIdx.x * 64, y0 = (int)blockIdx.y * 4;
    // the geometric weight between the staged pixel at word e (its normal n, position pos and 1 / (sigma_position t)^2) and the one o words on
    auto geometric = [&](int e, int o, const f3 &n, const f3 &pos, float inv_pos) {
        float g = 1.0f;
        if (a.use_normal) g = g * atrous_ew(atrous_dot3(gn[e + o] - n.x, gn[kPrepN0 + e + o] - n.y, gn[2 * kPrepN0 + e + o] - n.z) * a.inv_normal);
        if (a.use_position) g = g * atrous_ew(atrous_dot3(gp[e + o] - pos.x, gp[kPrepN0 + e + o] - pos.y, gp[2 * kPrepN0 + e + o] - pos.z) * inv_pos);
        return g;
    };
    for (int e = tid; e < kPrepN0; e += 256) {
        const int cy = e / kPrepW0, cx = e - cy * kPrepW0, qx = x0 - 4 + cx, qy = y0 - 4 + cy;
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
            const float4 v = a.image[q];
            f3 c = mk(v.x, v.y, v.z);
            if (a.demodulate) { const f3 d = atrous_divisor(a.albedo[q]); c = mk(c.x / d.x, c.y / d.y, c.z / d.z); }
            c0r[e] = c.x; c0g[e] = c.y; c0b[e] = c.z; l0[e] = guided_lum(c.x, c.y, c.z);
            if (a.use_normal) { const float4 u = a.normal[q]; gn[e] = u.x; gn[kPrepN0 + e] = u.y; gn[2 * kPrepN0 + e] = u.z; }
            if (a.use_position) { const float4 u = a.position[q]; gp[e] = u.x; gp[kPrepN0 + e] = u.y; gp[2 * kPrepN0 + e] = u.z; }
        }
    }
    __syncthreads();
    for (int e = tid; e < kPrepN1; e += 256) {
        const int cy = e / kPrepW1, cx = e - cy * kPrepW1, qx = x0 - 3 + cx, qy = y0 - 3 + cy;
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const int e0 = (cy + 1) * kPrepW0 + (cx + 1);
            float l = l0[e0];
            if (a.use_clamp) {
                f3 n = mk(0.0f, 0.0f, 0.0f), pos = mk(0.0f, 0.0f, 0.0f);
                float inv_pos = 0.0f;
                if (a.use_normal) n = mk(gn[e0], gn[kPrepN0 + e0], gn[2 * kPrepN0 + e0]);
                if (a.use_position) {
                    pos = mk(gp[e0], gp[kPrepN0 + e0], gp[2 * kPrepN0 + e0]);
                    const float sp = a.sigma_position * a.position[(size_t)qy * (size_t)a.width + (size_t)qx].w;
                    inv_pos = (sp > 0.0f) ? 1.0f / (sp * sp) : 0.0f;
                }
                float m = 0.0f;
                bool have = false;
#pragma unroll
                for (int j = -1; j <= 1; ++j)
#pragma unroll
                    for (int i = -1; i <= 1; ++i) {
                        if (i == 0 && j == 0) continue;
                        const int nx = qx + i, ny = qy + j, o = j * kPrepW0 + i;
                        if (nx < 0 || nx >= a.width || ny < 0 || ny >= a.height) continue;
                        if (!(geometric(e0, o, n, pos, inv_pos) > 0.0f)) continue;
                        const float lq = l0[e0 + o];
                        m = have ? (lq > m ? lq : m) : lq;
                        have = true;
                    }
                const float kk = a.firefly_ratio * m;
                if (have && l > kk) {
                    const float s = kk / l;
                    const f3 c = mk(c0r[e0] * s, c0g[e0] * s, c0b[e0] * s);
                    l = guided_lum(c.x, c.y, c.z);
                    c0r[e0] = c.x; c0g[e0] = c.y; c0b[e0] = c.z;       // (no other thread reads the colour of this pixel before the barrier)
                }
            }
            l1[e] = l;
        }
    }
    __syncthreads();
    const int x = x0 + lane, y = y0 + k;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const int ec = (k + 4) * kPrepW0 + lane + 4;
    const float *b = l1 + (k + 3) * kPrepW1 + lane + 3;
    f3 n = mk(0.0f, 0.0f, 0.0f), pos = mk(0.0f, 0.0f, 0.0f);
    float inv_pos = 0.0f;
    if (a.use_normal) n = mk(gn[ec], gn[kPrepN0 + ec], gn[2 * kPrepN0 + ec]);
    if (a.use_position) {
        pos = mk(gp[ec], gp[kPrepN0 + ec], gp[2 * kPrepN0 + ec]);
        const float sp = a.sigma_position * a.position[p].w;
        inv_pos = (sp > 0.0f) ? 1.0f / (sp * sp) : 0.0f;
    }
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    uint32_t near = 1u << 4;                                          // (the pixel itself always counts)
#pragma unroll
    for (int j = -3; j <= 3; ++j) {
        const int qy = y + j;
        if (qy < 0 || qy >= a.height) continue;
#pragma unroll
        for (int i = -3; i <= 3; ++i) {
            const int qx = x + i;
            // (a column outside the image was never staged: g and lq are then whatever LDS held, and `in` discards them.  No branch: the
            // lanes at the image's edge run in lockstep with the rest of their wave, so skipping their taps would save nothing)
            const float g = geometric(ec, j * kPrepW0 + i, n, pos, inv_pos);
            const float lq = b[j * kPrepW1 + i];
            const bool in = qx >= 0 && qx < a.width && g > 0.0f;
            if (in && j >= -1 && j <= 1 && i >= -1 && i <= 1) near |= 1u << (3 * (j + 1) + (i + 1));
            if (in && lq - lq == 0.0f) {
                s0 = s0 + g;
                s1 = s1 + g * lq;
                s2 = s2 + g * (lq * lq);
            }
        }
    }
    float mu = 0.0f, v0 = 0.0f;
    if (s0 > 0.0f) {
        mu = s1 / s0;
        const float v = s2 / s0 - mu * mu;
        v0 = (v > 0.0f) ? v : 0.0f;
    }
    f3 c = mk(c0r[ec], c0g[ec], c0b[ec]);
    store_through(a.variance + p, mu, v0, v0, s0);                    // (read by the last pass / the caller: rt_wavefront.hpp, store_through)
    store_through(a.near + p, near);                                  // (read by the passes)
    if (a.final_image) {
        if (a.demodulate) { const f3 d = atrous_divisor(a.albedo[p]); c = mk(c.x * d.x, c.y * d.y, c.z * d.z); }
        store_through(a.dst + p, c.x, c.y, c.z, a.image[p].w);
    } else {
        store_through(a.dst + p, c.x, c.y, c.z, v0);
    }
}

struct GuidedTvarArgs {
    GuidedArgs g;
    const float4 *moments;    // records {m1, m2, v, n} of the latest rtgl_temporal_accumulate (rt_temporal.hpp)
};

// guided_prepare_kernel with option "denoise_variance" = 1: the same tile, staging, clamp and 7 x 7 window (mu, s0 and the spatial v0 are
// still wanted); then v0 becomes the variance of the history mean, M.z / M.w of the pixel's moments record, where the history is at least
// 4 long and the record's moments are finite.  One more 16-byte load per pixel and a select.  A kernel of its own beside
// guided_prepare_kernel, not a shared body, so that the code generated for the option-off kernel stays exactly what it was.
__global__ void __launch_bounds__(256) guided_prepare_tvar_kernel(GuidedTvarArgs ta)
{
    const GuidedArgs &a = ta.g;
    extern __shared__ float seg[];                                   // 10 x [12][72], origin (x0 - 4, y0 - 4); then [10][70], origin (x0 - 3, y0 - 3)
    float *c0r = seg, *c0g = seg + kPrepN0, *c0b = seg + 2 * kPrepN0, *l0 = seg + 3 * kPrepN0, *gn = seg + 4 * kPrepN0, *gp = seg + 7 * kPrepN0;
    float *l1 = seg + 10 * kPrepN0;
    const int tid = (int)threadIdx.x, lane = tid & 63, k = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x0 = (int)blockIdx.x * 64, y0 = (int)blockIdx.y * 4;
    // the geometric weight between the staged pixel at word e (its normal n, position pos and 1 / (sigma_position t)^2) and the one o words on
    auto geometric = [&](int e, int o, const f3 &n, const f3 &pos, float inv_pos) {
        float g = 1.0f;
        if (a.use_normal) g = g * atrous_ew(atrous_dot3(gn[e + o] - n.x, gn[kPrepN0 + e + o] - n.y, gn[2 * kPrepN0 + e + o] - n.z) * a.inv_normal);
        if (a.use_position) g = g * atrous_ew(atrous_dot3(gp[e + o] - pos.x, gp[kPrepN0 + e + o] - pos.y, gp[2 * kPrepN0 + e + o] - pos.z) * inv_pos);
        return g;
    };
    for (int e = tid; e < kPrepN0; e += 256) {
        const int cy = e / kPrepW0, cx = e - cy * kPrepW0, qx = x0 - 4 + cx, qy = y0 - 4 + cy;
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
            const float4 v = a.image[q];
            f3 c = mk(v.x, v.y, v.z);
            if (a.demodulate) { const f3 d = atrous_divisor(a.albedo[q]); c = mk(c.x / d.x, c.y / d.y, c.z / d.z); }
            c0r[e] = c.x; c0g[e] = c.y; c0b[e] = c.z; l0[e] = guided_lum(c.x, c.y, c.z);
            if (a.use_normal) { const float4 u = a.normal[q]; gn[e] = u.x; gn[kPrepN0 + e] = u.y; gn[2 * kPrepN0 + e] = u.z; }
            if (a.use_position) { const float4 u = a.position[q]; gp[e] = u.x; gp[kPrepN0 + e] = u.y; gp[2 * kPrepN0 + e] = u.z; }
        }
    }
    __syncthreads();
    for (int e = tid; e < kPrepN1; e += 256) {
        const int cy = e / kPrepW1, cx = e - cy * kPrepW1, qx = x0 - 3 + cx, qy = y0 - 3 + cy;
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const int e0 = (cy + 1) * kPrepW0 + (cx + 1);
            float l = l0[e0];
            if (a.use_clamp) {
                f3 n = mk(0.0f, 0.0f, 0.0f), pos = mk(0.0f, 0.0f, 0.0f);
                float inv_pos = 0.0f;
                if (a.use_normal) n = mk(gn[e0], gn[kPrepN0 + e0], gn[2 * kPrepN0 + e0]);
                if (a.use_position) {
                    pos = mk(gp[e0], gp[kPrepN0 + e0], gp[2 * kPrepN0 + e0]);
                    const float sp = a.sigma_position * a.position[(size_t)qy * (size_t)a.width + (size_t)qx].w;
                    inv_pos = (sp > 0.0f) ? 1.0f / (sp * sp) : 0.0f;
                }
                float m = 0.0f;
                bool have = false;
#pragma unroll
                for (int j = -1; j <= 1; ++j)
#pragma unroll
                    for (int i = -1; i <= 1; ++i) {
                        if (i == 0 && j == 0) continue;
                        const int nx = qx + i, ny = qy + j, o = j * kPrepW0 + i;
                        if (nx < 0 || nx >= a.width || ny < 0 || ny >= a.height) continue;
                        if (!(geometric(e0, o, n, pos, inv_pos) > 0.0f)) continue;
                        const float lq = l0[e0 + o];
                        m = have ? (lq > m ? lq : m) : lq;
                        have = true;
                    }
                const float kk = a.firefly_ratio * m;
                if (have && l > kk) {
                    const float s = kk / l;
                    const f3 c = mk(c0r[e0] * s, c0g[e0] * s, c0b[e0] * s);
                    l = guided_lum(c.x, c.y, c.z);
                    c0r[e0] = c.x; c0g[e0] = c.y; c0b[e0] = c.z;       // (no other thread reads the colour of this pixel before the barrier)
                }
            }
            l1[e] = l;
        }
    }
    __syncthreads();
    const int x = x0 + lane, y = y0 + k;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const int ec = (k + 4) * kPrepW0 + lane + 4;
    const float *b = l1 + (k + 3) * kPrepW1 + lane + 3;
    f3 n = mk(0.0f, 0.0f, 0.0f), pos = mk(0.0f, 0.0f, 0.0f);
    float inv_pos = 0.0f;
    if (a.use_normal) n = mk(gn[ec], gn[kPrepN0 + ec], gn[2 * kPrepN0 + ec]);
    if (a.use_position) {
        pos = mk(gp[ec], gp[kPrepN0 + ec], gp[2 * kPrepN0 + ec]);
        const float sp = a.sigma_position * a.position[p].w;
        inv_pos = (sp > 0.0f) ? 1.0f / (sp * sp) : 0.0f;
    }
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    uint32_t near = 1u << 4;                                          // (the pixel itself always counts)
#pragma unroll
    for (int j = -3; j <= 3; ++j) {
        const int qy = y + j;
        if (qy < 0 || qy >= a.height) continue;
#pragma unroll
        for (int i = -3; i <= 3; ++i) {
            const int qx = x + i;
            // (a column outside the image was never staged: g and lq are then whatever LDS held, and `in` discards them.  No branch: the
            // lanes at the image's edge run in lockstep with the rest of their wave, so skipping their taps would save nothing)
            const float g = geometric(ec, j * kPrepW0 + i, n, pos, inv_pos);
            const float lq = b[j * kPrepW1 + i];
            const bool in = qx >= 0 && qx < a.width && g > 0.0f;
            if (in && j >= -1 && j <= 1 && i >= -1 && i <= 1) near |= 1u << (3 * (j + 1) + (i + 1));
            if (in && lq - lq == 0.0f) {
                s0 = s0 + g;
                s1 = s1 + g * lq;
                s2 = s2 + g * (lq * lq);
            }
        }
    }
    float mu = 0.0f, v0 = 0.0f;
    if (s0 > 0.0f) {
        mu = s1 / s0;
        const float v = s2 / s0 - mu * mu;
        v0 = (v > 0.0f) ? v : 0.0f;
    }
    const float4 M = ta.moments[p];
    const bool t = M.w >= 4.0f && M.x - M.x == 0.0f && M.y - M.y == 0.0f;
    v0 = t ? M.z / M.w : v0;
    f3 c = mk(c0r[ec], c0g[ec], c0b[ec]);
    store_through(a.variance + p, mu, v0, v0, s0);                    // (read by the last pass / the caller: rt_wavefront.hpp, store_through)
    store_through(a.near + p, near);                                  // (read by the passes)
    if (a.final_image) {
        if (a.demodulate) { const f3 d = atrous_divisor(a.albedo[p]); c = mk(c.x * d.x, c.y * d.y, c.z * d.z); }
        store_through(a.dst + p, c.x, c.y, c.z, a.image[p].w);
    } else {
        store_through(a.dst + p, c.x, c.y, c.z, v0);
    }
}

// One guided pass: atrous_kernel's staged form (above) over records {c.rgb, var}, with a tenth staged array for the variance.  The
// luminance tolerance of a pixel comes from the 3 x 3 blur of the variance about it, at unit spacing whatever the step, over the
// neighbours the prepare kernel marked: those words are not among the staged rows (which lie `step` apart) and are read from global
// memory, three runs of up to 66 adjacent records per wave.
// kLast: the result goes to the denoised image with the accumulation image's alpha (kRemod: times the pixel's albedo) and the variance to
// the third component of the variance buffer; otherwise both go into the next pass's record.
template <bool kLast, bool kRemod, bool kWide>
__global__ void __launch_bounds__(256) guided_kernel(GuidedArgs a)
{
    extern __shared__ float seg[];                                   // [2][10][wt]
    constexpr int kRecs = kWide ? 3 : 1;
    const int s = a.step, wt = 64 + 4 * s;
    const int tid = (int)threadIdx.x, lane = tid & 63, k = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x0 = (int)blockIdx.x * 64;
    const int chunk = (int)blockIdx.y >> a.step_log2, Y0 = 4 * s * chunk + ((int)blockIdx.y & (s - 1));
    if (Y0 >= a.height) return;                                      // (block-uniform, in front of every barrier)
    const int x = x0 + lane, y = Y0 + k * s;
    const bool live = x < a.width && y < a.height;
    f3 c = mk(0.0f, 0.0f, 0.0f), n = mk(0.0f, 0.0f, 0.0f), pos = mk(0.0f, 0.0f, 0.0f);
    float var = 0.0f, lum = 0.0f, inv_pos = 0.0f, inv_lum = 0.0f;
    const size_t p = live ? (size_t)y * (size_t)a.width + (size_t)x : 0;
    if (live) {
        const float4 v4 = a.src[p];
        c = mk(v4.x, v4.y, v4.z);
        var = v4.w;
        lum = guided_lum(c.x, c.y, c.z);
        const uint32_t near = a.near[p];
        float vs = 0.0f, vw = 0.0f;
#pragma unroll
        for (int j = -1; j <= 1; ++j)
#pragma unroll
            for (int i = -1; i <= 1; ++i) {
                const int qx = x + i, qy = y + j;
                if (!(near >> (3 * (j + 1) + (i + 1)) & 1u)) continue;       // (a neighbour outside the image is never marked)
                const float bw = (j == 0 ? 0.5f : 0.25f) * (i == 0 ? 0.5f : 0.25f);
                vs = vs + bw * a.src[(size_t)qy * (size_t)a.width + (size_t)qx].w;
                vw = vw + bw;
            }
        inv_lum = 1.0f / (a.lum2 * (vs / vw) + kGuidedVarFloor);
        if (a.use_normal) { const float4 v = a.normal[p]; n = mk(v.x, v.y, v.z); }
        if (a.use_position) {
            const float4 v = a.position[p];
            pos = mk(v.x, v.y, v.z);
            const float sp = a.sigma_position * v.w;
            inv_pos = (sp > 0.0f) ? 1.0f / (sp * sp) : 0.0f;
        }
    }
    float4 rc[kRecs], rn[kRecs], rp[kRecs];
    auto load_row = [&](int m) {
        const int ty = Y0 + (m - 2) * s;
        if (ty < 0 || ty >= a.height) return;
#pragma unroll
        for (int u = 0; u < kRecs; ++u) {
            const int col = tid + 256 * u, qx = x0 - 2 * s + col;
            if (col < wt && qx >= 0 && qx < a.width) {
                const size_t q = (size_t)ty * (size_t)a.width + (size_t)qx;
                rc[u] = a.src[q];
                if (a.use_normal) rn[u] = a.normal[q];
                if (a.use_position) rp[u] = a.position[q];
            }
        }
    };
    auto store_row = [&](int m) {
        const int ty = Y0 + (m - 2) * s;
        if (ty < 0 || ty >= a.height) return;
        float *b = seg + (m & 1) * 10 * wt;
#pragma unroll
        for (int u = 0; u < kRecs; ++u) {
            const int col = tid + 256 * u, qx = x0 - 2 * s + col;
            if (col < wt && qx >= 0 && qx < a.width) {
                b[col] = rc[u].x; b[wt + col] = rc[u].y; b[2 * wt + col] = rc[u].z; b[9 * wt + col] = rc[u].w;
                if (a.use_normal) { b[3 * wt + col] = rn[u].x; b[4 * wt + col] = rn[u].y; b[5 * wt + col] = rn[u].z; }
                if (a.use_position) { b[6 * wt + col] = rp[u].x; b[7 * wt + col] = rp[u].y; b[8 * wt + col] = rp[u].z; }
            }
        }
    };
    f3 acc = mk(0.0f, 0.0f, 0.0f);
    float ws = 0.0f, va = 0.0f;
    load_row(0);
    store_row(0);
    __syncthreads();
#pragma unroll 1
    for (int m = 0; m < 8; ++m) {
        if (m < 7) load_row(m + 1);
        const int j = m - 2 - k, ty = Y0 + (m - 2) * s;
        if (live && j >= -2 && j <= 2 && ty >= 0 && ty < a.height) {
            const float hj = (j == 0) ? 0.375f : ((j == -1 || j == 1) ? 0.25f : 0.0625f);
            const float *b = seg + (m & 1) * 10 * wt + lane + 2 * s;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int o = (i - 2) * s, qx = x + o;
                const float hi = (i == 2) ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f);
                const f3 t = mk(b[o], b[wt + o], b[2 * wt + o]);
                const float dl = guided_lum(t.x, t.y, t.z) - lum;                // (qx outside the image: unstaged words, discarded below, as in atrous_kernel)
                float w = hj * hi;
                w = w * atrous_ew((dl * dl) * inv_lum);
                if (a.use_normal) w = w * atrous_ew(atrous_dot3(b[3 * wt + o] - n.x, b[4 * wt + o] - n.y, b[5 * wt + o] - n.z) * a.inv_normal);
                if (a.use_position) w = w * atrous_ew(atrous_dot3(b[6 * wt + o] - pos.x, b[7 * wt + o] - pos.y, b[8 * wt + o] - pos.z) * inv_pos);
                if (qx >= 0 && qx < a.width && w > 0.0f) {
                    acc = mk(acc.x + w * t.x, acc.y + w * t.y, acc.z + w * t.z);
                    ws = ws + w;
                    va = va + (w * w) * b[9 * wt + o];
                }
            }
        }
        if (m < 7) store_row(m + 1);
        __syncthreads();
    }
    if (!live) return;
    f3 out = c;
    float vout = var;
    if (ws > 0.0f) { out = mk(acc.x / ws, acc.y / ws, acc.z / ws); vout = va / (ws * ws); }
    if (kLast) {
        if (kRemod) { const f3 d = atrous_divisor(a.albedo[p]); out = mk(out.x * d.x, out.y * d.y, out.z * d.z); }
        const float4 vb = a.variance[p];
        store_through(a.dst + p, out.x, out.y, out.z, a.image[p].w);   // (read by the caller: rt_wavefront.hpp, store_through)
        store_through(a.variance + p, vb.x, vb.y, vout, vb.w);
    } else {
        store_through(a.dst + p, out.x, out.y, out.z, vout);           // (read by the next pass)
    }
}

}  // namespace rt
