// rt_bucket_guide.hpp -- rtgl_robust_denoise: the resolve of a robust session and the records the guided filter takes, in one kernel.  The
// luminance tolerance of a pixel comes from the spread of its own K bucket means (Yuen's variance of the trimmed mean the resolve makes)
// where rtgl_denoise_guided estimates it from a 7 x 7 window of the picture.  The contract is in include/rtgl_amd.h ("robust denoise"),
// the reasoning and the figures in DESIGN.md 5.15, the host half (validation, states, sizes) in rt_bucket_guide_plan.hpp.  The passes
// behind this kernel are guided_kernel's (rt_denoise.hpp), launched as rtgl_denoise_guided launches them.  No reference counterpart.
//
// Tile of 64 columns x 4 rows per block of four waves (wave k: row k, lane: column), guided_prepare_kernel's mapping.  Only the guides
// have a neighbourhood: normal.xyz and position.xyz of the 66 x 6 pixels about the tile are staged in LDS, six arrays of 396 words, 9504
// bytes, lane l reading word l + const of a row: conflict free.  The colour has none: every lane loads its K bucket records first and
// keeps keys, ranks, G, t, the weighted mean and the winsorized variance in registers.  Every loop over the buckets has constant bounds
// and is unrolled, the order statistics are picked by compares: no array is indexed at run time.  The arithmetic of steps 1-9 of the
// resolve is restated from robust_resolve_kernel and spread_tiles_kernel, not shared, so that their code stays what it was.  Per pixel
// 16 K bytes of buckets and up to 48 of planes are read (plus the halo), 52 are written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.hpp"
#include "rt_wavefront.hpp"
#include "rt_error.hpp"
#include "rt_denoise.hpp"

#pragma clang fp contract(off)

namespace rt {

struct BucketGuideArgs {
    const float4 *buckets;    // K planes of `plane` pixels, bucket-major
    const float4 *albedo;     // first-hit planes; a plane the parameters do not need may be NULL and is never read
    const float4 *normal;
    const float4 *position;
    float4 *dst;              // records {c0.rgb, v0} for the first pass; with passes = 0 the denoised image
    float4 *resolved;         // passes > 0: the denoised buffer, which takes {out.rgb, out.w}: the last pass reads its own pixel's alpha there
    float4 *variance;         // {lum(c0), v0, v0, (float)h}; the last pass writes its third component again
    uint32_t *near;           // per pixel, the neighbours (of its 3 x 3) whose geometric weight is > 0: read by the passes
    size_t plane;
    int32_t width, height;
    uint32_t frames;          // N >= K
    float gain;
    float inv_normal;         // 1 / (sigma_normal sigma_normal)
    float sigma_position;
    uint32_t use_normal, use_position;
    uint32_t final_image;     // passes = 0
};

constexpr int kBgW = 66, kBgH = 6, kBgN = kBgW * kBgH;

__device__ __forceinline__ bool bucket_guide_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

template <int K, bool kDemod>
__global__ void __launch_bounds__(256) bucket_guide_kernel(BucketGuideArgs a)
{
    __shared__ float seg[6 * kBgN];                                  // normal.xyz, position.xyz: [6][66] each, origin (x0 - 1, y0 - 1)
    float *gn = seg, *gp = seg + 3 * kBgN;
    const int tid = (int)threadIdx.x, lane = tid & 63, k = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x0 = (int)blockIdx.x * 64, y0 = (int)blockIdx.y * 4;
    const int x = x0 + lane, y = y0 + k;
    const bool live = x < a.width && y < a.height;
    const size_t p = live ? (size_t)y * (size_t)a.width + (size_t)x : 0;
    float4 b[K];
    float4 alb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float pw = 0.0f;
    if (live) {
#pragma unroll
        for (int j = 0; j < K; ++j) b[j] = a.buckets[(size_t)j * a.plane + p];
        if (kDemod) alb = a.albedo[p];
        if (a.use_position) pw = a.position[p].w;
    }
    for (int e = tid; e < kBgN; e += 256) {
        const int cy = e / kBgW, cx = e - cy * kBgW, qx = x0 - 1 + cx, qy = y0 - 1 + cy;
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
            if (a.use_normal) { const float4 u = a.normal[q]; gn[e] = u.x; gn[kBgN + e] = u.y; gn[2 * kBgN + e] = u.z; }
            if (a.use_position) { const float4 u = a.position[q]; gp[e] = u.x; gp[kBgN + e] = u.y; gp[2 * kBgN + e] = u.z; }
        }
    }
    __syncthreads();
    if (!live) return;

    // steps 1-7 of the resolve
    float key[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float l = error_lum(b[j].x, b[j].y, b[j].z);
        key[j] = bucket_guide_finite(l) ? l : __uint_as_float(0x7F800000u);
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
    if (!bucket_guide_finite(S)) G = 1.0f;
    else if (!(S > 0.0f)) G = 0.0f;
    else G = A / ((float)K * S);
    if (!(G <= 1.0f)) G = 1.0f;
    if (!(G >= 0.0f)) G = 0.0f;
    const float u = (G * a.gain) * (float)(K / 2);
    constexpr int cap = (K - 1) / 2;
    const int t = (u >= (float)cap) ? cap : (int)u;                    // (N >= K: the host refuses the call otherwise, and every n_j > 0)
    // steps 8-9: the weighted mean of the kept buckets
    const uint32_t nq = a.frames / (uint32_t)K, rem = a.frames % (uint32_t)K;
    float W = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f, cw = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (t <= rank[j] && rank[j] <= K - 1 - t) {
            const float fn = (float)(nq + ((uint32_t)j < rem ? 1u : 0u));
            W = W + fn;
            cx = cx + fn * b[j].x; cy = cy + fn * b[j].y; cz = cz + fn * b[j].z; cw = cw + fn * b[j].w;
        }
    }
    const float ox = cx / W, oy = cy / W, oz = cz / W, ow = cw / W;
    // the divisor, c0 and the luminances x_j the variance is of
    f3 d = mk(1.0f, 1.0f, 1.0f), c0 = mk(ox, oy, oz);
    if (kDemod) { d = atrous_divisor(alb); c0 = mk(ox / d.x, oy / d.y, oz / d.z); }
    float xs[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (kDemod) {
            const float l = guided_lum(b[j].x / d.x, b[j].y / d.y, b[j].z / d.z);
            xs[j] = bucket_guide_finite(l) ? l : __uint_as_float(0x7F800000u);
        } else xs[j] = key[j];
    }
    // winsorized by the resolve's ranks, then Yuen's variance
    float lo = 0.0f, hi = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        lo = (rank[j] == t) ? xs[j] : lo;
        hi = (rank[j] == K - 1 - t) ? xs[j] : hi;
    }
    float M = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        xs[j] = (rank[j] < t) ? lo : ((rank[j] > K - 1 - t) ? hi : xs[j]);
        M = M + xs[j];
    }
    const float mw = M / (float)K;
    float D = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float dd = xs[j] - mw;
        D = D + dd * dd;
    }
    const int h = K - 2 * t;
    const float v = D / (float)(h * (h - 1));
    const float v0 = (v - v == 0.0f) ? v : 0.0f;

    // the near mask of rtgl_denoise_guided
    const int ec = (k + 1) * kBgW + lane + 1;
    f3 n = mk(0.0f, 0.0f, 0.0f), pos = mk(0.0f, 0.0f, 0.0f);
    float inv_pos = 0.0f;
    if (a.use_normal) n = mk(gn[ec], gn[kBgN + ec], gn[2 * kBgN + ec]);
    if (a.use_position) {
        pos = mk(gp[ec], gp[kBgN + ec], gp[2 * kBgN + ec]);
        const float sp = a.sigma_position * pw;
        inv_pos = (sp > 0.0f) ? 1.0f / (sp * sp) : 0.0f;
    }
    uint32_t near = 1u << 4;                                          // (the pixel itself always counts)
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
        const int qy = y + j;
        if (qy < 0 || qy >= a.height) continue;
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            if (i == 0 && j == 0) continue;
            const int qx = x + i, o = ec + j * kBgW + i;
            // (a column outside the image was never staged: g is then whatever LDS held, and the coordinates discard it)
            float g = 1.0f;
            if (a.use_normal) g = g * atrous_ew(atrous_dot3(gn[o] - n.x, gn[kBgN + o] - n.y, gn[2 * kBgN + o] - n.z) * a.inv_normal);
            if (a.use_position) g = g * atrous_ew(atrous_dot3(gp[o] - pos.x, gp[kBgN + o] - pos.y, gp[2 * kBgN + o] - pos.z) * inv_pos);
            if (qx >= 0 && qx < a.width && g > 0.0f) near |= 1u << (3 * (j + 1) + (i + 1));
        }
    }
    store_through(a.variance + p, guided_lum(c0.x, c0.y, c0.z), v0, v0, (float)h);      // (read by the last pass / the caller: rt_wavefront.hpp, store_through)
    store_through(a.near + p, near);                                  // (read by the passes)
    if (a.final_image) {
        if (kDemod) c0 = mk(c0.x * d.x, c0.y * d.y, c0.z * d.z);
        store_through(a.dst + p, c0.x, c0.y, c0.z, ow);               // (read by the caller)
    } else {
        store_through(a.dst + p, c0.x, c0.y, c0.z, v0);               // (read by the first pass)
        store_through(a.resolved + p, ox, oy, oz, ow);                // (the last pass takes the alpha of its own pixel from here before it writes that pixel)
    }
}

}  // namespace rt
