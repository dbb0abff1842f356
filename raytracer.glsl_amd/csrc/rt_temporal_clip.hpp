// rt_temporal_clip.hpp -- rtgl_temporal_clip: the latest history of rtgl_temporal_accumulate clamped, in place, into a per-pixel colour box
// taken from the 7 x 7 geometric neighbourhood of the current frame, and the history length of a clamped pixel cut (variance clipping,
// Salvi 2016; the history clamp of ReLAX).  The contract is in include/rtgl_amd.h ("temporal clip"), the reasoning in DESIGN.md 5.8.  No
// reference counterpart: the reference answers every change of lighting with u_reset_flag.
//
// Defined operation by operation like its neighbours (binary32, one rounding each, no contraction, correctly rounded divide and -- new
// here -- correctly rounded square root: __builtin_sqrtf under -fhip-fp32-correctly-rounded-divide-sqrt, csrc/Makefile), so that the
// numpy restatement (tests/temporal_clip_mirror.py) gives the same bits: nothing here may be reassociated or fused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.hpp"
#include "rt_wavefront.hpp"
#include "rt_denoise.hpp"

#pragma clang fp contract(off)

namespace rt {

struct TemporalClipArgs {
    const float4 *image;                  // this frame's own radiance
    const float4 *normal, *position;      // this frame's first-hit planes; normal is NULL and never read in the kNormal = false instances
    float4 *hist;                         // the latest history buffer {rgb, n}: read and written in place, every lane its own record only
    float4 *moments;                      // kMoments: the latest moments buffer {m1, m2, v, n}; its .w follows the history's
    int32_t width, height;
    float sigma_scale, clip_history;
    float inv_normal;                     // 1 / (sigma_normal sigma_normal)
    float sigma_position;
};

// The staged region of a block: its tile of 64 x 4 pixels and a halo of 3, origin (x0 - 3, y0 - 3).
constexpr int kClipW = 70, kClipH = 10, kClipN = kClipW * kClipH;
template <bool kNormal, bool kPosition> constexpr int clip_arrays() { return 3 + (kNormal ? 3 : 0) + (kPosition ? 3 : 0); }

// Tile of 64 columns x 4 rows per block of four waves (wave k: row k, lane: column), as guided_prepare_kernel.  The block stages the
// 70 x 10 pixels about its tile once -- I.rgb, N.xyz where the normal term is on, P.xyz where the position term is on, one array per
// component, and one byte per pixel for its kind (P.w > 0) -- and then every lane walks its 49 taps in LDS, lane l reading word l + const
// of a row: conflict free.  25.9 KB per block with both terms on.  A pixel outside the image is never staged: its LDS words are stale,
// and the tap on it is dropped by its coordinates.
template <bool kNormal, bool kPosition, bool kMoments>
__global__ void __launch_bounds__(256) temporal_clip_kernel(TemporalClipArgs a)
{
    constexpr int kArrays = clip_arrays<kNormal, kPosition>();
    __shared__ float seg[kArrays * kClipN];                           // [kArrays][10][70]
    __shared__ uint8_t kind[kClipN];
    float *cr = seg, *cg = seg + kClipN, *cb = seg + 2 * kClipN;
    float *gn = seg + 3 * kClipN, *gp = seg + (kNormal ? 6 : 3) * kClipN;
    const int tid = (int)threadIdx.x, lane = tid & 63, k = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x0 = (int)blockIdx.x * 64, y0 = (int)blockIdx.y * 4;
    for (int e = tid; e < kClipN; e += 256) {
        const int cy = e / kClipW, cx = e - cy * kClipW, qx = x0 - 3 + cx, qy = y0 - 3 + cy;
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
            const float4 v = a.image[q], u = a.position[q];
            cr[e] = v.x; cg[e] = v.y; cb[e] = v.z;
            kind[e] = u.w > 0.0f ? 1 : 0;
            if constexpr (kNormal) { const float4 t = a.normal[q]; gn[e] = t.x; gn[kClipN + e] = t.y; gn[2 * kClipN + e] = t.z; }
            if constexpr (kPosition) { gp[e] = u.x; gp[kClipN + e] = u.y; gp[2 * kClipN + e] = u.z; }
        }
    }
    __syncthreads();
    const int x = x0 + lane, y = y0 + k;
    if (x >= a.width || y >= a.height) return;                       // (behind the only barrier)
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const int ec = (k + 3) * kClipW + lane + 3;
    const float4 Hc = a.hist[p];
    const float tp = a.position[p].w;
    const bool hit = tp > 0.0f;
    const f3 own = mk(cr[ec], cg[ec], cb[ec]);
    f3 n = mk(0.0f, 0.0f, 0.0f), pos = mk(0.0f, 0.0f, 0.0f);
    float inv_pos = 0.0f;
    if constexpr (kNormal) n = mk(gn[ec], gn[kClipN + ec], gn[2 * kClipN + ec]);
    if constexpr (kPosition) {
        pos = mk(gp[ec], gp[kClipN + ec], gp[2 * kClipN + ec]);
        const float sp = a.sigma_position * tp;
        inv_pos = (sp > 0.0f) ? 1.0f / (sp * sp) : 0.0f;
    }
    float s0 = 0.0f;
    f3 s1 = mk(0.0f, 0.0f, 0.0f), s2 = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = -3; j <= 3; ++j) {
        const int qy = y + j;
        if (qy < 0 || qy >= a.height) continue;
#pragma unroll
        for (int i = -3; i <= 3; ++i) {
            const int qx = x + i, e = ec + j * kClipW + i;
            // (a column outside the image was never staged: what is read here is then whatever LDS held, and `in` discards it; no branch,
            // as in guided_prepare_kernel)
            float g = 1.0f;
            if constexpr (kNormal) g = g * atrous_ew(atrous_dot3(gn[e] - n.x, gn[kClipN + e] - n.y, gn[2 * kClipN + e] - n.z) * a.inv_normal);
            if constexpr (kPosition) g = g * atrous_ew(atrous_dot3(gp[e] - pos.x, gp[kClipN + e] - pos.y, gp[2 * kClipN + e] - pos.z) * inv_pos);
            const f3 c = mk(cr[e], cg[e], cb[e]);
            const bool in = qx >= 0 && qx < a.width && (kind[e] != 0) == hit && g > 0.0f;
            if (in && c.x - c.x == 0.0f && c.y - c.y == 0.0f && c.z - c.z == 0.0f) {
                s0 = s0 + g;
                s1 = mk(s1.x + g * c.x, s1.y + g * c.y, s1.z + g * c.z);
                s2 = mk(s2.x + g * (c.x * c.x), s2.y + g * (c.y * c.y), s2.z + g * (c.z * c.z));
            }
        }
    }
    f3 out = mk(Hc.x, Hc.y, Hc.z);
    float len = Hc.w;
    if (s0 > 0.0f) {
        bool clipped = false;
        auto channel = [&](float t1, float t2, float ic, float h) {
            const float mu = t1 / s0;
            float v = t2 / s0 - mu * mu;
            v = (v > 0.0f) ? v : 0.0f;                                // (a NaN gives 0)
            const float e = a.sigma_scale * __builtin_sqrtf(v);
            float lo = mu - e, hi = mu + e;
            lo = (ic < lo) ? ic : lo;                                 // the box always holds the pixel's own sample
            hi = (ic > hi) ? ic : hi;
            const bool below = h < lo;                                // (a NaN compares false: it clips nothing and changes nothing)
            float r = below ? lo : h;
            const bool above = r > hi;
            r = above ? hi : r;
            clipped = clipped || below || above;
            return r;
        };
        out = mk(channel(s1.x, s2.x, own.x, Hc.x), channel(s1.y, s2.y, own.y, Hc.y), channel(s1.z, s2.z, own.z, Hc.z));
        len = (clipped && len > a.clip_history) ? a.clip_history : len;
    }
    store_through(a.hist + p, out.x, out.y, out.z, len);              // (read by the denoisers, the next rtgl_temporal_accumulate and the caller)
    if constexpr (kMoments) {
        const float4 M = a.moments[p];
        store_through(a.moments + p, M.x, M.y, M.z, len);
    }
}

}  // namespace rt
