// rt_temporal.hpp -- rtgl_temporal_accumulate: the accumulated radiance of the previous view carried into the current one (the temporal
// half of SVGF, Schied et al. 2017; its spatial half is rt_denoise.hpp).  The contract is in include/rtgl_amd.h ("temporal accumulation"),
// the reasoning in DESIGN.md 5.6.  No reference counterpart: the reference answers a camera move with u_reset_flag.
// One kernel template, temporal_kernel; with option "temporal_moments" on, its instances also carry the luminance moments.
//
// Defined operation by operation like the denoisers (binary32, one rounding each, no contraction, correctly rounded divide; floor is
// exact), so that the numpy restatements (tests/temporal_mirror.py, tests/temporal_moments_mirror.py) give the same bits: nothing here
// may be reassociated or fused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rt_device.hpp"
#include "rt_wavefront.hpp"
#include "rt_denoise.hpp"

#pragma clang fp contract(off)

namespace rt {

// The camera record of one call, built on the host (rtgl_amd.hip, temporal_camera) from the frame parameters of that call.  The static
// shortcut applies when all 21 floats compare equal to the previous call's.
struct TemporalCamera {
    float pos[3], fwd[3], up[3], right[3];
    float hw, asp;            // tan(fov / 2) (in double, rounded once), height / width
    float wd, ht;             // 2 hw, 2 (hw asp)
    float ff, rr, uu;         // dot(forward, forward), dot(right, right), dot(up, up)
    float kx, ky;             // ff / (wd rr), ff / (ht uu)
};

struct TemporalArgs {
    const float4 *image;                  // this frame's radiance (the accumulation image as it stands)
    const float4 *normal, *position;      // this frame's first-hit planes; normal may be NULL (plane off): then it is neither read nor copied
    const float4 *hist_prev, *normal_prev, *position_prev;    // what the previous call wrote (kHistory instances only)
    float4 *hist_out, *normal_out, *position_out;             // the other buffer of each pair
    int32_t width, height;
    TemporalCamera cur, prev;
    float max_history;
    float inv_normal;         // 1 / (sigma_normal sigma_normal)
    float sigma_position;
};

// What option "temporal_moments" adds to a call (temporal_kernel, kMom = 1 or 2): the first and second moment of each frame's luminance carried
// through the same taps, weights and blend as the colour, records {m1, m2, v, n} in two buffers that take turns with the history's.
struct TemporalMomentsArgs {
    TemporalArgs t;
    const float4 *albedo;     // mode 2: the luminance is that of I.rgb / d; otherwise NULL and never read
    const float4 *mom_prev;   // what the previous call wrote (kHistory instances only)
    float4 *mom_out;
};

// The argument record of a mode: TemporalArgs with the option off, TemporalMomentsArgs with it on; temporal_base is its TemporalArgs.
template <int kMom> struct TemporalArgsOf { typedef TemporalMomentsArgs type; };
template <> struct TemporalArgsOf<0> { typedef TemporalArgs type; };
__host__ __device__ __forceinline__ const TemporalArgs &temporal_base(const TemporalArgs &x) { return x; }
__host__ __device__ __forceinline__ const TemporalArgs &temporal_base(const TemporalMomentsArgs &x) { return x.t; }

__device__ __forceinline__ float temporal_dot(const f3 &a, const float *b) { return (a.x * b[0] + a.y * b[1]) + a.z * b[2]; }

// One lane per pixel; a block of four waves takes 64 columns x 4 rows, so that the (up to) four taps of neighbouring lanes land on
// neighbouring records of two adjacent rows.  kHistory = false: the first call, or the first after a reset: the history becomes this frame.
// kStatic: the previous camera record equals the current one: the single tap q = p with b = 1.  kNormal / kPosition: the term is on.
// kMom: option "temporal_moments" (0, 1, 2).  1 and 2 carry the luminance moments along (TemporalMomentsArgs; 2 takes the luminance of
// I.rgb / d): the same geometry, taps, weights and blend, and the history written is the same bit for bit; per pixel 16 bytes more out,
// up to one tap's worth of 16 bytes more in and, in mode 2, the albedo record.  One __global__ template whose argument record follows
// from the mode, the moments' lines under `if constexpr`: the code generated for the kMom = 0 instances is what a kernel without those
// lines gives (which also says why a __device__ body shared by two kernels is not).
template <bool kHistory, bool kStatic, bool kNormal, bool kPosition, int kMom>
__global__ void __launch_bounds__(256) temporal_kernel(typename TemporalArgsOf<kMom>::type mo)
{
    const TemporalArgs &a = temporal_base(mo);
    const int x = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const float4 I = a.image[p], P4 = a.position[p];
    float4 N4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.normal) N4 = a.normal[p];
    f3 out = mk(I.x, I.y, I.z);
    float n = 1.0f;
    float m1 = 0.0f, m2 = 0.0f;
    if constexpr (kMom != 0) {
        f3 c = mk(I.x, I.y, I.z);                                       // this frame's luminance l and its square, the moments without history
        if constexpr (kMom == 2) { const f3 d = atrous_divisor(mo.albedo[p]); c = mk(c.x / d.x, c.y / d.y, c.z / d.z); }
        m1 = guided_lum(c.x, c.y, c.z);
        m2 = m1 * m1;
    }
    if (kHistory) {
        const bool hit = P4.w > 0.0f;
        const float Wf = (float)a.width, Hf = (float)a.height;
        f3 v;
        if (hit) {
            v = mk(P4.x - a.prev.pos[0], P4.y - a.prev.pos[1], P4.z - a.prev.pos[2]);
        } else {                                                        // the background is at infinity: the pixel's own direction
            const float xs = ((float)x / Wf) * 2.0f - 1.0f, ys = ((float)y / Hf) * 2.0f - 1.0f;
            v = mk((a.cur.fwd[0] + (a.cur.right[0] * a.cur.wd) * xs) + (a.cur.up[0] * a.cur.ht) * ys,
                   (a.cur.fwd[1] + (a.cur.right[1] * a.cur.wd) * xs) + (a.cur.up[1] * a.cur.ht) * ys,
                   (a.cur.fwd[2] + (a.cur.right[2] * a.cur.wd) * xs) + (a.cur.up[2] * a.cur.ht) * ys);
        }
        const float f = temporal_dot(v, a.prev.fwd);
        const float sx = ((((temporal_dot(v, a.prev.right) / f) * a.prev.kx) + 1.0f) * 0.5f) * Wf;
        const float sy = ((((temporal_dot(v, a.prev.up) / f) * a.prev.ky) + 1.0f) * 0.5f) * Hf;
        const bool have = f > 0.0f && sx >= -1.0f && sx < Wf && sy >= -1.0f && sy < Hf;       // (a NaN fails)
        if (have) {
            float inv_pos = 0.0f;
            if (kPosition) { const float sp = a.sigma_position * P4.w; inv_pos = (sp > 0.0f) ? 1.0f / (sp * sp) : 0.0f; }
            f3 acc = mk(0.0f, 0.0f, 0.0f);
            float na = 0.0f, ws = 0.0f, a1 = 0.0f, a2 = 0.0f;
            auto tap = [&](int qx, int qy, float b) {
                if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) return;
                const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
                const float4 Pq = a.position_prev[q];
                if ((Pq.w > 0.0f) != hit) return;
                float w = b;
                if (hit) {
                    if (kNormal) { const float4 Nq = a.normal_prev[q]; w = w * atrous_ew(atrous_dot3(Nq.x - N4.x, Nq.y - N4.y, Nq.z - N4.z) * a.inv_normal); }
                    if (kPosition) w = w * atrous_ew(atrous_dot3(Pq.x - P4.x, Pq.y - P4.y, Pq.z - P4.z) * inv_pos);
                }
                if (w > 0.0f) {
                    const float4 Hq = a.hist_prev[q];
                    acc = mk(acc.x + w * Hq.x, acc.y + w * Hq.y, acc.z + w * Hq.z);
                    na = na + w * Hq.w;
                    ws = ws + w;
                    if constexpr (kMom != 0) {
                        const float4 Mq = mo.mom_prev[q];
                        a1 = a1 + w * Mq.x;
                        a2 = a2 + w * Mq.y;
                    }
                }
            };
            if (kStatic) {
                tap(x, y, 1.0f);
            } else {
                const float x0 = __builtin_floorf(sx), y0 = __builtin_floorf(sy);
                const float fx = sx - x0, fy = sy - y0;
                const int xi = (int)x0, yi = (int)y0;                     // (-1 .. width - 1, -1 .. height - 1: `have`)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        tap(xi + i, yi + j, (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy));
            }
            if (ws > 0.0f) {
                const f3 h = mk(acc.x / ws, acc.y / ws, acc.z / ws);
                n = na / ws + 1.0f;
                n = (n > a.max_history) ? a.max_history : n;
                const float al = 1.0f / n;
                out = mk(h.x + (I.x - h.x) * al, h.y + (I.y - h.y) * al, h.z + (I.z - h.z) * al);
                if constexpr (kMom != 0) {
                    const float h1 = a1 / ws, h2 = a2 / ws;
                    m1 = h1 + (m1 - h1) * al;
                    m2 = h2 + (m2 - h2) * al;
                }
            }
        }
    }
    store_through(a.hist_out + p, out.x, out.y, out.z, n);              // (read by the next call / the caller: rt_wavefront.hpp, store_through)
    store_through(a.position_out + p, P4.x, P4.y, P4.z, P4.w);
    if (a.normal) store_through(a.normal_out + p, N4.x, N4.y, N4.z, N4.w);
    if constexpr (kMom != 0) {
        float v = m2 - m1 * m1;
        v = (v > 0.0f) ? v : 0.0f;                                      // (a NaN gives 0)
        store_through(mo.mom_out + p, m1, m2, v, n);                    // (read by the next call, rtgl_denoise_guided and the caller)
    }
}

}  // namespace rt