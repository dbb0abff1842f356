// The host half of rtgl_robust_denoise (include/rtgl_amd.h, "robust denoise"), as plain host C++: no HIP in this header, so that the host
// compiler can build it alone (tests/cpp/bucket_guide_plan_check.cpp).  The defaults and the validation of the parameter record, what
// state a session and the first-hit planes must be in, the planes a parameter set needs, the tile grid of the prepare kernel, its LDS
// and the sizes of the buffers the call writes.  tests/robust_denoise_mirror.py restates the validation and the states.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt_bucket_guide_plan {

constexpr uint32_t kDefaultPasses = 5u, kMaxPasses = 8u, kFlagDemodulate = 1u;      // (RTGL_DENOISE_DEMODULATE)
constexpr float kDefaultSigmaLum = 4.0f, kDefaultSigmaNormal = 0.3f, kDefaultSigmaPosition = 0.05f, kDefaultGain = 1.0f;
constexpr uint32_t kPlaneAlbedo = 1u, kPlaneNormal = 2u, kPlanePosition = 4u;      // (RTGL_AOV_*)
// the prepare kernel: a block per 64 x 4 pixels, the guides of the 66 x 6 pixels about them in LDS, six arrays (normal.xyz, position.xyz)
constexpr uint32_t kTileW = 64u, kTileH = 4u, kHaloW = kTileW + 2u, kHaloH = kTileH + 2u, kGuideArrays = 6u;
constexpr uint32_t kLdsBytes = kGuideArrays * kHaloW * kHaloH * 4u;

// rtgl_robust_denoise_params
struct Params { uint32_t passes; float sigma_lum, sigma_normal, sigma_position, gain; uint32_t flags, reserved[2]; };
static_assert(sizeof(Params) == 32, "the layout of include/rtgl_amd.h");
static_assert(kLdsBytes == 9504u, "about 9.5 KB");

inline Params default_params()
{
    Params p{};
    p.passes = kDefaultPasses; p.sigma_lum = kDefaultSigmaLum; p.sigma_normal = kDefaultSigmaNormal; p.sigma_position = kDefaultSigmaPosition;
    p.gain = kDefaultGain; p.flags = kFlagDemodulate;
    return p;
}

// what is wrong with a record (a message for rtgl_last_error), or NULL
inline const char *invalid(const Params &p)
{
    if (p.passes > kMaxPasses) return "passes must be 0..8";
    if (!std::isfinite(p.sigma_lum) || !std::isfinite(p.sigma_normal) || !std::isfinite(p.sigma_position))
        return "the sigmas must be finite (<= 0 switches the normal or the position term off)";
    if (!(p.sigma_lum > 0.0f)) return "sigma_lum must be > 0";
    if (!std::isfinite(p.gain) || !(p.gain >= 0.0f)) return "gain must be finite and >= 0";
    if (p.flags & ~kFlagDemodulate) return "unknown flag bits";
    for (uint32_t r : p.reserved) if (r) return "reserved fields must be 0";
    return nullptr;
}

inline bool demodulates(const Params &p) { return (p.flags & kFlagDemodulate) != 0u; }
// the first-hit planes a valid record reads (bits of option "aov")
inline uint32_t planes_needed(const Params &p)
{
    return (demodulates(p) ? kPlaneAlbedo : 0u) | (p.sigma_normal > 0.0f ? kPlaneNormal : 0u) | (p.sigma_position > 0.0f ? kPlanePosition : 0u);
}

// what is wrong with the session (RTGL_ERR_STATE), or NULL: every bucket must hold a sample
inline const char *refused(bool session, uint32_t N, uint32_t K)
{
    if (!session) return "no session (rtgl_robust_begin has not been called, or rtgl_robust_end has)";
    if (N < K) return "fewer frames than buckets: an empty bucket has no luminance";
    return nullptr;
}

// what is wrong with the first-hit planes (RTGL_ERR_STATE), or NULL: the conditions of rtgl_denoise_guided
inline const char *planes_refused(uint32_t needed, uint32_t enabled, bool restarted, uint32_t frames_in_planes)
{
    if (needed & ~enabled)
        return "a first-hit plane these parameters need is not enabled (option \"aov\": albedo to demodulate, normal for sigma_normal > 0, position for sigma_position > 0)";
    if (needed && (restarted || frames_in_planes == 0u)) return "no frame has been rendered since the first-hit planes last restarted";
    return nullptr;
}

// the grid of the prepare kernel, and the buffers of the call
inline uint32_t tiles_x(int width) { return width > 0 ? ((uint32_t)width + kTileW - 1u) / kTileW : 0u; }
inline uint32_t tiles_y(int rows) { return rows > 0 ? ((uint32_t)rows + kTileH - 1u) / kTileH : 0u; }
inline size_t pixels(int rows, int width) { return rows > 0 && width > 0 ? (size_t)rows * (size_t)width : 0u; }
inline size_t record_bytes(size_t px) { return px * 16u; }         // the denoised, the scratch and the variance buffers
inline size_t near_bytes(size_t px) { return px * 4u; }
inline uint32_t scratch_buffers(uint32_t passes) { return passes < 2u ? passes : 2u; }

}  // namespace rt_bucket_guide_plan
