// The host half of rtgl_denoise and rtgl_denoise_guided (include/rtgl_amd.h, "denoiser" and "variance-guided denoiser"), as plain host
// C++: no HIP in this header, so that the host compiler can build it alone (tests/cpp/denoise_plan_check.cpp).  The defaults and the
// validation of the two parameter records, the planes a record needs, what "denoise_variance" = 1 asks of the history, the geometry of a
// pass and of the prepare kernel, and the scratch buffers a call writes.  The refusals of the first-hit planes are
// rt_bucket_guide_plan::planes_refused.  tests/denoise_mirror.py and tests/denoise_guided_mirror.py restate the validation.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt_denoise_plan {

constexpr uint32_t kDefaultPasses = 5u, kMaxPasses = 8u, kFlagDemodulate = 1u;      // (RTGL_DENOISE_DEMODULATE)
constexpr float kDefaultSigmaColor = 16.0f, kDefaultSigmaLum = 4.0f, kDefaultSigmaNormal = 0.3f, kDefaultSigmaPosition = 0.05f, kDefaultFireflyRatio = 1.0f;
constexpr uint32_t kPlaneAlbedo = 1u, kPlaneNormal = 2u, kPlanePosition = 4u;      // (RTGL_AOV_*)
// a pass: a block per 64 columns x four rows `step` apart, two LDS buffers of nine (a-trous) or ten (guided) arrays of 64 + 4 step floats;
// above 256 floats a row takes the wide kernel
constexpr uint32_t kTileW = 64u, kTileRows = 4u, kAtrousArrays = 9u, kGuidedArrays = 10u, kWideAbove = 256u;
// the prepare kernel: a block per 64 x 4 pixels, ten arrays of the 72 x 12 pixels about them and one of the 70 x 10 in the middle
constexpr size_t kPrepLdsBytes = (size_t)(10 * 72 * 12 + 70 * 10) * 4u;

// rtgl_denoise_params, rtgl_denoise_guided_params
struct Params { uint32_t passes; float sigma_color, sigma_normal, sigma_position; uint32_t flags, reserved[3]; };
struct GuidedParams { uint32_t passes; float sigma_lum, sigma_normal, sigma_position, firefly_ratio; uint32_t flags, reserved[2]; };
static_assert(sizeof(Params) == 32 && sizeof(GuidedParams) == 32, "the layouts of include/rtgl_amd.h");

inline Params default_params()
{
    Params p{};
    p.passes = kDefaultPasses; p.sigma_color = kDefaultSigmaColor; p.sigma_normal = kDefaultSigmaNormal; p.sigma_position = kDefaultSigmaPosition;
    p.flags = kFlagDemodulate;
    return p;
}
inline GuidedParams default_guided_params()
{
    GuidedParams p{};
    p.passes = kDefaultPasses; p.sigma_lum = kDefaultSigmaLum; p.sigma_normal = kDefaultSigmaNormal; p.sigma_position = kDefaultSigmaPosition;
    p.firefly_ratio = kDefaultFireflyRatio; p.flags = kFlagDemodulate;
    return p;
}

// what is wrong with a record (a message for rtgl_last_error), or NULL
inline const char *invalid(const Params &p)
{
    if (p.passes > kMaxPasses) return "passes must be 0..8";
    if (!std::isfinite(p.sigma_color) || !std::isfinite(p.sigma_normal) || !std::isfinite(p.sigma_position)) return "the sigmas must be finite (<= 0 switches a term off)";
    if (p.flags & ~kFlagDemodulate) return "unknown flag bits";
    for (uint32_t r : p.reserved) if (r) return "reserved fields must be 0";
    return nullptr;
}
inline const char *invalid(const GuidedParams &p)
{
    if (p.passes > kMaxPasses) return "passes must be 0..8";
    if (!std::isfinite(p.sigma_lum) || !std::isfinite(p.sigma_normal) || !std::isfinite(p.sigma_position) || !std::isfinite(p.firefly_ratio))
        return "the sigmas and the firefly ratio must be finite (<= 0 switches the normal term, the position term or the clamp off)";
    if (!(p.sigma_lum > 0.0f)) return "sigma_lum must be > 0";
    if (p.flags & ~kFlagDemodulate) return "unknown flag bits";
    for (uint32_t r : p.reserved) if (r) return "reserved fields must be 0";
    return nullptr;
}

// the first-hit planes a valid record reads (bits of option "aov")
inline uint32_t planes_needed(uint32_t flags, float sigma_normal, float sigma_position)
{
    return ((flags & kFlagDemodulate) ? kPlaneAlbedo : 0u) | (sigma_normal > 0.0f ? kPlaneNormal : 0u) | (sigma_position > 0.0f ? kPlanePosition : 0u);
}
inline uint32_t planes_needed(const Params &p) { return planes_needed(p.flags, p.sigma_normal, p.sigma_position); }
inline uint32_t planes_needed(const GuidedParams &p) { return planes_needed(p.flags, p.sigma_normal, p.sigma_position); }

// what is wrong with what the two filters read (RTGL_ERR_STATE), or NULL: the context's pixels and, with option "denoise_source" = 1, the
// latest history of rtgl_temporal_accumulate
inline const char *input_refused(size_t px, int denoise_source, bool has_temporal)
{
    if (px == 0u) return "this context holds no pixels";
    if (denoise_source != 0 && !has_temporal) return "\"denoise_source\" is 1 and no rtgl_temporal_accumulate call has succeeded on this context";
    return nullptr;
}

// what is wrong with the history for a guided call (RTGL_ERR_STATE), or NULL: the options "denoise_variance" and "denoise_source", and the
// kind of moments the latest rtgl_temporal_accumulate stored (0: none)
inline const char *guided_variance_refused(int denoise_variance, int denoise_source, int stored_moments, bool demodulate)
{
    if (denoise_variance != 1) return nullptr;
    if (denoise_source != 1) return "\"denoise_variance\" is 1 and \"denoise_source\" is not: the temporal variance is that of the history";
    if (!stored_moments) return "\"denoise_variance\" is 1 and the latest rtgl_temporal_accumulate stored no moments (option \"temporal_moments\")";
    if (stored_moments != (demodulate ? 2 : 1))
        return "\"denoise_variance\" is 1 and the stored moments are of the other kind: RTGL_DENOISE_DEMODULATE needs \"temporal_moments\" = 2, a call without it 1";
    return nullptr;
}

// pass k of a call filters with step 1 << k
struct Pass { uint32_t tile_w, grid_x, grid_y; bool wide; };
inline Pass pass(uint32_t k, int width, int height)
{
    const int s = 1 << k;
    Pass g;
    g.tile_w = (uint32_t)(64 + 4 * s);
    g.grid_x = (uint32_t)((width + 63) / 64);
    g.grid_y = (uint32_t)(((height + 4 * s - 1) / (4 * s)) * s);
    g.wide = g.tile_w > kWideAbove;
    return g;
}
inline size_t lds_bytes(const Pass &g, uint32_t arrays) { return (size_t)2 * arrays * g.tile_w * sizeof(float); }

// the prepare kernel of the guided filter, and the identity kernel of rtgl_denoise with no pass
inline uint32_t prepare_grid_x(int width) { return (uint32_t)((width + 63) / 64); }
inline uint32_t prepare_grid_y(int height) { return (uint32_t)((height + 3) / 4); }
inline uint32_t identity_blocks(size_t n) { return (uint32_t)((n + 255) / 256); }

// the buffers of a call.  rtgl_denoise's pass k of K writes the denoised buffer (k = K - 1) or scratch k & 1; the guided prepare kernel
// writes scratch 0 whenever a pass follows, and pass k scratch (k + 1) & 1 or the denoised buffer
inline size_t pixels(int rows, int width) { return (size_t)rows * width; }
inline size_t record_bytes(size_t px) { return px * 16u; }         // the denoised, the scratch and the variance buffers
inline size_t near_bytes(size_t px) { return px * 4u; }
inline uint32_t scratch_buffers(uint32_t passes) { return passes < 1u ? 0u : (passes - 1u < 2u ? passes - 1u : 2u); }
inline uint32_t guided_scratch_buffers(uint32_t passes) { return passes < 2u ? passes : 2u; }

}  // namespace rt_denoise_plan
