// The host half of rtgl_tonemap (include/rtgl_amd.h, "display transform"), as plain host C++: no HIP in this header, so that the host
// compiler can build it alone (tests/cpp/tonemap_plan_check.cpp).  The defaults and the validation of the parameter record, which
// buffers a source needs, the blocks of the histogram and the map kernels, the layout of the state words and the turn of the two
// histogram sets.  tests/tonemap_mirror.py restates the validation.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt_tonemap_plan {

constexpr uint32_t kSourceImage = 0u, kSourceDenoised = 1u, kSourceTemporal = 2u;      // (RTGL_TONEMAP_SOURCE_*)
constexpr uint32_t kOpLinear = 0u, kOpReinhard = 1u, kOpAces = 2u;                     // (RTGL_TONEMAP_LINEAR, _REINHARD, _ACES)
constexpr uint32_t kFlagAuto = 1u;                                                     // (RTGL_TONEMAP_AUTO_EXPOSURE)
constexpr float kDefaultExposure = 1.0f, kDefaultKey = 0.18f, kDefaultWhite = 4.0f, kDefaultAdapt = 1.0f, kDefaultExposureMin = 0x1p-16f, kDefaultExposureMax = 0x1p16f;
constexpr uint32_t kDefaultLowPermille = 100u, kDefaultHighPermille = 20u;
// the state words: two histogram sets of 256 bins and a count of ignored pixels each, then the exposure and a spare word
constexpr int kBins = 256, kSetWords = kBins + 1, kExposureWord = 2 * kSetWords, kStateWords = kExposureWord + 2;
constexpr size_t kBlocksPerCu = 8u;

// rtgl_tonemap_params
struct Params { uint32_t source, op, flags; float exposure, key, white, adapt, exposure_min, exposure_max; uint32_t low_permille, high_permille, reserved[5]; };
static_assert(sizeof(Params) == 64, "the layout of include/rtgl_amd.h");

inline Params default_params()
{
    Params p{};
    p.source = kSourceImage; p.op = kOpReinhard; p.flags = kFlagAuto;
    p.exposure = kDefaultExposure; p.key = kDefaultKey; p.white = kDefaultWhite; p.adapt = kDefaultAdapt;
    p.exposure_min = kDefaultExposureMin; p.exposure_max = kDefaultExposureMax;
    p.low_permille = kDefaultLowPermille; p.high_permille = kDefaultHighPermille;
    return p;
}

// what is wrong with a record (a message for rtgl_last_error), or NULL
inline const char *invalid(const Params &p)
{
    if (p.source > kSourceTemporal) return "source must be 0 (image), 1 (denoised) or 2 (temporal history)";
    if (p.op > kOpAces) return "op must be 0 (linear), 1 (Reinhard with white point) or 2 (ACES fit)";
    if (p.flags & ~kFlagAuto) return "only flag bit 0 (auto exposure) is defined";
    const float positive[] = { p.exposure, p.key, p.white, p.adapt, p.exposure_min, p.exposure_max };
    for (float v : positive)
        if (!std::isfinite(v) || !(v > 0.0f)) return "exposure, key, white, adapt, exposure_min and exposure_max must be finite and > 0";
    if (p.adapt > 1.0f) return "adapt must be in (0, 1]";
    if (p.exposure_min > p.exposure_max) return "exposure_min must not exceed exposure_max";
    if ((uint64_t)p.low_permille + (uint64_t)p.high_permille >= 1000u) return "low_permille + high_permille must be < 1000";
    for (uint32_t r : p.reserved) if (r) return "reserved fields must be 0";
    return nullptr;
}

inline bool automatic(const Params &p) { return (p.flags & kFlagAuto) != 0u; }

// what is wrong with the buffer a valid source names (RTGL_ERR_STATE), or NULL
inline const char *source_refused(uint32_t source, bool has_denoised, bool has_temporal)
{
    if (source == kSourceDenoised && !has_denoised) return "source 1, and no rtgl_denoise or rtgl_denoise_guided call has succeeded on this context";
    if (source == kSourceTemporal && !has_temporal) return "source 2, and no rtgl_temporal_accumulate call has succeeded on this context";
    return nullptr;
}
inline const char *pixels_refused(size_t px) { return px == 0u ? "this context holds no pixels" : nullptr; }

// the histogram and the map kernels stride over n pixels: a block per 256 of them, eight per compute unit at the most
inline uint32_t blocks(size_t n, int n_cus) { const size_t want = (n + 255) / 256, cap = (size_t)n_cus * kBlocksPerCu; return (uint32_t)(want < cap ? want : cap); }
inline size_t display_bytes(size_t px) { return px * 4u; }

// the two histogram sets take turns.  set: the one the next auto call counts in (its solve clears the other); hist_set: the one the latest
// auto call counted in (-1: none yet); prev: the state holds an exposure stored since the last rtgl_tonemap_reset
struct Sets {
    int set = 0, hist_set = -1; bool prev = false;
    void after_auto_call() { hist_set = set; set ^= 1; prev = true; }
};

}  // namespace rt_tonemap_plan
