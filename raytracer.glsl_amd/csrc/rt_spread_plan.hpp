// The host half of rtgl_robust_error_estimate (include/rtgl_amd.h, "robust error estimate"), as plain host C++: no HIP in this header, so
// that the host compiler can build it alone (tests/cpp/spread_plan_check.cpp).  The defaults and the validation of the parameter record,
// what state a session must be in, the footprint, the tile grid and the sizes of the two buffers, and h and the divisor of Yuen's
// variance for a trim.  tests/robust_error_mirror.py restates the validation, the states and the footprint.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt_spread_plan {

constexpr float kDefaultThreshold = 0.05f, kDefaultFloor = 0.01f, kDefaultGain = 1.0f;
constexpr uint32_t kDefaultQuantile = 950u, kTile = 16u, kSummaryBytes = 64u, kRecordBytes = 16u;

// rtgl_robust_error_params
struct Params { float threshold, floor, gain; uint32_t quantile_permille, flags, reserved[3]; };
static_assert(sizeof(Params) == 32, "the layout of include/rtgl_amd.h");

inline Params default_params()
{
    Params p{};
    p.threshold = kDefaultThreshold; p.floor = kDefaultFloor; p.gain = kDefaultGain; p.quantile_permille = kDefaultQuantile;
    return p;
}

// what is wrong with a record (a message for rtgl_last_error), or NULL
inline const char *invalid(const Params &p)
{
    if (!std::isfinite(p.threshold) || !(p.threshold > 0.0f) || !std::isfinite(p.floor) || !(p.floor > 0.0f)) return "threshold and floor must be finite and > 0";
    if (!std::isfinite(p.gain) || !(p.gain >= 0.0f)) return "gain must be finite and >= 0";
    if (p.quantile_permille < 1u || p.quantile_permille > 1000u) return "quantile_permille must be in 1..1000";
    if (p.flags) return "no flag is defined";
    for (uint32_t r : p.reserved) if (r) return "reserved fields must be 0";
    return nullptr;
}

// what is wrong with the session (RTGL_ERR_STATE), or NULL: every bucket must hold a sample
inline const char *refused(bool session, uint32_t N, uint32_t K)
{
    if (!session) return "no session (rtgl_robust_begin has not been called, or rtgl_robust_end has)";
    if (N < K) return "fewer frames than buckets: an empty bucket has no luminance";
    return nullptr;
}

// the footprint of rtgl_error_estimate and its tiles
inline uint32_t footprint_side(int v) { return v > 0 ? (uint32_t)v / 8u * 8u : 0u; }
inline uint64_t footprint(int width, int height) { return (uint64_t)footprint_side(width) * (uint64_t)footprint_side(height); }
inline bool footprint_fits(int width, int height) { return footprint(width, height) <= 0xFFFFFFFFull; }
inline uint32_t tiles_along(int v) { return v > 0 ? ((uint32_t)v + kTile - 1u) / kTile : 0u; }
inline size_t record_bytes(int width, int height) { const size_t n = (size_t)tiles_along(width) * (size_t)tiles_along(height); return (n ? n : 1u) * kRecordBytes; }

// a trim of t at either end of K buckets keeps h = K - 2 t >= 2 of them; Yuen's variance divides by h (h - 1)
inline uint32_t kept(uint32_t K, uint32_t t) { return K - 2u * t; }
inline uint32_t yuen_divisor(uint32_t K, uint32_t t) { const uint32_t h = kept(K, t); return h * (h - 1u); }

}  // namespace rt_spread_plan
