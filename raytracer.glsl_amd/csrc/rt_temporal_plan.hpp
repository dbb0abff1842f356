// The host half of rtgl_temporal_accumulate and rtgl_temporal_clip (include/rtgl_amd.h, "temporal accumulation" and "variance clipping"),
// as plain host C++: no HIP in this header, so that the host compiler can build it alone (tests/cpp/temporal_plan_check.cpp).  The
// defaults and the validation of the two parameter records, the planes a record needs and what state they must be in, whether the stored
// history can be used, the turn of the two buffer sets and the grid.  The camera record of a frame (temporal_camera) is the kernel
// header's struct and stays in rtgl_amd.hip.  tests/temporal_mirror.py and tests/temporal_clip_mirror.py restate the validation.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt_temporal_plan {

constexpr float kDefaultMaxHistory = 32.0f, kDefaultSigmaNormal = 0.3f, kDefaultSigmaPosition = 0.05f, kDefaultSigmaScale = 2.0f, kDefaultClipHistory = 3.0f;
constexpr uint32_t kPlaneAlbedo = 1u, kPlaneNormal = 2u, kPlanePosition = 4u;      // (RTGL_AOV_*)
constexpr uint32_t kTileW = 64u, kTileH = 4u;                                       // a block per 64 x 4 pixels

// rtgl_temporal_params, rtgl_temporal_clip_params
struct Params { float max_history, sigma_normal, sigma_position; uint32_t flags, reserved[4]; };
struct ClipParams { float sigma_scale, clip_history, sigma_normal, sigma_position; uint32_t flags, reserved[3]; };
static_assert(sizeof(Params) == 32 && sizeof(ClipParams) == 32, "the layouts of include/rtgl_amd.h");

inline Params default_params()
{
    Params p{};
    p.max_history = kDefaultMaxHistory; p.sigma_normal = kDefaultSigmaNormal; p.sigma_position = kDefaultSigmaPosition;
    return p;
}
inline ClipParams default_clip_params()
{
    ClipParams p{};
    p.sigma_scale = kDefaultSigmaScale; p.clip_history = kDefaultClipHistory; p.sigma_normal = kDefaultSigmaNormal; p.sigma_position = kDefaultSigmaPosition;
    return p;
}

// what is wrong with a record (a message for rtgl_last_error), or NULL
inline const char *invalid(const Params &p)
{
    if (!std::isfinite(p.max_history) || !std::isfinite(p.sigma_normal) || !std::isfinite(p.sigma_position)) return "max_history and the sigmas must be finite (a sigma <= 0 switches its test off)";
    if (!(p.max_history >= 1.0f)) return "max_history must be >= 1";
    if (p.flags) return "no flag bits are defined";
    for (uint32_t r : p.reserved) if (r) return "reserved fields must be 0";
    return nullptr;
}
inline const char *invalid(const ClipParams &p)
{
    if (!std::isfinite(p.sigma_scale) || !std::isfinite(p.clip_history) || !std::isfinite(p.sigma_normal) || !std::isfinite(p.sigma_position))
        return "sigma_scale, clip_history and the sigmas must be finite (a sigma <= 0 switches its term off)";
    if (!(p.sigma_scale > 0.0f)) return "sigma_scale must be > 0";
    if (!(p.clip_history >= 1.0f)) return "clip_history must be >= 1";
    if (p.flags) return "no flag bits are defined";
    for (uint32_t r : p.reserved) if (r) return "reserved fields must be 0";
    return nullptr;
}

// the first-hit planes a valid record reads (bits of option "aov"); `moments` is option "temporal_moments"
inline uint32_t planes_needed(const Params &p, int moments)
{
    return kPlanePosition | (p.sigma_normal > 0.0f ? kPlaneNormal : 0u) | (moments == 2 ? kPlaneAlbedo : 0u);
}
inline uint32_t planes_needed(const ClipParams &p) { return kPlanePosition | (p.sigma_normal > 0.0f ? kPlaneNormal : 0u); }

// what is wrong with the first-hit planes (RTGL_ERR_STATE), or NULL
inline const char *planes_refused(uint32_t needed, uint32_t enabled, bool restarted, uint32_t frames_in_planes, bool clip)
{
    if (needed & ~enabled)
        return clip ? "a first-hit plane this call needs is not enabled (option \"aov\": position always, for the kind test; normal for sigma_normal > 0)"
                    : "a first-hit plane this call needs is not enabled (option \"aov\": position always, normal for sigma_normal > 0, albedo for \"temporal_moments\" = 2)";
    if (restarted || frames_in_planes == 0u) return "no frame has been rendered since the first-hit planes last restarted";
    return nullptr;
}

// ... with the context's pixels, and for rtgl_temporal_clip with the history (RTGL_ERR_STATE), or NULL
inline const char *pixels_refused(size_t px) { return px == 0u ? "this context holds no pixels" : nullptr; }
inline const char *clip_refused(bool has_temporal) { return has_temporal ? nullptr : "no rtgl_temporal_accumulate call has succeeded on this context"; }

// the stored history takes part: there is one (no reset since), and it holds a normal plane if the normal test is on
inline bool history_usable(bool tm_valid, bool use_normal, bool tm_has_normal) { return tm_valid && !(use_normal && !tm_has_normal); }
// the two buffer sets take turns once a call has succeeded: the set a call that reads `from` writes
inline int turn(bool has_temporal, int from) { return has_temporal ? from ^ 1 : from; }

inline uint32_t grid_x(int width) { return (uint32_t)((width + 63) / 64); }
inline uint32_t grid_y(int height) { return (uint32_t)((height + 3) / 4); }
inline size_t pixels(int rows, int width) { return (size_t)rows * width; }
inline size_t record_bytes(size_t px) { return px * 16u; }         // a history, position, normal or moments buffer of one set

}  // namespace rt_temporal_plan
