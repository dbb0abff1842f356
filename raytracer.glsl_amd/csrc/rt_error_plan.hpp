// The host half of rtgl_error_estimate (include/rtgl_amd.h, "error estimate"), as plain host C++: no HIP in this header, so that the host
// compiler can build it alone (tests/cpp/error_plan_check.cpp).  The defaults and the validation of the parameter record, the snapshot's
// life (which events drop it, when a call can use it, what a call leaves behind), the three factors of the estimate, the footprint, the
// tile grid and the buffer sizes.  tests/error_mirror.py (Estimator) restates the snapshot's life and the factors.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt_error_plan {

constexpr float kDefaultThreshold = 0.05f, kDefaultFloor = 0.01f;
constexpr uint32_t kDefaultQuantile = 950u, kFlagKeep = 1u;                       // (RTGL_ERROR_KEEP_SNAPSHOT)
constexpr int32_t kDefaultFirstFrames = 1;
constexpr uint32_t kTile = 16u, kSummaryBytes = 64u, kRecordBytes = 16u;
constexpr int kInvalid = -1, kState = -4;                                         // (RTGL_ERR_INVALID, RTGL_ERR_STATE)

// rtgl_error_params
struct Params { float threshold, floor; uint32_t quantile_permille; int32_t first_frames; uint32_t flags, reserved[3]; };
static_assert(sizeof(Params) == 32, "the layout of include/rtgl_amd.h");

inline Params default_params()
{
    Params p{};
    p.threshold = kDefaultThreshold; p.floor = kDefaultFloor; p.quantile_permille = kDefaultQuantile; p.first_frames = kDefaultFirstFrames;
    return p;
}

// what is wrong with a record (a message for rtgl_last_error), or NULL
inline const char *invalid(const Params &p)
{
    if (!std::isfinite(p.threshold) || !(p.threshold > 0.0f) || !std::isfinite(p.floor) || !(p.floor > 0.0f)) return "threshold and floor must be finite and > 0";
    if (p.quantile_permille < 1u || p.quantile_permille > 1000u) return "quantile_permille must be in 1..1000";
    if (p.first_frames < 0) return "first_frames must be >= 0";
    if (p.flags & ~kFlagKeep) return "only flag bit 0 (keep the snapshot) is defined";
    for (uint32_t r : p.reserved) if (r) return "reserved fields must be 0";
    return nullptr;
}

// What a context knows of its accumulation and of the snapshot.  The snapshot is usable while snap_epoch == epoch: every event that drops
// it (header, "error estimate") advances epoch.  fm, first: the snapshot's `frames` and first_frames; rendered, fn: a frame has been
// rendered, and its `frames`
struct Snapshot { uint64_t epoch = 1, snap_epoch = 0; int32_t fm = 0, first = 0, fn = 0; bool rendered = false; };

inline void drop(Snapshot &s) { ++s.epoch; }
// a frame with these uniforms has been rendered into the image
inline void rendered_frame(Snapshot &s, int32_t frames, bool reset_flag)
{
    if (reset_flag) drop(s);
    s.fn = frames; s.rendered = true;
}

// the footprint (the whole 8 x 8 blocks of the picture), the 16 x 16 tiles and the buffers
inline uint32_t footprint_side(int v) { return v > 0 ? (uint32_t)v / 8u * 8u : 0u; }
inline uint64_t footprint(int width, int height) { return (uint64_t)footprint_side(width) * (uint64_t)footprint_side(height); }
inline bool footprint_fits(int width, int height) { return footprint(width, height) <= 0xFFFFFFFFull; }
inline uint32_t tiles_along(int v) { return v > 0 ? ((uint32_t)v + kTile - 1u) / kTile : 0u; }
inline size_t record_bytes(int width, int height) { const size_t n = (size_t)tiles_along(width) * (size_t)tiles_along(height); return (n ? n : 1u) * kRecordBytes; }
inline size_t snapshot_bytes(int width, int height) { return (size_t)height * width * sizeof(float); }      // one luminance per pixel

// what is wrong with the accumulation or the picture for these parameters, or a NULL text: a state, a first_frames the latest frame does
// not reach, or a picture too large
struct Refusal { int code; const char *why; };
inline Refusal refused(const Snapshot &s, const Params &p, int width, int height)
{
    if (!s.rendered) return { kState, "no frame has been rendered on this context" };
    if ((int64_t)s.fn + 1 - (int64_t)p.first_frames < 1) return { kInvalid, "the latest frame's `frames` is below first_frames: the image would hold no frame" };
    if (!footprint_fits(width, height)) return { kInvalid, "the footprint does not fit 32-bit counts" };
    return { 0, nullptr };
}

// What a call that is not refused does.  usable: the snapshot is of an earlier moment of THIS accumulation, counted the same way; keep: it
// stays for the next call.  With n and m the frames in the image now and in the snapshot: g_n and g_m rescale the two images to their
// means over those frames and c = m / (n - m) turns the squared difference into the variance of the image now.  All 0 without a snapshot
struct Plan { bool usable, keep; float g_n, g_m, c; int32_t frames_now, frames_snapshot; };
inline Plan plan(const Snapshot &s, const Params &p)
{
    Plan q{};
    const int64_t fn = s.fn, n = fn + 1 - (int64_t)p.first_frames;
    q.usable = s.snap_epoch == s.epoch && fn > (int64_t)s.fm && p.first_frames == s.first;
    q.keep = q.usable && (p.flags & kFlagKeep);
    if (q.usable) {
        const int64_t m = (int64_t)s.fm + 1 - (int64_t)p.first_frames;      // (>= 1: the call that took the snapshot checked it)
        q.g_n = (float)((double)(fn + 1) / (double)n);
        q.g_m = (float)((double)((int64_t)s.fm + 1) / (double)m);
        q.c = (float)((double)m / (double)(n - m));
        q.frames_now = (int32_t)fn; q.frames_snapshot = s.fm;
    }
    return q;
}
// after the call: unless the snapshot was kept, the image now is the new one
inline void taken(Snapshot &s, const Params &p, bool keep)
{
    if (!keep) { s.snap_epoch = s.epoch; s.fm = s.fn; s.first = p.first_frames; }
}

}  // namespace rt_error_plan
