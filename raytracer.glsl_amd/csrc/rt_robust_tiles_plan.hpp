// The host half of a robust adaptive session (include/rtgl_amd.h, "robust adaptive sampling"), as plain host C++: no HIP in this header, so
// that the host compiler can build it alone (tests/cpp/robust_tiles_plan_check.cpp).  The defaults and the validation of the parameter
// record, the bucket a tile's next sample goes to and the samples a bucket holds after n of them, and the sizes of the session's buffers.
// The shapes, the mask rule, the lists and the summary are rt_adaptive_plan.hpp's, used as they are.
// tests/robust_adaptive_mirror.py restates every function here.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt_robust_tiles_plan {

constexpr uint32_t kDefaultBuckets = 8u, kDefaultMinSamples = 32u, kDefaultMaxSamples = 1024u;
constexpr float kDefaultThreshold = 0.05f, kDefaultFloor = 0.01f, kDefaultGain = 1.0f;
// (float) of every count up to here is exact
constexpr uint32_t kMaxSamples = 16777216u;

// rtgl_robust_adaptive_params
struct Params { uint32_t buckets; float threshold, floor, gain; uint32_t min_samples, max_samples, flags, reserved; };
static_assert(sizeof(Params) == 32, "the layout of include/rtgl_amd.h");

inline Params default_params()
{
    Params p{};
    p.buckets = kDefaultBuckets; p.threshold = kDefaultThreshold; p.floor = kDefaultFloor; p.gain = kDefaultGain;
    p.min_samples = kDefaultMinSamples; p.max_samples = kDefaultMaxSamples;
    return p;
}

inline bool valid_buckets(uint32_t K) { return K == 4u || K == 8u || K == 16u; }

// what is wrong with a record (a message for rtgl_last_error), or NULL
inline const char *invalid(const Params &p)
{
    if (!valid_buckets(p.buckets)) return "buckets must be 4, 8 or 16";
    if (!std::isfinite(p.threshold) || !(p.threshold > 0.0f) || !std::isfinite(p.floor) || !(p.floor > 0.0f)) return "threshold and floor must be finite and > 0";
    if (!std::isfinite(p.gain) || !(p.gain >= 0.0f)) return "gain must be finite and >= 0";
    if (p.min_samples < p.buckets) return "min_samples must be >= buckets: a tile is estimated once every bucket holds a sample";
    if (p.max_samples < p.min_samples || p.max_samples > kMaxSamples) return "min_samples <= max_samples <= 16777216 is required";
    if (p.flags) return "no flag is defined";
    if (p.reserved) return "reserved fields must be 0";
    return nullptr;
}

// sample n (counted from 0) of a tile goes to bucket n mod K, which holds n div K samples before it
inline uint32_t next_bucket(uint32_t n, uint32_t K) { return n % K; }
inline uint32_t next_count(uint32_t n, uint32_t K) { return n / K; }
// n_j: the samples bucket j of a tile holds after n of them
inline uint32_t bucket_samples(uint32_t n, uint32_t K, uint32_t j) { return n / K + (j < n % K ? 1u : 0u); }
// a tile is estimated once every bucket holds a sample
inline bool estimated(uint32_t n, uint32_t K) { return n >= K; }

// one plane: the image's pixels as float4 (an image without pixels still owns one); K of them bucket-major; the sample buffer and the output
// plane are one plane each; n per tile, then m per tile; two uint4 per tile; the active blocks, then the active tiles
inline size_t plane_pixels(int width, int height) { const size_t n = (size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0); return n ? n : 1u; }
inline size_t plane_bytes(size_t plane_px) { return plane_px * 16u; }
inline size_t bucket_bytes(size_t plane_px, uint32_t K) { return plane_px * 16u * (size_t)K; }
inline size_t count_bytes(size_t n_tiles) { return 2u * (n_tiles ? n_tiles : 1u) * sizeof(uint32_t); }
inline size_t record_bytes(size_t n_tiles) { return (n_tiles ? n_tiles : 1u) * 32u; }
inline size_t list_bytes(size_t n_blocks, size_t n_tiles) { const size_t n = n_blocks + n_tiles; return (n ? n : 1u) * sizeof(uint32_t); }

}  // namespace rt_robust_tiles_plan
