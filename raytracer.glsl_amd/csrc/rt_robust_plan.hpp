// The host half of robust accumulation (include/rtgl_amd.h, "robust accumulation"), as plain host C++: no HIP in this header, so that the
// host compiler can build it alone (tests/cpp/robust_plan_check.cpp).  Which bucket the next frame goes to and how many samples it holds,
// how many samples bucket j holds after N frames, the cap of the trim, the validation of the two parameter records and the sizes of the
// planes.  tests/robust_mirror.py restates every function here.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rt_robust_plan {

constexpr uint32_t kDefaultBuckets = 8u, kDestBuffer = 0u, kDestImage = 1u;
constexpr float kDefaultGain = 1.0f;

// rtgl_robust_params and rtgl_robust_resolve_params
struct Params { uint32_t buckets, flags, reserved[6]; };
struct ResolveParams { float gain; uint32_t dest, flags, reserved[5]; };
static_assert(sizeof(Params) == 32 && sizeof(ResolveParams) == 32, "the layouts of include/rtgl_amd.h");

inline Params default_params() { Params p{}; p.buckets = kDefaultBuckets; return p; }
inline ResolveParams default_resolve_params() { ResolveParams p{}; p.gain = kDefaultGain; p.dest = kDestBuffer; return p; }

inline bool valid_buckets(uint32_t K) { return K == 4u || K == 8u || K == 16u; }

// what is wrong with a record (a message for rtgl_last_error), or NULL
inline const char *invalid(const Params &p)
{
    if (!valid_buckets(p.buckets)) return "buckets must be 4, 8 or 16";
    if (p.flags) return "no flag is defined";
    for (uint32_t r : p.reserved) if (r) return "reserved fields must be 0";
    return nullptr;
}
inline const char *invalid(const ResolveParams &p)
{
    if (!std::isfinite(p.gain) || !(p.gain >= 0.0f)) return "gain must be finite and >= 0";
    if (p.dest > kDestImage) return "dest must be RTGL_ROBUST_DEST_BUFFER or RTGL_ROBUST_DEST_IMAGE";
    if (p.flags) return "no flag is defined";
    for (uint32_t r : p.reserved) if (r) return "reserved fields must be 0";
    return nullptr;
}

// frame N (counted from 0) goes to bucket N mod K, which holds N div K samples before it
inline uint32_t next_bucket(uint32_t N, uint32_t K) { return N % K; }
inline uint32_t next_count(uint32_t N, uint32_t K) { return N / K; }
// n_j: the samples bucket j holds after N frames
inline uint32_t bucket_samples(uint32_t N, uint32_t K, uint32_t j) { return N / K + (j < N % K ? 1u : 0u); }
// the most buckets the resolve drops at either end: at least one (K even: two) stays
inline uint32_t trim_cap(uint32_t K) { return (K - 1u) / 2u; }
// the frame counter is 32 bits wide: the fold after this many is refused
constexpr uint32_t kMaxFrames = 0xFFFFFFFFu;

// one plane: the context's rows of float4 (a context without rows still owns one); K of them bucket-major, then the output plane
inline size_t plane_pixels(int local_rows, int width) { return (size_t)(local_rows > 1 ? local_rows : 1) * (size_t)width; }
inline size_t bucket_bytes(size_t plane_px, uint32_t K) { return plane_px * 16u * (size_t)K; }
inline size_t output_bytes(size_t plane_px) { return plane_px * 16u; }

}  // namespace rt_robust_plan
