// The host half of robust accumulation (raytracer.glsl_amd/csrc/rt_robust_plan.hpp) as a stand-alone program: the bucket and the count of
// the next frame, n_j, the cap of the trim, the validation of both parameter records and the plane sizes.  Built by its test with the
// address and undefined-behaviour sanitizers (tests/test_robust_abi.py).
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "../../raytracer.glsl_amd/csrc/rt_robust_plan.hpp"

using namespace rt_robust_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main()
{
    // defaults
    {
        const Params p = default_params();
        const ResolveParams r = default_resolve_params();
        CHECK(p.buckets == 8 && p.flags == 0 && r.gain == 1.0f && r.dest == kDestBuffer && r.flags == 0);
        for (uint32_t v : p.reserved) CHECK(v == 0);
        for (uint32_t v : r.reserved) CHECK(v == 0);
        CHECK(!invalid(p) && !invalid(r));
    }
    // dealing the frames: a session replayed frame by frame against n_j
    for (uint32_t K : {4u, 8u, 16u}) {
        uint32_t held[16] = {};
        for (uint32_t N = 0; N < 3 * K + 2; ++N) {
            uint32_t sum = 0;
            for (uint32_t j = 0; j < K; ++j) { CHECK(bucket_samples(N, K, j) == held[j]); sum += held[j]; }
            CHECK(sum == N);
            const uint32_t j = next_bucket(N, K);
            CHECK(j < K && j == N % K && next_count(N, K) == held[j]);
            held[j]++;
        }
        // the counter's last values: no wrap
        CHECK(next_bucket(kMaxFrames, K) == K - 1 && next_count(kMaxFrames, K) == kMaxFrames / K);
        uint64_t sum = 0;
        for (uint32_t j = 0; j < K; ++j) sum += bucket_samples(kMaxFrames, K, j);
        CHECK(sum == kMaxFrames);
    }
    CHECK(trim_cap(4) == 1 && trim_cap(8) == 3 && trim_cap(16) == 7);
    // buckets
    for (uint32_t K = 0; K < 40; ++K) { Params p = default_params(); p.buckets = K; CHECK(!invalid(p) == (K == 4 || K == 8 || K == 16)); }
    { Params p = default_params(); p.buckets = 0xFFFFFFFFu; CHECK(invalid(p)); }
    { Params p = default_params(); p.flags = 1; CHECK(invalid(p)); p.flags = 0x80000000u; CHECK(invalid(p)); }
    for (int k = 0; k < 6; ++k) { Params p = default_params(); p.reserved[k] = 1; CHECK(invalid(p)); }
    // the resolve's record
    {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        for (float g : {0.0f, -0.0f, 1.0f, 1e-45f, 1e30f, std::numeric_limits<float>::max()}) { ResolveParams r = default_resolve_params(); r.gain = g; CHECK(!invalid(r)); }
        for (float g : {nan, -nan, inf, -inf, -1.0f, -1e-45f}) { ResolveParams r = default_resolve_params(); r.gain = g; CHECK(invalid(r)); }
        for (uint32_t d : {0u, 1u}) { ResolveParams r = default_resolve_params(); r.dest = d; CHECK(!invalid(r)); }
        for (uint32_t d : {2u, 3u, 0xFFFFFFFFu}) { ResolveParams r = default_resolve_params(); r.dest = d; CHECK(invalid(r)); }
        { ResolveParams r = default_resolve_params(); r.flags = 4; CHECK(invalid(r)); }
        for (int k = 0; k < 5; ++k) { ResolveParams r = default_resolve_params(); r.reserved[k] = 7; CHECK(invalid(r)); }
    }
    // sizes: 16 (K + 1) bytes per pixel; a context without rows owns one
    CHECK(plane_pixels(1080, 1920) == 2073600u && bucket_bytes(2073600u, 8) + output_bytes(2073600u) == 298598400u);
    CHECK(plane_pixels(0, 64) == 64 && plane_pixels(1, 64) == 64 && plane_pixels(32, 64) == 2048);
    CHECK(bucket_bytes(plane_pixels(65536, 65536), 16) == (size_t)65536 * 65536 * 256);      // no 32-bit product
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("robust_plan_check: ok\n");
    return 0;
}
