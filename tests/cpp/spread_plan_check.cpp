// The host half of rtgl_robust_error_estimate (raytracer.glsl_amd/csrc/rt_spread_plan.hpp) as a stand-alone program: the defaults, the
// validation of the parameter record, the states that are refused, the footprint, the tile grid, the buffer sizes and the divisor of
// Yuen's variance.  Built by its test with the address and undefined-behaviour sanitizers (tests/test_robust_error_abi.py).
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "../../raytracer.glsl_amd/csrc/rt_spread_plan.hpp"

using namespace rt_spread_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), big = std::numeric_limits<float>::max();
    // defaults
    {
        const Params p = default_params();
        CHECK(p.threshold == 0.05f && p.floor == 0.01f && p.gain == 1.0f && p.quantile_permille == 950u && p.flags == 0u);
        for (uint32_t v : p.reserved) CHECK(v == 0);
        CHECK(!invalid(p));
    }
    // the record
    for (float v : {1e-45f, 1e-6f, 1.0f, big}) {
        Params p = default_params(); p.threshold = v; CHECK(!invalid(p));
        p = default_params(); p.floor = v; CHECK(!invalid(p));
    }
    for (float v : {0.0f, -0.0f, -1.0f, -1e-45f, nan, -nan, inf, -inf}) {
        Params p = default_params(); p.threshold = v; CHECK(invalid(p));
        p = default_params(); p.floor = v; CHECK(invalid(p));
    }
    for (float g : {0.0f, -0.0f, 1e-45f, 1.0f, 1e30f, big}) { Params p = default_params(); p.gain = g; CHECK(!invalid(p)); }
    for (float g : {nan, -nan, inf, -inf, -1.0f, -1e-45f}) { Params p = default_params(); p.gain = g; CHECK(invalid(p)); }
    for (uint32_t q = 0; q < 1100; ++q) { Params p = default_params(); p.quantile_permille = q; CHECK(!invalid(p) == (q >= 1 && q <= 1000)); }
    { Params p = default_params(); p.quantile_permille = 0xFFFFFFFFu; CHECK(invalid(p)); }
    { Params p = default_params(); p.flags = 1; CHECK(invalid(p)); p.flags = 0x80000000u; CHECK(invalid(p)); }
    for (int k = 0; k < 3; ++k) { Params p = default_params(); p.reserved[k] = 1; CHECK(invalid(p)); }
    // the session: open, and every bucket with a sample
    for (uint32_t K : {4u, 8u, 16u}) {
        CHECK(refused(false, 0, 0) && refused(false, 4 * K, K));
        for (uint32_t N = 0; N < K; ++N) CHECK(refused(true, N, K));
        for (uint32_t N : {K, K + 1, 2 * K + 3, 0xFFFFFFFFu}) CHECK(!refused(true, N, K));
    }
    // footprint, tiles and sizes
    CHECK(footprint_side(0) == 0 && footprint_side(-3) == 0 && footprint_side(7) == 0 && footprint_side(8) == 8 && footprint_side(70) == 64 && footprint_side(1920) == 1920 && footprint_side(1080) == 1080);
    CHECK(footprint(7, 5) == 0 && footprint(1, 1) == 0 && footprint(17, 17) == 256 && footprint(70, 53) == 64 * 48 && footprint(1920, 1080) == 2073600u);
    CHECK(footprint_fits(65535, 65535) && footprint_fits(65536, 65528) && !footprint_fits(65536, 65536) && !footprint_fits(0x7FFFFFFF, 0x7FFFFFFF));
    CHECK(tiles_along(0) == 0 && tiles_along(1) == 1 && tiles_along(16) == 1 && tiles_along(17) == 2 && tiles_along(1080) == 68 && tiles_along(0x7FFFFFFF) == 0x8000000u);
    CHECK(record_bytes(1, 1) == 16 && record_bytes(17, 17) == 64 && record_bytes(1920, 1080) == 120u * 68u * 16u && record_bytes(0, 0) == 16);
    CHECK(record_bytes(0x7FFFFFFF, 0x7FFFFFFF) == (size_t)0x8000000u * 0x8000000u * 16u);      // no 32-bit product
    CHECK(kSummaryBytes == 64 && kRecordBytes == 16 && kTile == 16);
    // h >= 2 for every trim up to the cap (K - 1) / 2
    for (uint32_t K : {4u, 8u, 16u})
        for (uint32_t t = 0; t <= (K - 1) / 2; ++t) {
            CHECK(kept(K, t) == K - 2 * t && kept(K, t) >= 2 && kept(K, t) % 2 == 0);
            CHECK(yuen_divisor(K, t) == kept(K, t) * (kept(K, t) - 1) && yuen_divisor(K, t) >= 2);
        }
    CHECK(yuen_divisor(8, 0) == 56 && yuen_divisor(8, 3) == 2 && yuen_divisor(16, 0) == 240 && yuen_divisor(4, 1) == 2);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("spread_plan_check: ok\n");
    return 0;
}
