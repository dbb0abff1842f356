// The host half of rtgl_robust_denoise (raytracer.glsl_amd/csrc/rt_bucket_guide_plan.hpp) as a stand-alone program: the defaults, the
// validation of the parameter record, the planes a record needs, the states that are refused, the grid of the prepare kernel, its LDS and
// the buffer sizes.  Built by its test with the address and undefined-behaviour sanitizers (tests/test_robust_denoise_abi.py).
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "../../raytracer.glsl_amd/csrc/rt_bucket_guide_plan.hpp"

using namespace rt_bucket_guide_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), big = std::numeric_limits<float>::max();
    // defaults
    {
        const Params p = default_params();
        CHECK(p.passes == 5u && p.sigma_lum == 4.0f && p.sigma_normal == 0.3f && p.sigma_position == 0.05f && p.gain == 1.0f && p.flags == kFlagDemodulate);
        for (uint32_t v : p.reserved) CHECK(v == 0);
        CHECK(!invalid(p) && demodulates(p) && planes_needed(p) == 7u);
    }
    // the record
    for (uint32_t k = 0; k < 20; ++k) { Params p = default_params(); p.passes = k; CHECK(!invalid(p) == (k <= 8)); }
    { Params p = default_params(); p.passes = 0xFFFFFFFFu; CHECK(invalid(p)); }
    for (float v : {1e-45f, 1e-6f, 1.0f, big}) { Params p = default_params(); p.sigma_lum = v; CHECK(!invalid(p)); }
    for (float v : {0.0f, -0.0f, -1.0f, -1e-45f, nan, -nan, inf, -inf}) { Params p = default_params(); p.sigma_lum = v; CHECK(invalid(p)); }
    for (float v : {0.0f, -0.0f, -1.0f, 1e-45f, 1.0f, big, -big}) {
        Params p = default_params(); p.sigma_normal = v; CHECK(!invalid(p));
        p = default_params(); p.sigma_position = v; CHECK(!invalid(p));
    }
    for (float v : {nan, -nan, inf, -inf}) {
        Params p = default_params(); p.sigma_normal = v; CHECK(invalid(p));
        p = default_params(); p.sigma_position = v; CHECK(invalid(p));
    }
    for (float g : {0.0f, -0.0f, 1e-45f, 1.0f, 1e30f, big}) { Params p = default_params(); p.gain = g; CHECK(!invalid(p)); }
    for (float g : {nan, -nan, inf, -inf, -1.0f, -1e-45f}) { Params p = default_params(); p.gain = g; CHECK(invalid(p)); }
    { Params p = default_params(); p.flags = 0; CHECK(!invalid(p) && !demodulates(p)); p.flags = 2; CHECK(invalid(p)); p.flags = 3; CHECK(invalid(p)); p.flags = 0x80000001u; CHECK(invalid(p)); }
    for (int k = 0; k < 2; ++k) { Params p = default_params(); p.reserved[k] = 1; CHECK(invalid(p)); }
    // the planes a record reads
    {
        Params p = default_params();
        p.sigma_normal = 0.0f; CHECK(planes_needed(p) == (kPlaneAlbedo | kPlanePosition));
        p.sigma_position = -1.0f; CHECK(planes_needed(p) == kPlaneAlbedo);
        p.flags = 0; CHECK(planes_needed(p) == 0u);
        p.sigma_normal = 1e-45f; CHECK(planes_needed(p) == kPlaneNormal);
    }
    // the session: open, and every bucket with a sample
    for (uint32_t K : {4u, 8u, 16u}) {
        CHECK(refused(false, 0, 0) && refused(false, 4 * K, K));
        for (uint32_t N = 0; N < K; ++N) CHECK(refused(true, N, K));
        for (uint32_t N : {K, K + 1, 3 * K + 2, 0xFFFFFFFFu}) CHECK(!refused(true, N, K));
    }
    // the planes: enabled, and holding a frame
    CHECK(!planes_refused(0, 0, true, 0) && !planes_refused(0, 7, false, 3));
    CHECK(!planes_refused(7, 7, false, 1) && !planes_refused(5, 15, false, 9) && !planes_refused(1, 1, false, 0xFFFFFFFFu));
    CHECK(planes_refused(7, 3, false, 1) && planes_refused(1, 6, false, 1) && planes_refused(4, 0, false, 1));
    CHECK(planes_refused(7, 7, true, 1) && planes_refused(7, 7, false, 0) && planes_refused(2, 7, true, 0));
    // grid, LDS and sizes
    CHECK(tiles_x(0) == 0 && tiles_x(-5) == 0 && tiles_x(1) == 1 && tiles_x(64) == 1 && tiles_x(65) == 2 && tiles_x(1920) == 30 && tiles_x(0x7FFFFFFF) == 0x2000000u);
    CHECK(tiles_y(0) == 0 && tiles_y(-1) == 0 && tiles_y(1) == 1 && tiles_y(4) == 1 && tiles_y(5) == 2 && tiles_y(1080) == 270 && tiles_y(0x7FFFFFFF) == 0x20000000u);
    CHECK(kLdsBytes == 9504u && kHaloW == 66u && kHaloH == 6u && kGuideArrays == 6u);
    CHECK(pixels(0, 5) == 0 && pixels(5, 0) == 0 && pixels(-1, 5) == 0 && pixels(53, 70) == 3710u && pixels(1080, 1920) == 2073600u);
    CHECK(pixels(0x7FFFFFFF, 0x7FFFFFFF) == (size_t)0x7FFFFFFF * 0x7FFFFFFF);      // no 32-bit product
    CHECK(record_bytes(3710) == 59360u && near_bytes(3710) == 14840u && record_bytes(pixels(65536, 65536)) == ((size_t)1 << 36));
    CHECK(scratch_buffers(0) == 0 && scratch_buffers(1) == 1 && scratch_buffers(2) == 2 && scratch_buffers(8) == 2);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("bucket_guide_plan_check: ok\n");
    return 0;
}
