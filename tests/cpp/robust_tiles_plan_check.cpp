// The host half of a robust adaptive session (raytracer.glsl_amd/csrc/rt_robust_tiles_plan.hpp) as a stand-alone program: the defaults, the
// validation of the parameter record, the bucket and the count of a tile's next sample, n_j and the sizes of the session's buffers; and, with
// rt_adaptive_plan.hpp as the session uses it, a session of several tiles replayed on the host: every tile's counts add up whatever the
// masks were.  Built by its test with the address and undefined-behaviour sanitizers (tests/test_robust_adaptive_abi.py).
#include <cstdio>
#include <initializer_list>
#include <limits>
#include <vector>
#include "../../raytracer.glsl_amd/csrc/rt_adaptive_plan.hpp"
#include "../../raytracer.glsl_amd/csrc/rt_robust_tiles_plan.hpp"

using namespace rt_robust_tiles_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // defaults
    {
        const Params p = default_params();
        CHECK(p.buckets == 8 && p.threshold == 0.05f && p.floor == 0.01f && p.gain == 1.0f && p.min_samples == 32 && p.max_samples == 1024 && p.flags == 0 && p.reserved == 0);
        CHECK(!invalid(p));
    }
    // the record
    for (uint32_t K = 0; K < 40; ++K) { Params p = default_params(); p.buckets = K; p.min_samples = 64; p.max_samples = 64; CHECK(!invalid(p) == (K == 4 || K == 8 || K == 16)); }
    { Params p = default_params(); p.buckets = 0xFFFFFFFFu; CHECK(invalid(p)); }
    for (float v : {nan, -nan, inf, -inf, 0.0f, -0.0f, -0.05f}) {
        { Params p = default_params(); p.threshold = v; CHECK(invalid(p)); }
        { Params p = default_params(); p.floor = v; CHECK(invalid(p)); }
    }
    for (float v : {1e-45f, 0.05f, 1e30f, std::numeric_limits<float>::max()}) {
        { Params p = default_params(); p.threshold = v; CHECK(!invalid(p)); }
        { Params p = default_params(); p.floor = v; CHECK(!invalid(p)); }
    }
    for (float g : {0.0f, -0.0f, 1.0f, 1e-45f, 1e30f, std::numeric_limits<float>::max()}) { Params p = default_params(); p.gain = g; CHECK(!invalid(p)); }
    for (float g : {nan, -nan, inf, -inf, -1.0f, -1e-45f}) { Params p = default_params(); p.gain = g; CHECK(invalid(p)); }
    for (uint32_t K : {4u, 8u, 16u}) {
        Params p = default_params();
        p.buckets = K;
        p.min_samples = K - 1; CHECK(invalid(p));
        p.min_samples = 0; CHECK(invalid(p));
        p.min_samples = K; CHECK(!invalid(p));
        p.max_samples = K; CHECK(!invalid(p));
        p.max_samples = K - 1; CHECK(invalid(p));
        p.min_samples = kMaxSamples; p.max_samples = kMaxSamples; CHECK(!invalid(p));
        p.max_samples = kMaxSamples + 1; CHECK(invalid(p));
        p.max_samples = 0xFFFFFFFFu; CHECK(invalid(p));
    }
    { Params p = default_params(); p.flags = 1; CHECK(invalid(p)); p.flags = 0x80000000u; CHECK(invalid(p)); }
    { Params p = default_params(); p.reserved = 1; CHECK(invalid(p)); p.reserved = 0x80000000u; CHECK(invalid(p)); }
    // (float) of every count up to the cap is exact
    CHECK((uint32_t)(float)kMaxSamples == kMaxSamples && (uint32_t)(float)(kMaxSamples - 1) == kMaxSamples - 1 && (float)(kMaxSamples + 1) == (float)kMaxSamples);
    // dealing a tile's samples
    for (uint32_t K : {4u, 8u, 16u}) {
        uint32_t held[16] = {};
        for (uint32_t n = 0; n < 3 * K + 2; ++n) {
            uint32_t sum = 0;
            for (uint32_t j = 0; j < K; ++j) { CHECK(bucket_samples(n, K, j) == held[j]); sum += held[j]; }
            CHECK(sum == n && estimated(n, K) == (held[K - 1] > 0));
            const uint32_t j = next_bucket(n, K);
            CHECK(j < K && next_count(n, K) == held[j]);
            held[j]++;
        }
        uint64_t sum = 0;
        for (uint32_t j = 0; j < K; ++j) sum += bucket_samples(kMaxSamples, K, j);
        CHECK(sum == kMaxSamples);
    }
    // a session of 5 x 4 tiles (70 x 53: a row and a column of tiles without footprint pixels) under changing masks
    {
        const rt_adaptive_plan::Shape sh = rt_adaptive_plan::shape(70, 53);
        const uint32_t n_tiles = (uint32_t)sh.tx * (uint32_t)sh.ty, K = 4;
        CHECK(n_tiles == 20 && sh.fw == 64 && sh.fh == 48);
        std::vector<uint32_t> n(n_tiles, 0);
        std::vector<uint8_t> want(n_tiles), mask;
        std::vector<uint32_t> blocks, tiles;
        std::vector<rt_adaptive_plan::Tile> records(n_tiles);
        for (uint32_t round = 0; round < 11; ++round) {
            for (uint32_t t = 0; t < n_tiles; ++t) want[t] = (uint8_t)((t + round) % 3 != 0);
            rt_adaptive_plan::explicit_mask(sh, want.data(), mask);
            rt_adaptive_plan::build_lists(sh, mask, blocks, tiles);
            uint32_t px = 0;
            for (uint32_t t : tiles) { CHECK(t < n_tiles && mask[t] && rt_adaptive_plan::tile_pixels(sh, t) > 0); px += rt_adaptive_plan::tile_pixels(sh, t); n[t]++; }
            CHECK(blocks.size() * 64u == px);
            for (uint32_t b : blocks) CHECK(b < sh.blocks_x * sh.blocks_y);
        }
        for (uint32_t t = 0; t < n_tiles; ++t) {
            records[t] = rt_adaptive_plan::Tile{};
            records[t].samples = records[t].samples_snapshot = n[t];
            records[t].count = estimated(n[t], K) ? 1u : 0u;
            records[t].converged = 1;
            CHECK(rt_adaptive_plan::tile_pixels(sh, t) ? n[t] >= 7 : n[t] == 0);
        }
        for (uint32_t t = 0; t < n_tiles; ++t) mask[t] = rt_adaptive_plan::active(sh, t, records[t], 8, 16) ? 1 : 0;
        const rt_adaptive_plan::Summary s = rt_adaptive_plan::summary(sh, records.data(), mask, 0, 16);
        CHECK(s.tiles_total == 12 && s.tiles_converged == 12 && s.samples_min == 7 && s.samples_max == 8 && s.tiles_active == 8 && s.converged == 0);
    }
    // sizes: 16 (K + 2) bytes per pixel, 40 per tile, 4 per block and tile; a picture without pixels owns one of each
    {
        const size_t px = plane_pixels(1920, 1080);
        CHECK(px == 2073600u && bucket_bytes(px, 8) + 2 * plane_bytes(px) == 2073600u * 160u);
        CHECK(plane_pixels(0, 64) == 1 && plane_pixels(64, 0) == 1 && plane_pixels(-3, 5) == 1 && plane_pixels(1, 1) == 1);
        CHECK(bucket_bytes(plane_pixels(65536, 65536), 16) == (size_t)65536 * 65536 * 256);      // no 32-bit product
        CHECK(count_bytes(20) == 160 && record_bytes(20) == 640 && list_bytes(48, 20) == 272);
        CHECK(count_bytes(0) == 8 && record_bytes(0) == 32 && list_bytes(0, 0) == 4 && list_bytes(0, 1) == 4);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("robust_tiles_plan_check: ok\n");
    return 0;
}
