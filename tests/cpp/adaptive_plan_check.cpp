// The host half of adaptive sampling (raytracer.glsl_amd/csrc/rt_adaptive_plan.hpp) as a stand-alone program: shapes, explicit masks, the
// block and tile lists, the mask rule and the summary against values tests/adaptive_mirror.py produced.  Built by its test with the
// address and undefined-behaviour sanitizers (tests/test_adaptive_abi.py).
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../raytracer.glsl_amd/csrc/rt_adaptive_plan.hpp"

using namespace rt_adaptive_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

using U8 = std::vector<uint8_t>;
using U32 = std::vector<uint32_t>;

static U32 iota(uint32_t n) { U32 v(n); for (uint32_t i = 0; i < n; ++i) v[i] = i; return v; }

static void lists(int w, int h, const U8 &given, const U8 &want_mask, const U32 &want_blocks, const U32 &want_tiles)
{
    const Shape s = shape(w, h);
    U8 mask; U32 blocks, tiles;
    CHECK(given.size() == (size_t)s.tx * s.ty);
    explicit_mask(s, given.data(), mask);
    build_lists(s, mask, blocks, tiles);
    CHECK(mask == want_mask); CHECK(blocks == want_blocks); CHECK(tiles == want_tiles);
    for (uint32_t b : blocks) CHECK(b < s.blocks_x * s.blocks_y);      // what the ray generator indexes the footprint with
    for (uint32_t t : tiles) CHECK(t < (uint32_t)(s.tx * s.ty) && tile_pixels(s, t) > 0);
}

static U8 checker(uint32_t n) { U8 v(n); for (uint32_t t = 0; t < n; ++t) v[t] = (uint8_t)((t % 2) * 255); return v; }

int main()
{
    // shapes
    { const Shape s = shape(1, 1); CHECK(s.tx == 1 && s.ty == 1 && s.fw == 0 && s.fh == 0 && s.blocks_x == 0 && s.blocks_y == 0 && tile_pixels(s, 0) == 0); }
    { const Shape s = shape(8, 8); CHECK(s.tx == 1 && s.ty == 1 && s.blocks_x == 1 && s.blocks_y == 1 && tile_pixels(s, 0) == 64); }
    {
        const Shape s = shape(24, 40);
        const uint32_t px[6] = {256, 128, 256, 128, 128, 64};
        CHECK(s.tx == 2 && s.ty == 3 && s.blocks_x == 3 && s.blocks_y == 5);
        for (uint32_t t = 0; t < 6; ++t) CHECK(tile_pixels(s, t) == px[t]);
    }
    {
        const Shape s = shape(70, 53);
        CHECK(s.tx == 5 && s.ty == 4 && s.fw == 64 && s.fh == 48 && s.blocks_x == 8 && s.blocks_y == 6);
        for (uint32_t t = 0; t < 20; ++t) CHECK(tile_pixels(s, t) == ((t % 5 < 4 && t / 5 < 3) ? 256u : 0u));
    }
    // masks and lists: full, then every other tile
    lists(1, 1, U8{1}, U8{0}, U32{}, U32{});
    lists(8, 8, U8{1}, U8{1}, U32{0}, U32{0});
    lists(8, 8, U8{0}, U8{0}, U32{}, U32{});
    lists(24, 40, U8(6, 1), U8(6, 1), iota(15), iota(6));
    lists(24, 40, checker(6), U8{0, 1, 0, 1, 0, 1}, U32{2, 5, 8, 11, 14}, U32{1, 3, 5});
    lists(70, 53, U8(20, 7), U8{1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0}, iota(48), U32{0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13});
    lists(70, 53, checker(20), U8{0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0},
          U32{2, 3, 6, 7, 10, 11, 14, 15, 16, 17, 20, 21, 24, 25, 28, 29, 34, 35, 38, 39, 42, 43, 46, 47}, U32{1, 3, 5, 7, 11, 13});
    // the rule and the summary, 70 x 53, min 4, max 8
    {
        const Shape s = shape(70, 53);
        const uint32_t samples[20] = {5, 6, 9, 11, 0, 1, 9, 11, 2, 3, 10, 5, 3, 9, 3, 4, 7, 6, 1, 0};
        const uint32_t count[20] = {200, 200, 200, 200, 200, 0, 0, 200, 0, 0, 0, 0, 200, 0, 0, 0, 200, 0, 200, 0};
        const uint32_t conv[20] = {0, 1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1};
        const uint32_t mse[20] = {0x3f041d12, 0x3ded4af3, 0x3f1f9d06, 0x3f46d4b4, 0x3f1cedc9, 0x3f6ad406, 0x3d222c24, 0x3f0751a0, 0x3eeb2e13, 0x3d7f6246,
                                  0x3f242e15, 0x3f5a4625, 0x3f17cafc, 0x3e852b7e, 0x3f57027a, 0x3f026e52, 0x3f02c99d, 0x3f40c696, 0x3e1778e0, 0x3f51d30f};
        const U8 want{1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0};
        std::vector<Tile> r(20);
        U8 mask(20);
        for (uint32_t t = 0; t < 20; ++t) {
            r[t] = Tile{};
            std::memcpy(&r[t].mse, &mse[t], 4);
            r[t].count = count[t]; r[t].converged = conv[t]; r[t].samples = samples[t];
            mask[t] = active(s, t, r[t], 4, 8) ? 1 : 0;
        }
        CHECK(mask == want);
        U32 blocks, tiles;
        build_lists(s, mask, blocks, tiles);
        const Summary su = summary(s, r.data(), mask, (uint32_t)blocks.size(), 8);
        uint32_t mx; std::memcpy(&mx, &su.max_tile_mse, 4);
        CHECK(su.tiles_total == 12 && su.tiles_active == 5 && su.tiles_converged == 2 && su.tiles_capped == 5 && su.blocks_active == 20);
        CHECK(su.samples_min == 1 && su.samples_max == 11 && su.converged == 0 && su.samples_total == 20736 && mx == 0x3f46d4b4);
        for (uint32_t v : su.reserved) CHECK(v == 0);
    }
    // the rule alone: the minimum keeps a converged tile active, the cap stops an unconverged one, a record without a count is not valid
    {
        const Shape s = shape(16, 16);
        Tile r{};
        r.samples = 3; r.count = 256; r.converged = 1;
        CHECK(active(s, 0, r, 4, 8) && !active(s, 0, r, 3, 8));
        r.samples = 8; r.converged = 0;
        CHECK(!active(s, 0, r, 4, 8) && active(s, 0, r, 4, 9));
        r.converged = 1; r.count = 0;
        CHECK(active(s, 0, r, 4, 9));
        CHECK(!active(shape(7, 7), 0, Tile{}, 4, 9));
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("adaptive_plan_check: ok\n");
    return 0;
}
