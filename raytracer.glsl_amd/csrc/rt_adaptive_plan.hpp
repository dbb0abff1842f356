// The host half of adaptive sampling (include/rtgl_amd.h, "adaptive sampling"), as plain host C++: no HIP in this header, so that the host
// compiler can build it alone (tests/cpp/adaptive_plan_check.cpp).  The shapes, the mask rule, the block list a masked frame's ray
// generator reads, and the summary.  tests/adaptive_mirror.py restates every function here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rt_adaptive_plan {

constexpr int kTile = 16, kBlock = 8;

// tiles tx x ty over the whole image; the footprint fw x fh (what a frame writes); its 8 x 8 blocks, row-major, blocks_x per row
struct Shape { int width, height, tx, ty, fw, fh; uint32_t blocks_x, blocks_y; };
inline Shape shape(int width, int height)
{
    Shape s{};
    s.width = width; s.height = height;
    s.tx = (width + kTile - 1) / kTile; s.ty = (height + kTile - 1) / kTile;
    s.fw = width / kBlock * kBlock; s.fh = height / kBlock * kBlock;
    s.blocks_x = (uint32_t)(s.fw / kBlock); s.blocks_y = (uint32_t)(s.fh / kBlock);
    return s;
}

// the footprint pixels of tile t (0: the tile lies in the image's unwritten margin)
inline uint32_t tile_pixels(const Shape &s, uint32_t t)
{
    const int x0 = (int)(t % (uint32_t)s.tx) * kTile, y0 = (int)(t / (uint32_t)s.tx) * kTile;
    const int w = s.fw - x0 < kTile ? s.fw - x0 : kTile, h = s.fh - y0 < kTile ? s.fh - y0 : kTile;
    return w > 0 && h > 0 ? (uint32_t)(w * h) : 0u;
}

// the record of a tile as the device leaves it (rtgl_adaptive_tile)
struct Tile { float sum, mse; uint32_t count, converged, samples, samples_snapshot, reserved[2]; };

inline bool done(const Tile &r) { return r.count > 0u && r.converged != 0u; }      // valid and converged

// the mask rule
inline bool active(const Shape &s, uint32_t t, const Tile &r, uint32_t min_samples, uint32_t max_samples)
{
    if (!tile_pixels(s, t)) return false;
    return r.samples < min_samples || (r.samples < max_samples && !done(r));
}

// an explicit mask: non-zero = active, a tile without footprint pixels stays inactive
inline void explicit_mask(const Shape &s, const uint8_t *tiles, std::vector<uint8_t> &mask)
{
    const uint32_t n = (uint32_t)s.tx * (uint32_t)s.ty;
    mask.assign(n, 0);
    for (uint32_t t = 0; t < n; ++t) mask[t] = (tiles[t] != 0 && tile_pixels(s, t)) ? 1 : 0;
}

// the blocks of the footprint that lie in active tiles, ascending, and the active tiles, ascending
inline void build_lists(const Shape &s, const std::vector<uint8_t> &mask, std::vector<uint32_t> &blocks, std::vector<uint32_t> &tiles)
{
    blocks.clear(); tiles.clear();
    for (uint32_t by = 0; by < s.blocks_y; ++by)
        for (uint32_t bx = 0; bx < s.blocks_x; ++bx)
            if (mask[(size_t)(by / 2u) * (uint32_t)s.tx + bx / 2u]) blocks.push_back(by * s.blocks_x + bx);
    for (uint32_t t = 0; t < (uint32_t)mask.size(); ++t) if (mask[t]) tiles.push_back(t);
}

// rtgl_adaptive_summary
struct Summary {
    uint32_t tiles_total, tiles_active, tiles_converged, tiles_capped, blocks_active, samples_min, samples_max, converged;
    uint64_t samples_total;
    float max_tile_mse;
    uint32_t reserved[5];
};
static_assert(sizeof(Tile) == 32 && sizeof(Summary) == 64, "the layouts of include/rtgl_amd.h");

inline Summary summary(const Shape &s, const Tile *records, const std::vector<uint8_t> &mask, uint32_t n_blocks, uint32_t max_samples)
{
    Summary out{};
    bool first = true;
    for (uint32_t t = 0; t < (uint32_t)s.tx * (uint32_t)s.ty; ++t) {
        const uint32_t px = tile_pixels(s, t);
        if (!px) continue;
        const Tile &r = records[t];
        out.tiles_total++;
        if (mask[t]) out.tiles_active++;
        if (done(r)) out.tiles_converged++;
        else if (r.samples >= max_samples) out.tiles_capped++;
        if (first || r.samples < out.samples_min) out.samples_min = r.samples;
        if (first || r.samples > out.samples_max) out.samples_max = r.samples;
        first = false;
        out.samples_total += (uint64_t)r.samples * px;
        if (r.count > 0u && r.mse > out.max_tile_mse) out.max_tile_mse = r.mse;
    }
    out.blocks_active = n_blocks;
    out.converged = out.tiles_active == 0u ? 1u : 0u;
    return out;
}

}  // namespace rt_adaptive_plan
