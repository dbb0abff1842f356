// The host half of rtgl_denoise and rtgl_denoise_guided (raytracer.glsl_amd/csrc/rt_denoise_plan.hpp) as a stand-alone program: the
// defaults, the planes, the geometry of every pass and the scratch buffers; with the argument `replay`, the answers of the two calls to the
// records and states of standard input (tests/cpp/post_replay.hpp).  Built by its test with the address and undefined-behaviour
// sanitizers (tests/test_post_plans.py).
#include <vector>
#include "../../raytracer.glsl_amd/csrc/rt_bucket_guide_plan.hpp"
#include "../../raytracer.glsl_amd/csrc/rt_denoise_plan.hpp"
#include "post_replay.hpp"

using namespace rt_denoise_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the order of rtgl_amd.hip: the record, the tiled refusal, the planes, the input, the temporal variance
struct State { bool tiled, restart, has_temporal; size_t px; uint32_t aov, aov_n; int source, variance, stored; };
static void answer(const State &s, const char *who, const char *bad, uint32_t need, bool guided, bool demod)
{
    using post_replay::refuse;
    if (refuse(post_replay::kInvalid, who, bad)) return;
    if (s.tiled) { std::puts("tiled"); return; }
    if (refuse(post_replay::kState, who, rt_bucket_guide_plan::planes_refused(need, s.aov, s.restart, s.aov_n))) return;
    if (refuse(post_replay::kState, who, input_refused(s.px, s.source, s.has_temporal))) return;
    if (guided && refuse(post_replay::kState, who, guided_variance_refused(s.variance, s.source, s.stored, demod))) return;
    std::puts("0");
}

static int replay()
{
    State s{};
    for (post_replay::Line line; post_replay::next(line);) {
        if (line.verb == "state") {
            const auto &n = line.n;
            s = State{n.at(0) != 0, n.at(3) != 0, n.at(8) != 0, (size_t)n.at(1), (uint32_t)n.at(2), (uint32_t)n.at(4), (int)n.at(5), (int)n.at(6), (int)n.at(7)};
        } else if (line.verb == "rtgl_denoise") {
            Params p = default_params();
            post_replay::take(line, p);
            answer(s, "rtgl_denoise", invalid(p), planes_needed(p), false, false);
        } else if (line.verb == "rtgl_denoise_guided") {
            GuidedParams p = default_guided_params();
            post_replay::take(line, p);
            answer(s, "rtgl_denoise_guided", invalid(p), planes_needed(p), true, (p.flags & kFlagDemodulate) != 0);
        } else return 2;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "replay")) return replay();
    // defaults: the numbers of host.py's DENOISE_DEFAULTS and DENOISE_GUIDED_DEFAULTS and of the header's text
    {
        const Params p = default_params();
        CHECK(p.passes == 5u && p.sigma_color == 16.0f && p.sigma_normal == 0.3f && p.sigma_position == 0.05f && p.flags == 1u && !invalid(p));
        for (uint32_t r : p.reserved) CHECK(r == 0u);
        const GuidedParams g = default_guided_params();
        CHECK(g.passes == 5u && g.sigma_lum == 4.0f && g.sigma_normal == 0.3f && g.sigma_position == 0.05f && g.firefly_ratio == 1.0f && g.flags == 1u && !invalid(g));
        for (uint32_t r : g.reserved) CHECK(r == 0u);
        CHECK(planes_needed(p) == 7u && planes_needed(g) == 7u);
        Params q = p; q.flags = 0; q.sigma_normal = 0.0f; CHECK(planes_needed(q) == kPlanePosition);
        q.sigma_position = -1.0f; CHECK(planes_needed(q) == 0u);
        q.passes = 8; CHECK(!invalid(q)); q.passes = 9; CHECK(invalid(q));
        GuidedParams h = g; h.passes = 8; CHECK(!invalid(h)); h.passes = 9; CHECK(invalid(h));
        h = g; h.sigma_lum = 1e-45f; CHECK(!invalid(h)); h.sigma_lum = 0.0f; CHECK(invalid(h));
    }
    // a pass: LDS below 64 KB, the wide form exactly above 256 columns, and every row of the picture in exactly one block's four
    for (uint32_t k = 0; k < kMaxPasses; ++k)
        for (int width : {1, 63, 64, 65, 1080, 1920})
            for (int height : {1, 3, 4, 5, 63, 64, 65, 1080}) {
                const Pass g = pass(k, width, height);
                const int s = 1 << k;
                CHECK(g.tile_w == 64u + 4u * (uint32_t)s && g.wide == (g.tile_w > 256u) && g.wide == (k >= 6u));
                CHECK(lds_bytes(g, kAtrousArrays) == 2u * 9u * g.tile_w * 4u && lds_bytes(g, kGuidedArrays) == 2u * 10u * g.tile_w * 4u);
                CHECK(lds_bytes(g, kGuidedArrays) < 65536u);
                CHECK(g.grid_x * 64u >= (uint32_t)width && (g.grid_x - 1u) * 64u < (uint32_t)width);
                std::vector<int> seen((size_t)height, 0);
                for (uint32_t b = 0; b < g.grid_y; ++b)                     // the rows of block b, as the kernels place them
                    for (int j = 0; j < 4; ++j) {
                        const int y = 4 * s * (int)(b >> k) + (int)(b & (uint32_t)(s - 1)) + j * s;
                        if (y < height) ++seen[(size_t)y];
                    }
                for (int v : seen) CHECK(v == 1);
                CHECK(g.grid_y % (uint32_t)s == 0u && (g.grid_y / (uint32_t)s - 1u) * 4u * (uint32_t)s < (uint32_t)height);      // no chunk of blocks past the picture
            }
    // the prepare and the identity kernels, the buffers
    CHECK(prepare_grid_x(1) == 1 && prepare_grid_x(64) == 1 && prepare_grid_x(65) == 2 && prepare_grid_y(1) == 1 && prepare_grid_y(4) == 1 && prepare_grid_y(5) == 2 && prepare_grid_y(1080) == 270);
    CHECK(identity_blocks(1) == 1 && identity_blocks(256) == 1 && identity_blocks(257) == 2 && kPrepLdsBytes == 37360u && kPrepLdsBytes < 65536u);
    CHECK(pixels(1080, 1920) == 2073600u && pixels(0, 32) == 0u && record_bytes(10) == 160u && near_bytes(10) == 40u);
    for (uint32_t passes = 0; passes <= kMaxPasses; ++passes) {
        uint32_t atrous = 0, guided = 0;                                    // the scratch buffers the passes of rtgl_amd.hip write or read
        for (uint32_t k = 0; k + 1u < passes; ++k) atrous |= 1u << (k & 1u);
        for (uint32_t k = 0; k < passes; ++k) guided |= 1u << (k & 1u);
        CHECK((1u << scratch_buffers(passes)) - 1u == atrous && (1u << guided_scratch_buffers(passes)) - 1u == guided);
    }
    // the temporal variance: off, or the history's moments of the call's kind
    CHECK(!guided_variance_refused(0, 0, 0, true) && guided_variance_refused(1, 0, 2, true) && guided_variance_refused(1, 1, 0, true));
    CHECK(guided_variance_refused(1, 1, 1, true) && !guided_variance_refused(1, 1, 2, true) && guided_variance_refused(1, 1, 2, false) && !guided_variance_refused(1, 1, 1, false));
    CHECK(input_refused(0, 0, true) && !input_refused(1, 0, false) && input_refused(1, 1, false) && !input_refused(1, 1, true));
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("denoise_plan_check: ok\n");
    return 0;
}
