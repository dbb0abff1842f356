// The host half of rtgl_tonemap (raytracer.glsl_amd/csrc/rt_tonemap_plan.hpp) as a stand-alone program: the defaults, the record's
// bounds, the blocks, the state words and the turn of the two histogram sets; with the argument `replay`, the call's answers to the
// records and states of standard input (tests/cpp/post_replay.hpp).  Built by its test with the address and undefined-behaviour
// sanitizers (tests/test_post_plans.py).
#include "../../raytracer.glsl_amd/csrc/rt_tonemap_plan.hpp"
#include "post_replay.hpp"

using namespace rt_tonemap_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static int replay()
{
    using post_replay::refuse;
    const char *who = "rtgl_tonemap";
    bool tiled = false, has_denoised = false, has_temporal = false;
    size_t px = 0;
    for (post_replay::Line line; post_replay::next(line);) {
        if (line.verb == "state") { tiled = line.n.at(0) != 0; px = (size_t)line.n.at(1); has_denoised = line.n.at(2) != 0; has_temporal = line.n.at(3) != 0; continue; }
        if (line.verb != who) return 2;
        Params p = default_params();      // the order of rtgl_amd.hip: the record, the tiled refusal, the source, the pixels
        post_replay::take(line, p);
        if (refuse(post_replay::kInvalid, who, invalid(p))) continue;
        if (tiled) { std::puts("tiled"); continue; }
        if (refuse(post_replay::kState, who, source_refused(p.source, has_denoised, has_temporal)) || refuse(post_replay::kState, who, pixels_refused(px))) continue;
        std::puts("0");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "replay")) return replay();
    // defaults: the numbers of host.py's TONEMAP_DEFAULTS and of the header's text
    const Params d = default_params();
    CHECK(d.source == 0u && d.op == 1u && d.flags == 1u && d.exposure == 1.0f && d.key == 0.18f && d.white == 4.0f && d.adapt == 1.0f);
    CHECK(d.exposure_min == 1.0f / 65536.0f && d.exposure_max == 65536.0f && d.low_permille == 100u && d.high_permille == 20u && !invalid(d) && automatic(d));
    for (uint32_t r : d.reserved) CHECK(r == 0u);
    // the bounds, from both sides
    { Params p = d; p.adapt = 1.0f; CHECK(!invalid(p)); p.adapt = 0x1.000002p0f; CHECK(invalid(p)); p.adapt = 1e-45f; CHECK(!invalid(p)); p.adapt = 0.0f; CHECK(invalid(p)); }
    { Params p = d; p.exposure_min = p.exposure_max = 2.0f; CHECK(!invalid(p)); p.exposure_min = 0x1.000002p1f; CHECK(invalid(p)); }
    for (uint32_t low : {0u, 1u, 499u, 500u, 999u, 1000u, 0xFFFFFFFFu})
        for (uint32_t high : {0u, 1u, 499u, 500u, 999u, 1000u, 0xFFFFFFFFu}) {
            Params p = d; p.low_permille = low; p.high_permille = high;
            CHECK(!invalid(p) == ((uint64_t)low + high < 1000u));
        }
    { Params p = d; p.source = 2; CHECK(!invalid(p)); p.source = 3; CHECK(invalid(p)); p = d; p.op = 2; CHECK(!invalid(p)); p.op = 3; CHECK(invalid(p)); }
    { Params p = d; p.flags = 0; CHECK(!invalid(p) && !automatic(p)); p.flags = 2; CHECK(invalid(p)); }
    CHECK(!source_refused(0, false, false) && source_refused(1, false, true) && !source_refused(1, true, false) && source_refused(2, true, false) && !source_refused(2, false, true));
    CHECK(pixels_refused(0) && !pixels_refused(1));
    // a block per 256 pixels, eight per compute unit at the most
    CHECK(blocks(1, 256) == 1 && blocks(256, 256) == 1 && blocks(257, 256) == 2 && blocks(2073600, 256) == 2048 && blocks(2073600, 2000) == 8100 && blocks(1024, 1) == 4);
    CHECK(display_bytes(10) == 40u && kSetWords == 257 && kExposureWord == 514 && kStateWords == 516);
    // the sets: a call counts in the set the call before cleared, and the histogram read is of the latest
    Sets s;
    CHECK(s.set == 0 && s.hist_set == -1 && !s.prev);
    s.after_auto_call(); CHECK(s.set == 1 && s.hist_set == 0 && s.prev);
    s.prev = false;
    s.after_auto_call(); CHECK(s.set == 0 && s.hist_set == 1 && s.prev);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("tonemap_plan_check: ok\n");
    return 0;
}
