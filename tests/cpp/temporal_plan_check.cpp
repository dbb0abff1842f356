// The host half of rtgl_temporal_accumulate and rtgl_temporal_clip (raytracer.glsl_amd/csrc/rt_temporal_plan.hpp) as a stand-alone
// program: the defaults, the planes, the history, the turn of the two sets and the grid; with the argument `replay`, the answers of the
// two calls to the records and states of standard input (tests/cpp/post_replay.hpp).  Built by its test with the address and
// undefined-behaviour sanitizers (tests/test_post_plans.py).
#include "../../raytracer.glsl_amd/csrc/rt_temporal_plan.hpp"
#include "post_replay.hpp"

using namespace rt_temporal_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static int replay()
{
    using post_replay::refuse;
    using post_replay::kState;
    bool tiled = false, restart = true, has_temporal = false;
    size_t px = 0;
    uint32_t aov = 0, aov_n = 0;
    int moments = 0;
    for (post_replay::Line line; post_replay::next(line);) {
        if (line.verb == "state") {
            const auto &n = line.n;
            tiled = n.at(0) != 0; px = (size_t)n.at(1); aov = (uint32_t)n.at(2); restart = n.at(3) != 0; aov_n = (uint32_t)n.at(4); moments = (int)n.at(5); has_temporal = n.at(6) != 0;
        } else if (line.verb == "rtgl_temporal_accumulate") {      // the order of rtgl_amd.hip: the record, the tiled refusal, the planes, the pixels
            const char *who = "rtgl_temporal_accumulate";
            Params p = default_params();
            post_replay::take(line, p);
            if (refuse(post_replay::kInvalid, who, invalid(p))) continue;
            if (tiled) { std::puts("tiled"); continue; }
            if (refuse(kState, who, planes_refused(planes_needed(p, moments), aov, restart, aov_n, false)) || refuse(kState, who, pixels_refused(px))) continue;
            std::puts("0");
        } else if (line.verb == "rtgl_temporal_clip") {            // ... the record, the tiled refusal, the history, the planes, the pixels
            const char *who = "rtgl_temporal_clip";
            ClipParams p = default_clip_params();
            post_replay::take(line, p);
            if (refuse(post_replay::kInvalid, who, invalid(p))) continue;
            if (tiled) { std::puts("tiled"); continue; }
            if (refuse(kState, who, clip_refused(has_temporal)) || refuse(kState, who, planes_refused(planes_needed(p), aov, restart, aov_n, true)) || refuse(kState, who, pixels_refused(px))) continue;
            std::puts("0");
        } else return 2;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "replay")) return replay();
    // defaults: the numbers of host.py's TEMPORAL_DEFAULTS and TEMPORAL_CLIP_DEFAULTS and of the header's text
    const Params p = default_params();
    CHECK(p.max_history == 32.0f && p.sigma_normal == 0.3f && p.sigma_position == 0.05f && p.flags == 0u && !invalid(p));
    for (uint32_t r : p.reserved) CHECK(r == 0u);
    const ClipParams c = default_clip_params();
    CHECK(c.sigma_scale == 2.0f && c.clip_history == 3.0f && c.sigma_normal == 0.3f && c.sigma_position == 0.05f && c.flags == 0u && !invalid(c));
    for (uint32_t r : c.reserved) CHECK(r == 0u);
    { Params q = p; q.max_history = 1.0f; CHECK(!invalid(q)); q.max_history = 0x1.fffffep-1f; CHECK(invalid(q)); }
    { ClipParams q = c; q.clip_history = 1.0f; CHECK(!invalid(q)); q.clip_history = 0x1.fffffep-1f; CHECK(invalid(q)); q = c; q.sigma_scale = 0.0f; CHECK(invalid(q)); }
    // the planes: position always, normal for its test, albedo for moments of the demodulated radiance
    CHECK(planes_needed(p, 0) == 6u && planes_needed(p, 1) == 6u && planes_needed(p, 2) == 7u && planes_needed(c) == 6u);
    { Params q = p; q.sigma_normal = 0.0f; CHECK(planes_needed(q, 0) == 4u); ClipParams d = c; d.sigma_normal = -1.0f; CHECK(planes_needed(d) == 4u); }
    CHECK(planes_refused(6, 4, false, 1, false) && planes_refused(6, 4, false, 1, true) && planes_refused(6, 4, false, 1, false) != planes_refused(6, 4, false, 1, true));
    CHECK(!planes_refused(6, 15, false, 1, false) && planes_refused(4, 4, true, 1, false) && planes_refused(4, 4, false, 0, true) && !planes_refused(4, 4, false, 1, true));
    CHECK(pixels_refused(0) && !pixels_refused(1) && clip_refused(false) && !clip_refused(true));
    // the history: a stored one, with a normal plane if the normal test is on
    CHECK(!history_usable(false, false, true) && history_usable(true, false, false) && !history_usable(true, true, false) && history_usable(true, true, true));
    // the turn: the first call writes the set it would read, every later one the other
    CHECK(turn(false, 0) == 0 && turn(false, 1) == 1 && turn(true, 0) == 1 && turn(true, 1) == 0);
    CHECK(grid_x(1) == 1 && grid_x(64) == 1 && grid_x(65) == 2 && grid_x(1920) == 30 && grid_y(1) == 1 && grid_y(4) == 1 && grid_y(5) == 2 && grid_y(1080) == 270);
    CHECK(pixels(1080, 1920) == 2073600u && pixels(0, 64) == 0u && record_bytes(3) == 48u);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("temporal_plan_check: ok\n");
    return 0;
}
