// The host half of rtgl_guides_frame (raytracer.glsl_amd/csrc/rt_guides_plan.hpp) as a stand-alone program: the refusals and their order,
// the count of the planes' mean, the intersect stage per (option "kernel", triangle visits), the launches and what the pass writes.
// Built by its test with the address and undefined-behaviour sanitizers (tests/test_guides_abi.py).
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "../../raytracer.glsl_amd/csrc/rt_guides_plan.hpp"

using namespace rt_guides_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main()
{
    // refusals: NULL context, multi-device handle, no frame parameters, no plane -- the first that applies
    CHECK(refused(true, false, true, 1u).code == kOk && refused(true, false, true, 1u).why == nullptr);
    for (uint32_t aov : {1u, 2u, 4u, 8u, 15u, 5u}) CHECK(!refused(true, false, true, aov).why);
    for (int multi = 0; multi < 2; ++multi) for (int params = 0; params < 2; ++params) for (uint32_t aov : {0u, 15u}) {
        const Refusal r = refused(false, multi != 0, params != 0, aov);
        CHECK(r.code == kErrInvalid && r.why && std::strlen(r.why) > 0);
    }
    for (int params = 0; params < 2; ++params) for (uint32_t aov : {0u, 15u}) {
        const Refusal r = refused(true, true, params != 0, aov);
        CHECK(r.code == kErrState && r.why && std::strstr(r.why, "multi-device"));
    }
    for (uint32_t aov : {0u, 15u}) {
        const Refusal r = refused(true, false, false, aov);
        CHECK(r.code == kErrState && r.why && std::strstr(r.why, "rtgl_set_frame_params"));
    }
    { const Refusal r = refused(true, false, true, 0u); CHECK(r.code == kErrState && r.why && std::strstr(r.why, "\"aov\"")); }
    CHECK(kOk == 0 && kErrInvalid == -1 && kErrState == -4);

    // the count: a pending restart -> 1, otherwise + 1; the restart is consumed; a frame's reset flag restarts as well
    {
        Count c{0u, true};                                   // as setting "aov" leaves it
        c = after_pass(c); CHECK(c.n == 1u && !c.restart);
        c = after_pass(c); CHECK(c.n == 2u && !c.restart);
        c = after_frame(c, false); CHECK(c.n == 3u && !c.restart);      // a later frame continues the same n
        c = after_pass(c); CHECK(c.n == 4u);
        c = after_restart(c); CHECK(c.n == 4u && c.restart);            // the contents stay, a refused call in between moves nothing
        c = after_pass(c); CHECK(c.n == 1u && !c.restart);
        c = after_frame(c, true); CHECK(c.n == 1u && !c.restart);
        c = after_pass(c); CHECK(c.n == 2u);
        c = after_restart(after_restart(c)); c = after_frame(c, false); CHECK(c.n == 1u && !c.restart);
        Count big{0xFFFFFFFEu, false}; big = after_pass(big); CHECK(big.n == 0xFFFFFFFFu);
        for (uint32_t n : {0u, 1u, 9u}) { CHECK(after_pass({n, true}).n == 1u && after_frame({n, true}, false).n == 1u && after_frame({n, false}, true).n == 1u); }
    }

    // the stage: none without triangle visits; kernel 2's for option 2; kernel 4's for 0, 1 and 4
    for (int k : {0, 1, 2, 4}) CHECK(stage(k, 0u) == kStageNone && !generates_rays(stage(k, 0u)));
    for (uint32_t t : {1u, 200u, 0xFFFFFFFFu}) {
        CHECK(stage(0, t) == kStageSolo && stage(1, t) == kStageSolo && stage(4, t) == kStageSolo && stage(2, t) == kStageSplit);
        for (int k : {0, 1, 2, 4}) CHECK(generates_rays(stage(k, t)));
    }
    CHECK(stage_kernel(kStageSolo, 0) == 4 && stage_kernel(kStageSolo, 1) == 4 && stage_kernel(kStageSolo, 4) == 4 && stage_kernel(kStageSplit, 2) == 2);
    for (int k : {0, 1, 2, 4}) CHECK(stage_kernel(kStageNone, k) == k);
    CHECK(kKernelSplit == 2 && kKernelSolo == 4);

    // launches
    CHECK(blocks(0u) == 0u && blocks(1u) == 1u && blocks(64u) == 1u && blocks(256u) == 1u && blocks(257u) == 2u && blocks(1920u * 1080u) == 8100u);
    CHECK(blocks(0xFFFFFFF0u) == 0x1000000u);               // no 32-bit wrap in the round-up
    CHECK(wave_bounces() == 1u);
    CHECK(!enqueues(0u) && enqueues(64u) && enqueues(0xFFFFFFF0u));

    // what the pass writes: the planes, their count, the frame timer, and the scratch every frame rewrites -- nothing else
    int written = 0;
    for (int t = 0; t < (int)kTargets; ++t) written += writes((Target)t) ? 1 : 0;
    CHECK(written == 4 && writes(kPlanes) && writes(kPlanesCount) && writes(kFrameTimer) && writes(kWaveBuffers));
    for (Target t : {kImage, kSampleBuffers, kBucketBuffers, kRngStates, kCounters, kDenoised, kTemporal, kDisplay, kErrorSnapshot, kSessions, kRayEstimates, kKeptCameraBits})
        CHECK(!writes(t));
    CHECK(!takes_kept_bits() && !drops_kept_bits());

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("guides_plan_check: ok\n");
    return 0;
}
