// facade_null_check.cpp -- a Renderer that got no context (no device, or a device index that does not exist: the constructor prints and
// carries on, as the reference does): every post-process method of include/rtgl/renderer.h then returns false / empty / -1 / 0 frames /
// a zeroed summary and touches nothing.  Stand-alone; tests/test_facade_post.py builds it with the address and undefined-behaviour
// sanitizers on the executable and runs it.  Exit code: 0, or the number of the first check that failed, from 10.
#include <cstdio>
#include <cstring>
#include <string>

#include "rtgl/renderer.h"

#define REQUIRE(cond)                                                                                                   \
    do {                                                                                                                \
        const int id_ = __COUNTER__;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "facade_null_check: check %d failed (line %d): %s\n", id_, __LINE__, #cond); return 10 + id_; } \
    } while (0)

template <typename T> static bool all_zero(const T &v)
{
    const T zero{};
    return std::memcmp(&v, &zero, sizeof v) == 0;
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    Renderer r(70, 53, 1 << 20);                                         // no such device anywhere
    REQUIRE(r.context() == nullptr);
    srand(12345);
    std::vector<rtgl_frame_params> log;
    r.set_frame_params_log(&log);
    r.set_spheres({Sphere({0.0f, 0.0f, 0.0f}, 1.0f, 0)});
    r.set_materials({Material(gfx::rgb(0xAAAAAA))});
    r.set_frame_budget(3);
    r.run();                                                             // render() returns at once: no frame, no rand()
    REQUIRE(log.empty());
    REQUIRE(r.read_image().empty());

    r.set_aov(RTGL_AOV_ALL);
    REQUIRE(r.read_aov(RTGL_AOV_NORMAL).empty());
    REQUIRE(r.read_aov<int32_t>(RTGL_AOV_IDS).empty());
    REQUIRE(r.read_aov<float>(RTGL_AOV_IDS).empty());
    REQUIRE(!r.save_aov_pfm(RTGL_AOV_ALBEDO, dir + "/albedo.pfm"));
    REQUIRE(!r.save_aov_pfm(RTGL_AOV_IDS, dir + "/ids.pfm"));

    rtgl_denoise_params dp{};
    rtgl_denoise_guided_params gp{};
    REQUIRE(!r.denoise());
    REQUIRE(!r.denoise(&dp));
    REQUIRE(!r.denoise_guided());
    REQUIRE(!r.denoise_guided(&gp));
    REQUIRE(r.read_denoise_variance().empty());
    REQUIRE(r.read_denoised().empty());
    REQUIRE(!r.save_denoised_pfm(dir + "/denoised.pfm"));

    rtgl_temporal_params tp{};
    rtgl_temporal_clip_params cp{};
    REQUIRE(!r.temporal_accumulate());
    REQUIRE(!r.temporal_accumulate(&tp));
    REQUIRE(!r.temporal_clip());
    REQUIRE(!r.temporal_clip(&cp));
    REQUIRE(!r.temporal_reset());
    REQUIRE(r.read_temporal().empty());
    REQUIRE(r.read_temporal_moments().empty());

    rtgl_tonemap_params mp{};
    REQUIRE(!r.tonemap());
    REQUIRE(!r.tonemap(&mp));
    REQUIRE(r.read_display().empty());
    REQUIRE(r.read_display(true).empty());
    REQUIRE(!r.save_display_png(dir + "/display.png"));

    rtgl_error_params ep{};
    rtgl_error_summary es;
    std::memset(&es, 0xff, sizeof es);
    REQUIRE(!r.error_estimate());
    REQUIRE(!r.error_estimate(&ep));
    REQUIRE(all_zero(r.read_error_summary()));
    REQUIRE(r.render_until(0.05f, 11, 4, nullptr, &es) == 0);
    REQUIRE(all_zero(es));
    REQUIRE(r.render_until(0.05f, 11, 4, &ep) == 0);
    REQUIRE(r.render_until(0.05f, 11, 0) == 0);

    rtgl_adaptive_params ap{};
    rtgl_adaptive_summary as;
    std::memset(&as, 0xff, sizeof as);
    REQUIRE(!r.adaptive_begin());
    REQUIRE(!r.adaptive_begin(&ap));
    REQUIRE(!r.adaptive_frame());
    REQUIRE(!r.adaptive_update());
    REQUIRE(!r.adaptive_update(&as));
    REQUIRE(!r.adaptive_set_mask(std::vector<uint8_t>(5 * 4, 1)));
    REQUIRE(!r.adaptive_set_mask({}));
    REQUIRE(r.adaptive_get_mask().empty());
    REQUIRE(r.read_adaptive_tiles().empty());
    std::memset(&as, 0xff, sizeof as);
    REQUIRE(r.render_adaptive(0.05f, 64, 16, 16, &as) == 0);
    REQUIRE(all_zero(as));
    REQUIRE(r.render_adaptive(0.05f, 64) == 0);

    rtgl_robust_params rp{};
    rtgl_robust_resolve_params rr{};
    REQUIRE(!r.robust_begin());
    REQUIRE(!r.robust_begin(&rp));
    REQUIRE(!r.robust_accumulate());
    REQUIRE(!r.robust_frame());
    REQUIRE(!r.robust_resolve());
    REQUIRE(!r.robust_resolve(&rr));
    REQUIRE(!r.robust_end());
    REQUIRE(r.robust_frames() == -1);
    REQUIRE(r.read_robust().empty());
    REQUIRE(r.read_robust_bucket(0).empty());
    REQUIRE(r.render_robust(9, 4, 2.0f, false) == 0);
    REQUIRE(r.render_robust(9) == 0);

    REQUIRE(log.empty());                                                // nothing was a frame, nothing drew from rand()
    REQUIRE(all_zero(r.last_frame_params()));
    const int next = rand();
    srand(12345);
    REQUIRE(next == rand());                                             // (still the stream's first word)
    std::printf("facade_null_check: %d checks passed\n", __COUNTER__);
    return 0;
}
