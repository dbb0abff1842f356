// facade_robust_until.cpp -- Renderer::render_robust_until(), robust_error_estimate() and read_robust_error_summary() of
// include/rtgl/renderer.h driven on facade_demo's spheres (the light, the mirror and the glass: a scene with fireflies, no mesh, no cube
// map).  Used by tests/test_gpu_robust_error.py: one Renderer after srand(0), the uniforms of every frame logged, and what the methods
// return dumped raw, so that the test can run host.HeadlessRenderer, the Python twin, and the numpy mirror over the same inputs.  A
// check that fails ends the program with the check's number (from 10) and its text on stderr.
//   facade_robust_until <dir> <width> <height>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "rtgl/renderer.h"

#define REQUIRE(cond)                                                                                                   \
    do {                                                                                                                \
        const int id_ = __COUNTER__;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "facade_robust_until: check %d failed (line %d): %s\n", id_, __LINE__, #cond); return 10 + id_; } \
    } while (0)

static bool dump(const std::string &path, const void *data, size_t bytes)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(data, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}
template <typename T> static bool dump(const std::string &path, const std::vector<T> &v) { return !v.empty() && dump(path, v.data(), v.size() * sizeof(T)); }

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: facade_robust_until <dir> <width> <height>\n"); return 2; }
    const std::string dir = argv[1];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    const float room = 16.0f, sr = 4.0f, big = 10000;
    const std::vector<Sphere> spheres = {
        Sphere({0.0f, -(room + big), 0.0f}, big, 0),
        Sphere({3.0f, room + 10.0f, 0.0f}, 3.0f, 1),
        Sphere({-18.0f, -room + sr, 0.0f}, sr, 4),
        Sphere({-6.0f, -room + sr, 0.0f}, sr, 5),
        Sphere({+18.0f, -room + sr, 0.0f}, sr, 7),
    };
    const std::vector<Material> materials = {
        Material(gfx::rgb(0xAAAAAA)),
        Material(gfx::rgb(0xFFFFFF), gfx::rgb(0xFFFEFA) * 30.0f),
        Material(gfx::rgb(0xBC0000)),
        Material(gfx::rgb(0x00BC00)),
        Material(gfx::rgb(0xAAAAAA), gfx::rgb(0x0), 1.0f, MaterialType::SPECULAR),
        Material(gfx::rgb(0xFFFFFF), gfx::rgb(0x0), 0.0f, MaterialType::TRANSMISSIVE),
        Material(gfx::rgb(0xFF5733), gfx::rgb(0x0), 0.0f, MaterialType::TRANSMISSIVE),
        Material(gfx::rgb(0xAAAAAA), gfx::rgb(0x0), 0.5f, MaterialType::SPECULAR),
    };
    {
        KdTree<Sphere, 1, 2> tree(spheres);
        REQUIRE(dump(dir + "/materials.raw", materials) && dump(dir + "/nodes.raw", tree.nodes()) && dump(dir + "/spheres.raw", tree.primitives()));
    }
    // The device runtime reseeds rand() when the process's first context brings it up (tests/cpp/facade_post.cpp), so a Renderer that
    // renders nothing comes first: from here on srand(0) is followed by the words of the frames only.
    { Renderer first(8, 8); REQUIRE(first.context() != nullptr); }
    srand(0);
    Renderer r(w, h);
    REQUIRE(r.context() != nullptr);
    std::vector<rtgl_frame_params> log;
    r.set_frame_params_log(&log);
    r.set_materials(materials);
    r.set_kdtree(spheres);
    r.set_bounces(4);
    // before a session, and in a session with fewer frames than buckets: refused, and the summary stays unreadable
    REQUIRE(!r.robust_error_estimate());
    REQUIRE(r.robust_begin() && r.robust_frame() && !r.robust_error_estimate());
    REQUIRE(r.read_robust_error_summary().valid == 0);
    // one ordinary frame and a pending reset: a session frame sends frames 0 and reset_flag 1 whatever they are, and leaves both alone
    r.set_frame_budget(1);
    r.run();
    r.reset_buffer();
    rtgl_error_summary first{}, second{};
    const long a = r.render_robust_until(0.35f, 40, 6, 4, 1.0f, false, nullptr, &first);
    const long frames_a = r.robust_frames();
    REQUIRE(dump(dir + "/picture_first.raw", r.read_robust()));
    // by hand, on the open session: another gain and quantile
    rtgl_robust_error_params p;
    REQUIRE(rtgl_robust_error_defaults(&p) == RTGL_OK);
    p.gain = 0.0f; p.quantile_permille = 500u; p.threshold = 0.2f;
    REQUIRE(r.robust_error_estimate(&p));
    const rtgl_error_summary hand = r.read_robust_error_summary();
    for (uint32_t j = 0; j < 4; ++j) REQUIRE(dump(dir + "/bucket" + std::to_string(j) + ".raw", r.read_robust_bucket(j)));
    // a threshold no picture meets: max_frames ends it; the picture goes to the image
    const long b = r.render_robust_until(1e-6f, 21, 8, 8, 0.5f, true, &p, &second);
    const long frames_b = r.robust_frames();
    REQUIRE(dump(dir + "/picture_second.raw", r.read_image()));
    r.set_frame_budget(2);
    r.run();
    REQUIRE(dump(dir + "/final_image.raw", r.read_image()));
    REQUIRE(r.robust_end() && !r.robust_error_estimate() && r.read_robust_error_summary().valid == 0);
    const int64_t values[5] = {a, frames_a, b, frames_b, (int64_t)log.size()};
    const rtgl_error_summary summaries[3] = {first, hand, second};
    REQUIRE(dump(dir + "/returns.raw", values, sizeof values) && dump(dir + "/summaries.raw", summaries, sizeof summaries) && dump(dir + "/params.raw", log));
    std::printf("facade_robust_until: ok\n");
    return 0;
}
