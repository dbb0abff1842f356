// facade_robust_adaptive.cpp -- Renderer::render_robust_adaptive() and the robust_adaptive_*() methods of include/rtgl/renderer.h driven on
// facade_demo's spheres (the light, the mirror and the glass: a scene with fireflies, no mesh, no cube map).  Used by
// tests/test_gpu_robust_adaptive.py: one Renderer after srand(0), the uniforms of every frame logged, and what the methods return dumped
// raw, so that the test can run host.HeadlessRenderer, the Python twin, and the numpy mirror over the same inputs.  A check that fails ends
// the program with the check's number (from 10) and its text on stderr.
//   facade_robust_adaptive <dir> <width> <height>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "rtgl/renderer.h"

#define REQUIRE(cond)                                                                                                   \
    do {                                                                                                                \
        const int id_ = __COUNTER__;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "facade_robust_adaptive: check %d failed (line %d): %s\n", id_, __LINE__, #cond); return 10 + id_; } \
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
    if (argc != 4) { std::fprintf(stderr, "usage: facade_robust_adaptive <dir> <width> <height>\n"); return 2; }
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
    // without a session every method refuses (robust_adaptive_frame() too, at the end: a refused frame has drawn its random word)
    REQUIRE(!r.robust_adaptive_accumulate() && !r.robust_adaptive_update() && !r.robust_adaptive_resolve() && !r.robust_adaptive_end());
    REQUIRE(r.robust_adaptive_get_mask().empty() && r.read_robust_adaptive().empty() && r.read_robust_adaptive_tiles().empty());
    // one ordinary frame and a pending reset: a session frame leaves both alone
    r.set_frame_budget(1);
    r.run();
    r.reset_buffer();
    rtgl_adaptive_summary first{}, hand{}, second{};
    const long a = r.render_robust_adaptive(0.35f, 48, 8, 6, 4, 1.0f, false, &first);
    REQUIRE(dump(dir + "/picture_first.raw", r.read_robust_adaptive()) && dump(dir + "/tiles_first.raw", r.read_robust_adaptive_tiles()));
    for (uint32_t j = 0; j < 4; ++j) REQUIRE(dump(dir + "/bucket" + std::to_string(j) + ".raw", r.read_robust_adaptive_bucket(j)));
    // by hand, on the open session: a mask of the first tile alone, one frame, an update
    std::vector<uint8_t> mask = r.robust_adaptive_get_mask();
    REQUIRE(!mask.empty());
    for (size_t t = 0; t < mask.size(); ++t) mask[t] = t == 0;
    REQUIRE(r.robust_adaptive_set_mask(mask) && r.robust_adaptive_get_mask() == mask);
    REQUIRE(r.robust_adaptive_frame() && r.robust_adaptive_update(&hand));
    REQUIRE(dump(dir + "/tiles_hand.raw", r.read_robust_adaptive_tiles()));
    // a threshold no picture meets: max_samples ends it; the picture goes to the image
    const long b = r.render_robust_adaptive(1e-6f, 11, 8, 4, 8, 0.5f, true, &second);
    REQUIRE(dump(dir + "/picture_second.raw", r.read_image()));
    r.set_frame_budget(2);
    r.run();
    REQUIRE(dump(dir + "/final_image.raw", r.read_image()));
    REQUIRE(r.robust_adaptive_end() && !r.robust_adaptive_update() && !r.robust_adaptive_frame());
    const int64_t values[3] = {a, b, (int64_t)log.size()};
    const rtgl_adaptive_summary summaries[3] = {first, hand, second};
    REQUIRE(dump(dir + "/returns.raw", values, sizeof values) && dump(dir + "/summaries.raw", summaries, sizeof summaries) && dump(dir + "/params.raw", log));
    std::printf("facade_robust_adaptive: ok\n");
    return 0;
}
