// facade_robust_denoise.cpp -- Renderer::robust_denoise() of include/rtgl/renderer.h driven on facade_demo's spheres (the light, the mirror
// and the glass: a scene with fireflies, no mesh, no cube map).  Used by tests/test_gpu_robust_denoise.py: one Renderer after srand(0),
// the uniforms of every frame logged, and the buckets, the first-hit planes and what the call leaves dumped raw, so that the test can run
// host.HeadlessRenderer, the Python twin, and the numpy mirror over the same inputs.  A check that fails ends the program with the
// check's number (from 10) and its text on stderr.
//   facade_robust_denoise <dir> <width> <height>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "rtgl/renderer.h"

#define REQUIRE(cond)                                                                                                   \
    do {                                                                                                                \
        const int id_ = __COUNTER__;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "facade_robust_denoise: check %d failed (line %d): %s\n", id_, __LINE__, #cond); return 10 + id_; } \
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
    if (argc != 4) { std::fprintf(stderr, "usage: facade_robust_denoise <dir> <width> <height>\n"); return 2; }
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
    REQUIRE(rtgl_set_option(r.context(), "aov", RTGL_AOV_ALBEDO | RTGL_AOV_NORMAL | RTGL_AOV_POSITION) == RTGL_OK);
    // before a session: refused
    REQUIRE(!r.robust_denoise());
    REQUIRE(r.render_robust(16, 8) == 16 && r.robust_frames() == 16);
    REQUIRE(r.robust_denoise());
    REQUIRE(dump(dir + "/denoised_default.raw", r.read_denoised()) && dump(dir + "/variance_default.raw", r.read_denoise_variance()));
    rtgl_robust_denoise_params p;
    REQUIRE(rtgl_robust_denoise_defaults(&p) == RTGL_OK);
    p.passes = 2u; p.flags = 0u; p.gain = 0.5f; p.sigma_lum = 2.0f;
    REQUIRE(r.robust_denoise(&p));
    REQUIRE(dump(dir + "/denoised_hand.raw", r.read_denoised()) && dump(dir + "/variance_hand.raw", r.read_denoise_variance()));
    p.passes = 9u;
    REQUIRE(!r.robust_denoise(&p));
    for (uint32_t j = 0; j < 8; ++j) REQUIRE(dump(dir + "/bucket" + std::to_string(j) + ".raw", r.read_robust_bucket(j)));
    std::vector<float> plane((size_t)w * h * 4);
    REQUIRE(rtgl_read_aov(r.context(), RTGL_AOV_ALBEDO, plane.data()) == RTGL_OK && dump(dir + "/albedo.raw", plane));
    REQUIRE(rtgl_read_aov(r.context(), RTGL_AOV_NORMAL, plane.data()) == RTGL_OK && dump(dir + "/normal.raw", plane));
    REQUIRE(rtgl_read_aov(r.context(), RTGL_AOV_POSITION, plane.data()) == RTGL_OK && dump(dir + "/position.raw", plane));
    REQUIRE(r.robust_end() && !r.robust_denoise());
    REQUIRE(dump(dir + "/params.raw", log));
    std::printf("facade_robust_denoise: ok\n");
    return 0;
}
