// facade_guides.cpp -- Renderer::render_guides() of include/rtgl/renderer.h driven on facade_demo's spheres.  Used by
// tests/test_gpu_guides.py: one Renderer after srand(0), the uniforms of every pass logged, and the scene, the four first-hit planes and
// the image dumped raw, so that the test can make the same passes through the C ABI and compare.  A check that fails ends the program
// with the check's number (from 10) and its text on stderr.
//   facade_guides <dir> <width> <height>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "rtgl/renderer.h"

#define REQUIRE(cond)                                                                                                   \
    do {                                                                                                                \
        const int id_ = __COUNTER__;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "facade_guides: check %d failed (line %d): %s\n", id_, __LINE__, #cond); return 10 + id_; } \
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
    if (argc != 4) { std::fprintf(stderr, "usage: facade_guides <dir> <width> <height>\n"); return 2; }
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
    // renders nothing comes first: from here on srand(0) is followed by the words of the passes only.
    { Renderer first(8, 8); REQUIRE(first.context() != nullptr); }
    srand(0);
    Renderer r(w, h);
    REQUIRE(r.context() != nullptr);
    std::vector<rtgl_frame_params> log;
    r.set_frame_params_log(&log);
    r.set_materials(materials);
    r.set_kdtree(spheres);
    r.set_bounces(4);
    // without a plane: refused, nothing logged
    REQUIRE(!r.guides_frame() && r.render_guides(2) == 0 && log.empty());
    r.set_aov(RTGL_AOV_ALL);
    REQUIRE(r.render_guides(3) == 3 && log.size() == 3);
    REQUIRE(dump(dir + "/albedo.raw", r.read_aov(RTGL_AOV_ALBEDO)) && dump(dir + "/normal.raw", r.read_aov(RTGL_AOV_NORMAL))
            && dump(dir + "/position.raw", r.read_aov(RTGL_AOV_POSITION)) && dump(dir + "/ids.raw", r.read_aov<int32_t>(RTGL_AOV_IDS)));
    REQUIRE(dump(dir + "/image.raw", r.read_image()));
    REQUIRE(dump(dir + "/params.raw", log));
    std::printf("facade_guides: ok\n");
    return 0;
}
