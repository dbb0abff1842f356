// facade_post.cpp -- the post-process methods of include/rtgl/renderer.h driven the way an integrator would, on facade_demo's scene.
// Used by tests/test_gpu_facade_post.py: every scenario runs on a fresh Renderer after srand(0), logs the uniforms of every frame of any
// kind (set_frame_params_log) and dumps raw what the methods return, so that the test can replay the same inputs through the oracle, a
// host.Context and the numpy mirrors.  Only the facade is called, except rtgl_set_option(renderer.context(), ...) for the three options
// the facade documents that way.  The first method that fails where success is expected (or succeeds where a refusal is) ends the
// program with a code of its own (the check's number in the file, from 10; 120..139 are left out) and its text on stderr.
//   facade_post <dir> <width> <height>        <dir> holds mesh.obj and the six cube map faces, and receives one directory per scenario
#include <cstdio>
#include <cstdlib>
#include <string>
#include <sys/stat.h>

#include "rtgl/renderer.h"

static int exit_code(int id) { return id < 110 ? 10 + id : 30 + id; }
#define REQUIRE(cond)                                                                                                   \
    do {                                                                                                                \
        const int id_ = __COUNTER__;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "facade_post: check %d failed (line %d): %s\n", id_, __LINE__, #cond); return exit_code(id_); } \
    } while (0)

static bool dump(const std::string &path, const void *data, size_t bytes)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    bool ok = std::fwrite(data, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}
template <typename T> static bool dump(const std::string &path, const std::vector<T> &v) { return !v.empty() && dump(path, v.data(), v.size() * sizeof(T)); }

static const float room = 16.0f, sr = 4.0f;

// facade_demo's scene: five spheres through set_kdtree, the octahedron, the sky cube map
static void set_scene(Renderer &renderer, const std::string &dir, bool dump_inputs)
{
    const float r = 10000;
    const std::vector<Sphere> spheres = {
        Sphere({0.0f, -(room + r), 0.0f}, r, 0),
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
    renderer.set_materials(materials);
    renderer.set_kdtree(spheres);
    std::vector<glm::vec4> obj = Renderer::load_obj(dir + "/mesh.obj");
    glm::mat4 matrix = Renderer::transform(glm::vec3(6.0f, -room + sr, -2.0f), glm::vec3(sr), glm::quat(glm::vec3(0.0f, 0.6f, 0.0f)));
    for (glm::vec4 &vertex : obj) {
        vertex = matrix * vertex;
        vertex.w = 6;
    }
    renderer.set_vertices(obj);
    renderer.set_meshes({Mesh(0, (unsigned int)obj.size() / 3, 6)});
    const std::array<std::string, 6> faces = {dir + "/right.png", dir + "/left.png", dir + "/top.png", dir + "/bottom.png", dir + "/front.png", dir + "/back.png"};
    renderer.set_envmap(std::make_unique<CubemapTexture>(faces));
    renderer.set_bounces(4);
    if (dump_inputs) {
        KdTree<Sphere, 1, 2> tree(spheres);
        auto nodes = tree.nodes();
        auto prims = tree.primitives();
        CubemapTexture probe(faces);
        dump(dir + "/materials.raw", materials);
        dump(dir + "/nodes.raw", nodes);
        dump(dir + "/spheres.raw", prims);
        dump(dir + "/vertices.raw", obj);
        dump(dir + "/envmap.raw", probe.data);
    }
}

// one scenario: its directory, its Renderer after srand(0), the log of every frame's uniforms
struct Scenario {
    std::string dir;
    std::vector<rtgl_frame_params> log;
    Renderer renderer;
    Scenario(const std::string &root, const std::string &name, int width, int height, bool dump_inputs = false)
        : dir(root + "/" + name), renderer((srand(0), width), height)
    {
        mkdir(dir.c_str(), 0777);
        set_scene(renderer, root, dump_inputs);
        renderer.set_frame_params_log(&log);
    }
    bool frames(long n) { renderer.set_frame_budget(n); const size_t before = log.size(); renderer.run(); return log.size() == before + (size_t)n; }
    bool put(const std::string &name, const void *data, size_t bytes) const { return dump(dir + "/" + name, data, bytes); }
    template <typename T> bool put(const std::string &name, const std::vector<T> &v) const { return dump(dir + "/" + name, v); }
    bool put_log() const { return put("params.raw", log); }
    std::string path(const std::string &name) const { return dir + "/" + name; }
};

static int planes_denoise(const std::string &root, int w, int h)
{
    Scenario s(root, "planes_denoise", w, h, true);
    Renderer &r = s.renderer;
    REQUIRE(r.context() != nullptr);
    r.set_aov(RTGL_AOV_ALL);
    for (int f = 0; f < 4; ++f) REQUIRE(s.frames(1));
    REQUIRE(s.put("image.raw", r.read_image()));
    REQUIRE(s.put("albedo.raw", r.read_aov(RTGL_AOV_ALBEDO)));
    REQUIRE(s.put("normal.raw", r.read_aov<float>(RTGL_AOV_NORMAL)));
    REQUIRE(s.put("position.raw", r.read_aov(RTGL_AOV_POSITION)));
    REQUIRE(s.put("ids.raw", r.read_aov<int32_t>(RTGL_AOV_IDS)));
    REQUIRE(r.save_aov_pfm(RTGL_AOV_ALBEDO, s.path("albedo.pfm")));
    REQUIRE(r.save_aov_pfm(RTGL_AOV_NORMAL, s.path("normal.pfm")));
    REQUIRE(r.save_aov_pfm(RTGL_AOV_POSITION, s.path("position.pfm")));
    REQUIRE(r.read_aov<float>(RTGL_AOV_IDS).empty());                     // the two documented refusals
    REQUIRE(!r.save_aov_pfm(RTGL_AOV_IDS, s.path("ids.pfm")));
    REQUIRE(r.read_aov<int32_t>(RTGL_AOV_NORMAL).empty());
    REQUIRE(r.denoise());
    REQUIRE(s.put("denoised.raw", r.read_denoised()));
    REQUIRE(r.save_denoised_pfm(s.path("denoised.pfm")));
    REQUIRE(r.denoise_guided());
    REQUIRE(s.put("guided.raw", r.read_denoised()));
    REQUIRE(s.put("guided_variance.raw", r.read_denoise_variance()));
    REQUIRE(s.put("image_after.raw", r.read_image()));                    // (the denoisers leave the image alone)
    REQUIRE(s.put_log());
    return 0;
}

static int temporal_display(const std::string &root, int w, int h, int mode)
{
    Scenario s(root, "temporal_display_" + std::to_string(mode), w, h);
    Renderer &r = s.renderer;
    REQUIRE(r.context() != nullptr);
    r.set_aov(RTGL_AOV_ALBEDO | RTGL_AOV_NORMAL | RTGL_AOV_POSITION);
    REQUIRE(rtgl_set_option(r.context(), "temporal_moments", mode) == RTGL_OK);
    for (int f = 0; f < 6; ++f) {
        const std::string k = "f" + std::to_string(f) + "_";
        if (f % 2 == 0) {                                                // a key held for this frame ...
            r.set_key(SDL_SCANCODE_D, true);
        } else {                                                         // ... or a drag with the left button
            SDL_Event e{};
            e.type = SDL_MOUSEBUTTONDOWN; e.button.button = SDL_BUTTON_LEFT;
            r.push_event(e);
            e = SDL_Event{};
            e.type = SDL_MOUSEMOTION; e.motion.xrel = f; e.motion.yrel = f == 3 ? -1 : 1;
            r.push_event(e);
            e = SDL_Event{};
            e.type = SDL_MOUSEBUTTONUP; e.button.button = SDL_BUTTON_LEFT;
            r.push_event(e);
        }
        REQUIRE(s.frames(1));
        r.set_key(SDL_SCANCODE_D, false);
        REQUIRE(s.log.back().reset_flag == 1);
        REQUIRE(s.put(k + "image.raw", r.read_image()));
        REQUIRE(s.put(k + "albedo.raw", r.read_aov(RTGL_AOV_ALBEDO)));
        REQUIRE(s.put(k + "normal.raw", r.read_aov(RTGL_AOV_NORMAL)));
        REQUIRE(s.put(k + "position.raw", r.read_aov(RTGL_AOV_POSITION)));
        REQUIRE(r.temporal_accumulate());
        REQUIRE(s.put(k + "history.raw", r.read_temporal()));
        REQUIRE(s.put(k + "moments.raw", r.read_temporal_moments()));
        REQUIRE(r.temporal_clip());
        REQUIRE(s.put(k + "history_clipped.raw", r.read_temporal()));
        REQUIRE(s.put(k + "moments_clipped.raw", r.read_temporal_moments()));
    }
    REQUIRE(rtgl_set_option(r.context(), "denoise_source", 1) == RTGL_OK);
    REQUIRE(rtgl_set_option(r.context(), "denoise_variance", 1) == RTGL_OK);
    rtgl_denoise_guided_params g;
    REQUIRE(rtgl_denoise_guided_defaults(&g) == RTGL_OK);
    g.flags &= ~(uint32_t)RTGL_DENOISE_DEMODULATE;                       // moments of mode 1 go with a filter that does not demodulate
    REQUIRE(r.denoise_guided(mode == 2 ? nullptr : &g));
    REQUIRE(s.put("guided.raw", r.read_denoised()));
    REQUIRE(s.put("guided_variance.raw", r.read_denoise_variance()));
    REQUIRE(!r.denoise_guided(mode == 2 ? &g : nullptr));                // the other pairing is refused and leaves the buffer alone
    REQUIRE(s.put("guided_after_refusal.raw", r.read_denoised()));
    REQUIRE(r.tonemap());
    REQUIRE(s.put("display_image.raw", r.read_display(false)));
    rtgl_tonemap_params t;
    REQUIRE(rtgl_tonemap_defaults(&t) == RTGL_OK);
    t.source = RTGL_TONEMAP_SOURCE_DENOISED;
    REQUIRE(r.tonemap(&t));
    REQUIRE(s.put("display_denoised.raw", r.read_display()));
    t.source = RTGL_TONEMAP_SOURCE_TEMPORAL;
    REQUIRE(r.tonemap(&t));
    REQUIRE(s.put("display_temporal.raw", r.read_display(false)));
    REQUIRE(s.put("display_temporal_flipped.raw", r.read_display(true)));
    REQUIRE(r.save_display_png(s.path("display_temporal.png")));
    REQUIRE(r.temporal_reset());
    REQUIRE(r.temporal_accumulate());
    REQUIRE(s.put("history_after_reset.raw", r.read_temporal()));
    REQUIRE(s.put("moments_after_reset.raw", r.read_temporal_moments()));
    REQUIRE(s.put_log());
    return 0;
}

static int until(const std::string &root, int w, int h)
{
    Scenario s(root, "until", w, h);
    Renderer &r = s.renderer;
    REQUIRE(r.context() != nullptr);
    rtgl_error_summary first{}, second{};
    const long a = r.render_until(1.0e-6f, 11, 4, nullptr, &first);      // out of reach: rounds of 4, 4 and 3
    const size_t logged = s.log.size();
    REQUIRE(s.put("image_first.raw", r.read_image()));
    const rtgl_error_summary read_back = r.read_error_summary();
    REQUIRE(std::memcmp(&read_back, &first, sizeof first) == 0);
    const long b = r.render_until(0.5f, 6, 2, nullptr, &second);         // generous: stops at the first round whose summary is converged
    REQUIRE(s.put("image.raw", r.read_image()));
    const int64_t values[4] = {a, (int64_t)logged, b, (int64_t)s.log.size()};
    REQUIRE(s.put("returns.raw", values, sizeof values));
    REQUIRE(s.put("summary_first.raw", &first, sizeof first));
    REQUIRE(s.put("summary_second.raw", &second, sizeof second));
    REQUIRE(s.put_log());
    return 0;
}

static int adaptive(const std::string &root, int w, int h)
{
    Scenario s(root, "adaptive", w, h);
    Renderer &r = s.renderer;
    REQUIRE(r.context() != nullptr);
    rtgl_adaptive_summary sum{};
    const long a = r.render_adaptive(0.2f, 6, 2, 2, &sum);
    REQUIRE(a > 0);
    REQUIRE(s.put("summary.raw", &sum, sizeof sum));
    REQUIRE(s.put("tiles.raw", r.read_adaptive_tiles()));
    REQUIRE(s.put("mask.raw", r.adaptive_get_mask()));
    REQUIRE(s.put("image.raw", r.read_image()));
    // a session driven by hand under a checkerboard of tiles
    rtgl_adaptive_params p;
    REQUIRE(rtgl_adaptive_defaults(&p) == RTGL_OK);
    p.threshold = 0.2f; p.min_samples = 2; p.max_samples = 6;
    REQUIRE(r.adaptive_begin(&p));
    const int tx = (w + 15) / 16, ty = (h + 15) / 16;
    std::vector<uint8_t> checker((size_t)tx * ty);
    for (int y = 0; y < ty; ++y)
        for (int x = 0; x < tx; ++x) checker[(size_t)y * tx + x] = (uint8_t)((x + y) % 2);
    REQUIRE(r.adaptive_set_mask(checker));
    const std::vector<uint8_t> set = r.adaptive_get_mask();
    REQUIRE(s.put("hand_mask_set.raw", set));
    REQUIRE(!r.adaptive_set_mask(std::vector<uint8_t>((size_t)(w / 16) * (h / 16) + 1, 1)));      // a wrong size: refused, the mask stays
    REQUIRE(!r.adaptive_set_mask(std::vector<uint8_t>()));
    REQUIRE(r.adaptive_get_mask() == set);
    for (int f = 0; f < 3; ++f) REQUIRE(r.adaptive_frame());
    REQUIRE(s.put("hand_image_before_update.raw", r.read_image()));
    REQUIRE(r.adaptive_update(&sum));
    REQUIRE(s.put("hand_summary.raw", &sum, sizeof sum));
    REQUIRE(s.put("hand_tiles.raw", r.read_adaptive_tiles()));
    REQUIRE(s.put("hand_mask.raw", r.adaptive_get_mask()));
    REQUIRE(s.put("hand_image.raw", r.read_image()));
    // ordinary frames end the session
    REQUIRE(s.frames(2));
    REQUIRE(!r.adaptive_frame());                                        // (refused: not logged, but its rand() is drawn)
    REQUIRE(s.put("final_image.raw", r.read_image()));
    const int64_t values[2] = {a, (int64_t)s.log.size()};
    REQUIRE(s.put("returns.raw", values, sizeof values));
    REQUIRE(s.put_log());
    return 0;
}

static int robust(const std::string &root, int w, int h)
{
    Scenario s(root, "robust", w, h);
    Renderer &r = s.renderer;
    REQUIRE(r.context() != nullptr);
    REQUIRE(s.frames(2));                                                // the frame count stands at 2: a session frame still sends 0
    const long a = r.render_robust(9, 4, 2.0f, false);
    const long frames_a = r.robust_frames();
    REQUIRE(s.put("robust.raw", r.read_robust()));
    for (uint32_t j = 0; j < 4; ++j) REQUIRE(s.put("bucket" + std::to_string(j) + ".raw", r.read_robust_bucket(j)));
    REQUIRE(r.read_robust_bucket(4).empty());
    REQUIRE(s.put("image_first.raw", r.read_image()));
    r.reset_buffer();                                                    // stays pending through the session
    const long b = r.render_robust(9, 4, 2.0f, true);
    const long frames_b = r.robust_frames();
    REQUIRE(s.put("image_second.raw", r.read_image()));
    for (uint32_t j = 0; j < 4; ++j) REQUIRE(s.put("second_bucket" + std::to_string(j) + ".raw", r.read_robust_bucket(j)));
    REQUIRE(s.frames(2));
    REQUIRE(s.put("final_image.raw", r.read_image()));
    REQUIRE(r.robust_end());
    REQUIRE(r.robust_frames() == -1);
    REQUIRE(r.read_robust().empty());
    REQUIRE(r.read_robust_bucket(0).empty());
    REQUIRE(!r.robust_end());
    const int64_t values[5] = {a, frames_a, b, frames_b, (int64_t)s.log.size()};
    REQUIRE(s.put("returns.raw", values, sizeof values));
    REQUIRE(s.put_log());
    return 0;
}

// a Renderer whose window is closed while it renders: SDL_QUIT arrives after its `at`-th frame, is polled at the start of the next one,
// which Window::run() still renders, and ends the loop there
struct Closing : Renderer {
    int at, seen = 0;
    Closing(int w, int h, int at_) : Renderer(w, h), at(at_) {}
    void render(float dt) override
    {
        Renderer::render(dt);
        if (++seen == at) { SDL_Event e{}; e.type = SDL_QUIT; push_event(e); }
    }
};

// the stop rule m_quit of the three loops: each returns the frames it rendered, which is what the log holds
static int quit(const std::string &root, int w, int h)
{
    const std::string dir = root + "/quit";
    mkdir(dir.c_str(), 0777);
    std::vector<rtgl_frame_params> log;
    srand(0);
    Closing r(w, h, 5);
    REQUIRE(r.context() != nullptr);
    set_scene(r, root, false);
    r.set_frame_params_log(&log);
    rtgl_error_summary es{};
    const long a = r.render_until(1.0e-6f, 11, 4, nullptr, &es);         // a round of 4, then a round cut short after its second frame
    const size_t logged = log.size();
    REQUIRE(dump(dir + "/summary.raw", &es, sizeof es));
    REQUIRE(dump(dir + "/image.raw", r.read_image()));
    const long b = r.render_until(1.0e-6f, 11, 4);                       // the window is closed: nothing more is rendered
    rtgl_adaptive_summary as{};
    const long c = r.render_adaptive(0.2f, 6, 2, 2, &as);                // the session opens (the image is cleared) and no frame follows
    REQUIRE(as.tiles_active > 0 && as.converged == 0);
    const long d = r.render_robust(9, 4, 2.0f, false);
    REQUIRE(r.robust_frames() == 0);
    REQUIRE(r.read_robust().empty());                                    // nothing was folded, nothing resolved
    const int64_t values[5] = {a, (int64_t)logged, b, c, d};
    REQUIRE(log.size() == logged);
    REQUIRE(dump(dir + "/returns.raw", values, sizeof values));
    REQUIRE(dump(dir + "/params.raw", log));
    // SDL_QUIT already waiting when the call begins: the first frame of the first round is the only one
    std::vector<rtgl_frame_params> log2;
    srand(0);
    Closing q(w, h, 0);
    REQUIRE(q.context() != nullptr);
    set_scene(q, root, false);
    q.set_frame_params_log(&log2);
    SDL_Event e{};
    e.type = SDL_QUIT;
    q.push_event(e);
    const int64_t first[2] = {q.render_until(1.0e-6f, 11, 4), (int64_t)log2.size()};
    REQUIRE(dump(dir + "/returns_waiting.raw", first, sizeof first));
    REQUIRE(dump(dir + "/image_waiting.raw", q.read_image()));
    REQUIRE(dump(dir + "/params_waiting.raw", log2));
    return 0;
}

// before the prerequisite call every read-out is empty / zeroed / -1 and every bool false
static int nothing_yet(const std::string &root, int w, int h)
{
    Scenario s(root, "nothing_yet", w, h);
    Renderer &r = s.renderer;
    REQUIRE(r.context() != nullptr);
    const rtgl_error_summary zero{};
    REQUIRE(r.read_denoised().empty());
    REQUIRE(!r.save_denoised_pfm(s.path("denoised.pfm")));
    REQUIRE(r.read_denoise_variance().empty());
    REQUIRE(r.read_temporal().empty());
    REQUIRE(r.read_temporal_moments().empty());
    REQUIRE(!r.temporal_clip());
    REQUIRE(r.read_display().empty());
    REQUIRE(r.read_display(true).empty());
    REQUIRE(!r.save_display_png(s.path("display.png")));
    const rtgl_error_summary e = r.read_error_summary();
    REQUIRE(std::memcmp(&e, &zero, sizeof e) == 0);
    REQUIRE(!r.adaptive_frame());
    REQUIRE(!r.adaptive_update());
    REQUIRE(r.adaptive_get_mask().empty());
    REQUIRE(r.read_adaptive_tiles().empty());
    REQUIRE(!r.adaptive_set_mask(std::vector<uint8_t>((size_t)((w + 15) / 16) * ((h + 15) / 16), 1)));
    REQUIRE(!r.robust_accumulate());
    REQUIRE(!r.robust_resolve());
    REQUIRE(r.read_robust().empty());
    REQUIRE(r.read_robust_bucket(0).empty());
    REQUIRE(r.robust_frames() == -1);
    REQUIRE(!r.robust_end());
    REQUIRE(r.read_aov(RTGL_AOV_NORMAL).empty());                         // the planes are off
    REQUIRE(!r.save_aov_pfm(RTGL_AOV_NORMAL, s.path("normal.pfm")));
    REQUIRE(!r.denoise());                                               // (they need the planes and a frame)
    REQUIRE(!r.denoise_guided());
    REQUIRE(!r.temporal_accumulate());
    REQUIRE(!r.tonemap() || !r.read_display().empty());                   // (the image exists, zeroed: a display of it is allowed)
    r.set_aov(RTGL_AOV_NORMAL);                                          // a masked frame is refused while a plane is on:
    REQUIRE(r.render_adaptive(0.2f, 6, 2, 2) == 0);                      // the loop's first frame fails and is not counted
    r.set_aov(0);
    REQUIRE(s.log.empty());                                              // none of them was a frame (the two refused adaptive_frame()s drew a word each)
    REQUIRE(s.frames(1));                                                // and the renderer still renders
    REQUIRE(s.put("image.raw", r.read_image()));
    REQUIRE(s.put_log());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: facade_post dir width height\n"); return 2; }
    const std::string root = argv[1];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    // The device runtime reseeds rand() when the process's first context brings it up, so a Renderer that renders nothing comes first:
    // from here on a scenario's srand(0) is followed by the words of its own frames only.
    { Renderer first(8, 8); if (!first.context()) return 3; }
    if (int rc = planes_denoise(root, w, h)) return rc;
    if (int rc = temporal_display(root, w, h, 1)) return rc;
    if (int rc = temporal_display(root, w, h, 2)) return rc;
    if (int rc = until(root, w, h)) return rc;
    if (int rc = adaptive(root, w, h)) return rc;
    if (int rc = robust(root, w, h)) return rc;
    if (int rc = quit(root, w, h)) return rc;
    if (int rc = nothing_yet(root, w, h)) return rc;
    std::printf("facade_post: %d checks passed\n", __COUNTER__);
    return 0;
}
