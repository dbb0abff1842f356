// renderer.h -- C++ facade with the reference's Renderer API (src/renderer.h:22-148) over the C ABI in
// include/rtgl_amd.h.  A program written against the reference's `Renderer` (see src/main.cpp there:
// construct, set_* / load_obj / transform, run()) compiles against this header unchanged and links
// librtgl_amd.so instead of OpenGL.  Header-only; any C++17 host compiler.
//
// Kept from the reference: class and method names, argument meaning, POD layouts (static_asserted
// against the shader's buffer strides), copy-on-set ownership, "print and continue" error behaviour
// (src/gfx/gl.cpp:79-94,254-258; src/renderer.cpp:264-267), frame / reset bookkeeping
// (src/renderer.cpp:98,123-127), the camera controls (src/renderer.cpp:311-420).
// Deliberate differences, each one where the reference is in GL-undefined or platform-dependent
// territory: Mesh is 16 bytes on every compiler (item 13); the accumulation image starts
// zeroed (item 9); set_kdtree(vec4) is accepted but only uploads the vertices (item 15: the shader would
// read triangle nodes as sphere ranges); the ImGui panel does not exist (public setters replace it).
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include "../rtgl_amd.h"
#include "glm_shim.h"
#include "kdtree.h"
#include "png_io.h"
#include "window.h"

struct Triangle
{
    glm::vec4 v[3];
    AABB bounds() const { return {glm::min(v[0], glm::min(v[1], v[2])), glm::max(v[0], glm::max(v[1], v[2]))}; }
};
static_assert(sizeof(Triangle) == 48, "3 x vec4 per triangle (shaders/raytracer.glsl:54-56)");

inline std::vector<Triangle> to_triangles(const std::vector<glm::vec4> &vertices)
{
    std::vector<Triangle> out(vertices.size() / 3);     // a trailing partial triangle is dropped
    for (size_t i = 0; i < out.size(); ++i)
        for (int k = 0; k < 3; ++k) out[i].v[k] = vertices[i * 3 + k];
    return out;
}

struct alignas(16) Sphere {
    glm::vec3 center;
    float radius;
    int material = 0;
    Sphere(const glm::vec3 &center_, float radius_, int mat = 0) : center(center_), radius(radius_), material(mat) {}
    AABB bounds() const { return {glm::vec4(center - radius, 0.0f), glm::vec4(center + radius, 0.0f)}; }
};
static_assert(sizeof(Sphere) == 32, "Sphere stride (std140, shaders/raytracer.glsl:11-15)");

// stream form of the reference (src/renderer.h:64-68)
inline std::ostream &operator<<(std::ostream &os, const Sphere &obj)
{
    os << "Sphere { c = " << obj.center << ", r = " << obj.radius << " }";
    return os;
}

enum MaterialType : unsigned int { DIFFUSE = 0, SPECULAR = 1, TRANSMISSIVE = 2 };

struct alignas(16) Material {
    glm::vec4 albedo;        // rgb + smoothness in w
    glm::vec3 emission;
    MaterialType type;
    Material(const glm::vec3 &albedo_, const glm::vec3 &emission_ = glm::vec3(0.0f), float smoothness = 0.0f,
             const MaterialType &type_ = DIFFUSE)
        : albedo(albedo_, smoothness), emission(emission_), type(type_) {}
};
static_assert(sizeof(Material) == 32, "Material stride (std140, shaders/raytracer.glsl:17-21)");

struct alignas(16) Mesh {
    unsigned int start;   // first triangle
    unsigned int size;    // triangle count
    int material;         // unused by the shader
    Mesh(unsigned int start_, unsigned int size_, int mat = 0) : start(start_), size(size_), material(mat) {}
};
static_assert(sizeof(Mesh) == 16, "Mesh stride (std140, shaders/raytracer.glsl:23-27)");

namespace gfx {
// [0,255] -> [0,1] (src/gfx/util.h:11-21)
template <typename T> constexpr glm::vec3 rgb(T r, T g, T b) { return glm::vec3(static_cast<float>(r), static_cast<float>(g), static_cast<float>(b)) / 255.0f; }
constexpr glm::vec3 rgb(uint32_t hex) { return rgb((hex & 0xff0000U) >> 16, (hex & 0x00ff00U) >> 8, (hex & 0x0000ffU) >> 0); }
namespace gl {
// Six 8-bit face images, +X,-X,+Y,-Y,+Z,-Z (src/gfx/gl.h:209-212, src/gfx/gl.cpp:241-260).  A face that
// fails to load prints "failed to load image" and stops, leaving the cube incomplete (lookups return
// black), exactly as the reference does.
struct CubemapTexture {
    int width = 0, height = 0, channels = 0, faces = 0;
    std::vector<uint8_t> data;
    CubemapTexture(const std::array<std::string, 6> &paths, bool flip_vertically = false)
    {
        for (int i = 0; i < 6; ++i) {
            rtgl::Image8 img;
            if (!rtgl::read_png(paths[i], img, flip_vertically) || (faces > 0 && (img.width != width || img.height != height || img.channels != channels))) {
                std::cerr << "failed to load image " << paths[i] << std::endl;
                break;
            }
            width = img.width; height = img.height; channels = img.channels;
            data.insert(data.end(), img.pixels.begin(), img.pixels.end());
            faces++;
        }
    }
    // from memory (no reference counterpart): faces tightly packed in the same order
    CubemapTexture(const uint8_t *pixels, int nfaces, int w, int h, int c)
        : width(w), height(h), channels(c), faces(nfaces), data(pixels, pixels + (size_t)nfaces * w * h * c) {}
};
}  // namespace gl
}  // namespace gfx
using namespace gfx::gl;

inline glm::vec3 vector_from_spherical(float pitch, float yaw)
{
    return {std::cos(yaw) * std::sin(pitch), std::cos(pitch), std::sin(yaw) * std::sin(pitch)};
}

struct Camera {
    glm::vec3 position;
    float fov = 45.0f;
    float focal_length = 10.0f;
    float aperture = 0.001f;
    float pitch = (float)(M_PI / 2);
    float yaw = (float)(M_PI / 2);
    glm::vec3 forward = {0.0f, 0.0f, 1.0f};
    glm::vec3 up = {0.0f, 1.0f, 0.0f};
    glm::vec3 right = {-1.0f, 0.0f, 0.0f};
    Camera(const glm::vec3 &position_, float fov_) : position(position_), fov(fov_) {}
};

class Renderer : public Window
{
public:
    // src/renderer.cpp:21-64; `device` and the tiling arguments are extensions with defaults
    Renderer(int width, int height, int device = 0, int rank = 0, int world = 1, int strip_rows = 16)
        : Window(width, height, "Pathtracer"), m_camera(glm::vec3(0.0f, 0.0f, -35.0f), 33.0f)
    {
        std::vector<int> devices;                                               // RTGL_AMD_DEVICES=0,1,2,3: tile the frame across these GPUs
        if (const char *env = std::getenv("RTGL_AMD_DEVICES"))
            for (const char *c = env; *c;) { char *end = nullptr; const long v = std::strtol(c, &end, 10); if (end == c) break; devices.push_back((int)v); c = (*end == ',') ? end + 1 : end; }
        const int rc = (world == 1 && devices.size() > 1) ? rtgl_create_multi(&m_ctx, width, height, devices.data(), (int)devices.size(), 8)
                                                          : rtgl_create_tiled(&m_ctx, width, height, device, rank, world, strip_rows);
        if (rc != RTGL_OK) {
            std::cerr << "rtgl: " << rtgl_last_error(nullptr) << std::endl;     // the reference prints and carries on
            m_ctx = nullptr;
        }
    }
    // one process, several devices: the frame is tiled across `devices` (strips of strip_rows rows) and gathered to devices[0]
    // when it is read or saved; RTGL_AMD_DEVICES=0,1,2,... does the same for an unmodified caller of Renderer(width, height)
    Renderer(int width, int height, const std::vector<int> &devices, int strip_rows = 8)
        : Window(width, height, "Pathtracer"), m_camera(glm::vec3(0.0f, 0.0f, -35.0f), 33.0f)
    {
        if (rtgl_create_multi(&m_ctx, width, height, devices.data(), (int)devices.size(), strip_rows) != RTGL_OK) {
            std::cerr << "rtgl: " << rtgl_last_error(nullptr) << std::endl;
            m_ctx = nullptr;
        }
    }
    ~Renderer() override { rtgl_destroy(m_ctx); }
    Renderer(const Renderer &) = delete;
    Renderer &operator=(const Renderer &) = delete;

    void render(float dt) override                                          // src/renderer.cpp:66-149
    {
        (void)dt;
        if (!m_ctx) return;
        const rtgl_frame_params p = frame_params(m_frames, m_reset ? 1 : 0);
        record(p);
        if (m_reset) {                       // the stale frame count was already captured above
            m_reset = false;
            m_time = 0; m_frames = 0;
        }
        check(rtgl_set_frame_params(m_ctx, &p));
        check(rtgl_render_frame(m_ctx));
    }

    void event(const SDL_Event &event) override                             // src/renderer.cpp:311-392
    {
        switch (event.type) {
        case SDL_MOUSEBUTTONDOWN: if (event.button.button == SDL_BUTTON_LEFT) m_mousedown = true; break;
        case SDL_MOUSEBUTTONUP: if (event.button.button == SDL_BUTTON_LEFT) m_mousedown = false; break;
        case SDL_MOUSEMOTION:
            if (m_mousedown) {
                const float sensitivity = 0.01f;
                m_camera.yaw += static_cast<float>(event.motion.xrel) * sensitivity;
                m_camera.pitch += static_cast<float>(event.motion.yrel) * sensitivity;
                m_camera.forward = vector_from_spherical(m_camera.pitch, m_camera.yaw);
                m_camera.right = glm::normalize(glm::cross(m_camera.forward, glm::vec3(0.0f, 1.0f, 0.0f)));
                m_camera.up = glm::normalize(glm::cross(m_camera.right, m_camera.forward));
                reset_buffer();
            }
            break;
        case SDL_KEYDOWN:
            if (event.key.repeat != 0) return;
            switch (event.key.keysym.sym) {
            case SDLK_SPACE: save_to_file(); break;
            case SDLK_r: reset_buffer(); break;
            case SDLK_j: m_bounces++; reset_buffer(); break;
            case SDLK_k: if (m_bounces > 1) { m_bounces--; reset_buffer(); } break;
            default: break;
            }
            break;
        default: break;
        }
    }

    void keyboard_state(const Uint8 *state) override                        // src/renderer.cpp:394-420
    {
        const float speed = 10.0f * m_clock.delta;
        auto move = [&](int sc, const glm::vec3 &dir, float sign) {
            if (state[sc]) { m_camera.position += dir * (speed * sign); reset_buffer(); }
        };
        move(SDL_SCANCODE_W, m_camera.forward, +1); move(SDL_SCANCODE_S, m_camera.forward, -1);
        move(SDL_SCANCODE_A, m_camera.right, -1);   move(SDL_SCANCODE_D, m_camera.right, +1);
        move(SDL_SCANCODE_E, m_camera.up, +1);      move(SDL_SCANCODE_Q, m_camera.up, -1);
    }

    // ---- scene setters: synchronous copies, like glBufferData (src/renderer.cpp:151-216)
    void set_spheres(const std::vector<Sphere> &spheres) { if (m_ctx) check(rtgl_upload_spheres(m_ctx, spheres.data(), (uint32_t)spheres.size())); }
    void set_materials(const std::vector<Material> &materials) { if (m_ctx) check(rtgl_upload_materials(m_ctx, materials.data(), (uint32_t)materials.size())); }
    void set_envmap(std::unique_ptr<CubemapTexture> envmap)
    {
        m_envmap = std::move(envmap);
        if (m_ctx && m_envmap)
            check(rtgl_upload_envmap(m_ctx, m_envmap->data.data(), m_envmap->faces, std::max(m_envmap->width, 1), std::max(m_envmap->height, 1),
                                     m_envmap->channels == 3 ? 3 : 4));
    }
    void set_vertices(const std::vector<glm::vec4> &vertices)
    {
        auto triangles = to_triangles(vertices);
        if (m_ctx) check(rtgl_upload_vertices(m_ctx, triangles.data(), (uint32_t)triangles.size() * 3));
    }
    void set_meshes(const std::vector<Mesh> &meshes) { if (m_ctx) check(rtgl_upload_meshes(m_ctx, meshes.data(), (uint32_t)meshes.size())); }
    void set_nodes(const std::vector<KdNode> &nodes) { if (m_ctx) check(rtgl_upload_nodes(m_ctx, nodes.data(), (uint32_t)nodes.size())); }
    void set_kdtree(const std::vector<Sphere> &objects)                     // src/renderer.cpp:193-203
    {
        KdTree<Sphere, 1, 2> tree(objects);
        set_spheres(tree.primitives());
        set_nodes(tree.nodes());
        m_use_bvh = true;
    }
    void set_kdtree(const std::vector<glm::vec4> &objects)                  // src/renderer.cpp:205-216, see header note
    {
        std::cerr << "rtgl: set_kdtree(vertices): triangle nodes are not consumed by the path tracer; uploading vertices only" << std::endl;
        set_vertices(objects);
    }

    // triangle soup with w = 1.0 (src/renderer.cpp:255-304); polygons are fanned; failure -> empty vector
    static std::vector<glm::vec4> load_obj(const std::string &path)
    {
        std::ifstream in(path);
        if (!in) { std::cerr << "obj: cannot open " << path << std::endl; return {}; }
        std::vector<glm::vec3> pos;
        std::vector<glm::vec4> out;
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string tag;
            ls >> tag;
            if (tag == "v") { glm::vec3 p; ls >> p.x >> p.y >> p.z; pos.push_back(p); }
            else if (tag == "f") {
                std::vector<long> idx;
                std::string tok;
                while (ls >> tok) {
                    long i = std::strtol(tok.c_str(), nullptr, 10);          // "v", "v/vt", "v//vn", "v/vt/vn"
                    if (i < 0) i = (long)pos.size() + i + 1;
                    idx.push_back(i);
                }
                for (size_t k = 1; k + 1 < idx.size(); ++k)
                    for (long i : {idx[0], idx[k], idx[k + 1]}) {
                        if (i < 1 || (size_t)i > pos.size()) { std::cerr << "obj: bad index in " << path << std::endl; return {}; }
                        out.emplace_back(pos[(size_t)i - 1], 1.0f);
                    }
            }
        }
        std::printf("# of vertices  = %d\n# of triangles = %d\n", (int)pos.size(), (int)out.size() / 3);
        return out;
    }

    // T * R * S (src/renderer.cpp:247-253)
    static glm::mat4 transform(const glm::vec3 &translate, const glm::vec3 &scale, const glm::quat &rotate = glm::quat(glm::vec3(0.0f)))
    {
        return glm::translate(glm::mat4(1.0f), translate) * glm::mat4(rotate) * glm::scale(glm::mat4(1.0f), scale);
    }

    // ---- what the ImGui panel exposes in the reference (src/renderer.cpp:68-83)
    void reset_buffer() { m_reset = true; }
    void set_bounces(int b) { m_bounces = b; }
    void set_use_envmap(bool v) { m_use_envmap = v; }
    void set_use_dof(bool v) { m_use_dof = v; }
    void set_background(const glm::vec3 &c) { m_background = c; }
    Camera &camera() { return m_camera; }
    rtgl_context *context() { return m_ctx; }
    const rtgl_frame_params &last_frame_params() const { return m_last_params; }   // what the last frame of any kind uploaded
    // every frame of any kind (render(), adaptive_frame(), robust_frame(), also inside run() and the render_*() loops) appends what it
    // uploaded to `log` (extension; nullptr: stop).  The vector is the caller's and must outlive the logging.  A session frame that the
    // library refused (no session, say) has drawn its rand() but is neither logged nor shown by last_frame_params().
    void set_frame_params_log(std::vector<rtgl_frame_params> *log) { m_params_log = log; }

    // 8-bit, clamped, vertically flipped PNG named render_<W>x<H>_<unixtime>_<frames>.png (src/renderer.cpp:218-245)
    void save_to_file() const
    {
        if (!m_ctx) return;
        const int rows = rtgl_local_rows(m_ctx);
        std::vector<uint8_t> px((size_t)m_width * rows * 4);
        if (rtgl_read_image_u8(m_ctx, px.data(), 1) != RTGL_OK) { std::cerr << rtgl_last_error(m_ctx) << std::endl; return; }
        const std::time_t ts = std::chrono::system_clock::to_time_t(std::chrono::system_clock::now());
        const std::string filename = "render_" + std::to_string(m_width) + "x" + std::to_string(m_height) + "_" + std::to_string(ts) + "_" + std::to_string(m_frames) + ".png";
        if (rtgl::write_png(filename, px.data(), m_width, rows, 4)) std::cout << "Wrote render to " << filename << std::endl;
        else std::cerr << "Could not write render to " << filename << std::endl;
    }
    // raw accumulation image, RGBA32F, row 0 = bottom (extension)
    std::vector<float> read_image() const
    {
        std::vector<float> img((size_t)m_width * (m_ctx ? rtgl_local_rows(m_ctx) : 0) * 4);
        if (m_ctx) check(rtgl_read_image_f32(m_ctx, img.data()));
        return img;
    }


    // ---- lossless outputs and a resumable state (the reference itself only writes the 8-bit PNG above).  Like the
    // reference's file operations they print and return false on failure.
    // RGBA32F as it sits in the accumulation image: width * height * 16 bytes, no header, row 0 = bottom
    bool save_raw(const std::string &path) const
    {
        const std::vector<float> img = read_image();
        return write_file(path, "", img.data(), img.size() * sizeof(float));
    }
    // Portable float map: "PF\n<w> <h>\n-1.0\n" (colour, little-endian), RGB float32, bottom row first -- the image's own row order
    bool save_pfm(const std::string &path) const { return write_pfm(path, read_image()); }

    // ---- first-hit planes (option "aov", include/rtgl_amd.h; extension): albedo, normal, position and hit ids of the camera ray's first hit.
    // set_aov(mask of RTGL_AOV_* bits) allocates the planes zeroed and restarts their running mean; 0 frees them.
    void set_aov(int mask) { if (m_ctx) check(rtgl_set_option(m_ctx, "aov", mask)); }
    // one plane (a single RTGL_AOV_* bit), 4 values per pixel, row 0 = bottom: read_aov(RTGL_AOV_NORMAL) for the float planes,
    // read_aov<int32_t>(RTGL_AOV_IDS) for the ids.  Empty (and a message) when the plane is not enabled or T does not fit it.
    template <typename T = float>
    std::vector<T> read_aov(int plane) const
    {
        static_assert(std::is_same<T, float>::value || std::is_same<T, int32_t>::value, "the planes hold float32 or int32 values");
        if (!m_ctx) return {};
        if ((plane == RTGL_AOV_IDS) != std::is_same<T, int32_t>::value) { std::cerr << "rtgl: read_aov: the ids plane is int32, the others float" << std::endl; return {}; }
        std::vector<T> out((size_t)m_width * rtgl_local_rows(m_ctx) * 4);
        if (rtgl_read_aov(m_ctx, plane, out.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return out;
    }
    // a float plane as a PFM, exactly like save_pfm (its first three channels)
    bool save_aov_pfm(int plane, const std::string &path) const
    {
        if (plane == RTGL_AOV_IDS) { std::cerr << "rtgl: save_aov_pfm: the ids plane is not a float image" << std::endl; return false; }
        const std::vector<float> img = read_aov(plane);
        if (!m_ctx || img.size() != (size_t)m_width * rtgl_local_rows(m_ctx) * 4) return false;      // (read_aov has said why)
        return write_pfm(path, img);
    }
    // ---- guide pass (rtgl_guides_frame, include/rtgl_amd.h; extension): the camera rays' first hits folded into the enabled planes and
    // nothing else -- no image, no RNG state, no session ends.  guides_frame(): one pass with the uniforms of a frame (one rand(), like every
    // frame; frames and reset_flag are ignored, the frame count is not advanced and a pending reset_buffer() stays pending).
    // render_guides(n): n passes, returns how many the library took.  Prints and returns false / stops on failure.
    bool guides_frame() { return masked_frame(rtgl_guides_frame); }
    long render_guides(long n = 1)
    {
        long done = 0;
        while (done < n && guides_frame()) ++done;
        return done;
    }
    // ---- denoiser (rtgl_denoise, include/rtgl_amd.h; extension): an edge-avoiding a-trous filter over the image as it stands, guided by the
    // first-hit planes -- set_aov(RTGL_AOV_ALBEDO | RTGL_AOV_NORMAL | RTGL_AOV_POSITION) before rendering.  nullptr: the documented defaults.
    // The result is a snapshot in a buffer of its own; the accumulation image is not touched.  Prints and returns false on failure.
    bool denoise(const rtgl_denoise_params *params = nullptr)
    {
        if (!m_ctx) return false;
        const int rc = rtgl_denoise(m_ctx, params);
        check(rc);
        return rc == RTGL_OK;
    }
    // ... or the variance-guided filter with its firefly clamp (rtgl_denoise_guided): the same buffer, read with read_denoised().
    // nullptr: its defaults (passes 5, sigma_lum 4, sigma_normal 0.3, sigma_position 0.05, firefly_ratio 1, demodulate on)
    bool denoise_guided(const rtgl_denoise_guided_params *params = nullptr)
    {
        if (!m_ctx) return false;
        const int rc = rtgl_denoise_guided(m_ctx, params);
        check(rc);
        return rc == RTGL_OK;
    }
    // {mu, v0, variance after the last pass, s0} per pixel of the last denoise_guided(); empty (and a message) before the first
    std::vector<float> read_denoise_variance() const
    {
        if (!m_ctx) return {};
        std::vector<float> img((size_t)m_width * rtgl_local_rows(m_ctx) * 4);
        if (rtgl_read_denoise_variance_f32(m_ctx, img.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return img;
    }
    // the denoised image, RGBA32F, row 0 = bottom; empty (and a message) before the first successful denoise() or denoise_guided()
    std::vector<float> read_denoised() const
    {
        if (!m_ctx) return {};
        std::vector<float> img((size_t)m_width * rtgl_local_rows(m_ctx) * 4);
        if (rtgl_read_denoised_f32(m_ctx, img.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return img;
    }
    // ... as a PFM, exactly like save_pfm
    bool save_denoised_pfm(const std::string &path) const
    {
        const std::vector<float> img = read_denoised();
        if (!m_ctx || img.size() != (size_t)m_width * rtgl_local_rows(m_ctx) * 4) return false;      // (read_denoised has said why)
        return write_pfm(path, img);
    }
    // ---- temporal accumulation (rtgl_temporal_accumulate, include/rtgl_amd.h; extension): the history of the previous view reprojected into
    // the current one and blended with the image as it stands -- set_aov(RTGL_AOV_NORMAL | RTGL_AOV_POSITION), render every frame with
    // reset_flag = 1, frames = 0 and call this after it.  nullptr: its defaults (max_history 32, sigma_normal 0.3, sigma_position 0.05).
    // Prints and returns false on failure.
    bool temporal_accumulate(const rtgl_temporal_params *params = nullptr)
    {
        if (!m_ctx) return false;
        const int rc = rtgl_temporal_accumulate(m_ctx, params);
        check(rc);
        return rc == RTGL_OK;
    }
    // ---- temporal clip (rtgl_temporal_clip, include/rtgl_amd.h; extension): the history temporal_accumulate() just wrote clamped into the
    // colour box of the current frame's 7 x 7 geometric neighbourhood, the history length of a clamped pixel cut -- call it right after
    // temporal_accumulate(), so that lighting that changed without the geometry changing does not ghost.  nullptr: its defaults
    // (sigma_scale 2, clip_history 3, sigma_normal 0.3, sigma_position 0.05).  Prints and returns false on failure.
    bool temporal_clip(const rtgl_temporal_clip_params *params = nullptr)
    {
        if (!m_ctx) return false;
        const int rc = rtgl_temporal_clip(m_ctx, params);
        check(rc);
        return rc == RTGL_OK;
    }
    // the next temporal_accumulate() starts without history
    bool temporal_reset()
    {
        if (!m_ctx) return false;
        const int rc = rtgl_temporal_reset(m_ctx);
        check(rc);
        return rc == RTGL_OK;
    }
    // ---- display transform (rtgl_tonemap, include/rtgl_amd.h; extension): the image, the denoised buffer or the temporal history exposed,
    // tone-mapped and sRGB-encoded into an RGBA8 display buffer on the device.  nullptr: its defaults (source 0, op 1, auto exposure on,
    // exposure 1, key 0.18, white 4, adapt 1, exposure_min 2^-16, exposure_max 2^16, low_permille 100, high_permille 20).  save_to_file()
    // stays the reference's clamp; this is the picture to look at.  Prints and returns false on failure.
    bool tonemap(const rtgl_tonemap_params *params = nullptr)
    {
        if (!m_ctx) return false;
        const int rc = rtgl_tonemap(m_ctx, params);
        check(rc);
        return rc == RTGL_OK;
    }
    // the display buffer of the last tonemap(), RGBA8, row 0 = bottom unless flip; empty (and a message) before the first successful tonemap()
    std::vector<uint8_t> read_display(bool flip = false) const
    {
        if (!m_ctx) return {};
        std::vector<uint8_t> px((size_t)m_width * rtgl_local_rows(m_ctx) * 4);
        if (rtgl_read_display_u8(m_ctx, px.data(), flip ? 1 : 0) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return px;
    }
    // the display buffer as a PNG, top row first like save_to_file()
    bool save_display_png(const std::string &path) const
    {
        const std::vector<uint8_t> px = read_display(true);
        if (px.empty()) return false;
        return rtgl::write_png(path, px.data(), m_width, rtgl_local_rows(m_ctx), 4);
    }
    // ---- error estimate (rtgl_error_estimate, include/rtgl_amd.h; extension): how noisy the accumulation image still is, per 16 x 16 tile and
    // for the picture, from the image and the luminance snapshot the previous call left.  nullptr: its defaults (threshold 0.05, floor 0.01,
    // quantile_permille 950, first_frames 1, flags 0) -- run() counts the frames the reference's way, so first_frames is 1.  The first call,
    // and the first after reset_buffer() has taken effect, only takes the snapshot (summary.valid == 0).  Prints and returns false on failure.
    bool error_estimate(const rtgl_error_params *params = nullptr)
    {
        if (!m_ctx) return false;
        const int rc = rtgl_error_estimate(m_ctx, params);
        check(rc);
        return rc == RTGL_OK;
    }
    // the summary of the last error_estimate() (synchronises); all zero (and a message) before the first successful one
    rtgl_error_summary read_error_summary() const
    {
        rtgl_error_summary s{};
        if (m_ctx && rtgl_read_error_summary(m_ctx, &s) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; s = rtgl_error_summary{}; }
        return s;
    }
    // "render until the picture is this clean": run() in rounds of check_every frames with an error_estimate() after each, until a summary
    // is converged at `threshold` (a relative RMSE per tile; the other parameters from `params`, nullptr: the defaults), m_quit is set or
    // max_frames frames have been rendered by this call.  Returns the frames rendered; `summary` (if not null) receives the latest summary.
    // The frame budget is left at the size of the last round.
    long render_until(float threshold, long max_frames, long check_every = 16, const rtgl_error_params *params = nullptr, rtgl_error_summary *summary = nullptr)
    {
        rtgl_error_params p;
        rtgl_error_defaults(&p);
        if (params) p = *params;
        p.threshold = threshold;
        rtgl_error_summary s{};
        long done = 0;
        while (m_ctx && !m_quit && done < max_frames && check_every > 0) {
            const long round = std::min(check_every, max_frames - done);
            const long before = m_recorded;
            set_frame_budget(round);
            run();
            done += m_recorded - before;                         // (what run() rendered: SDL_QUIT cuts a round short)
            if (!error_estimate(&p)) break;
            s = read_error_summary();
            if (s.valid && s.converged) break;
        }
        if (summary) *summary = s;
        return done;
    }
    // ---- adaptive sampling (rtgl_adaptive_*, include/rtgl_amd.h; extension): frames that trace only the 16 x 16 tiles that are still noisy.
    // adaptive_begin() clears the image and opens a session (nullptr: the defaults, threshold 0.05, floor 0.01, min_samples 16, max_samples
    // 1024, flags 0); adaptive_frame() renders one sample over the active tiles with the uniforms render() would send (one rand() per frame;
    // the frame count is not advanced and a pending reset_buffer() stays pending for the next render(): a tile's own count is what the
    // accumulation divides by); adaptive_update() estimates the tiles, sets
    // the mask and returns the summary.  render(), reset of the image and load_state() end the session.  Each prints and returns false on failure.
    bool adaptive_begin(const rtgl_adaptive_params *params = nullptr)
    {
        if (!m_ctx) return false;
        rtgl_adaptive_params p;
        rtgl_adaptive_defaults(&p);
        if (params) p = *params;
        const int rc = rtgl_adaptive_begin(m_ctx, &p);
        check(rc);
        return rc == RTGL_OK;
    }
    bool adaptive_frame() { return masked_frame(rtgl_adaptive_frame); }
    bool adaptive_update(rtgl_adaptive_summary *summary = nullptr)
    {
        rtgl_adaptive_summary s{};
        if (!m_ctx) return false;
        const int rc = rtgl_adaptive_update(m_ctx, &s);
        check(rc);
        if (summary) *summary = s;
        return rc == RTGL_OK;
    }
    // the mask, ceil(width / 16) x ceil(height / 16) bytes, row by row, non-zero = active; set: until the next adaptive_update()
    bool adaptive_set_mask(const std::vector<uint8_t> &tiles) { return set_tile_mask(rtgl_adaptive_set_mask, tiles); }
    std::vector<uint8_t> adaptive_get_mask() const { return get_tile_mask(rtgl_adaptive_get_mask); }
    // the tile records, row by row; empty (and a message) before the first adaptive_begin()
    std::vector<rtgl_adaptive_tile> read_adaptive_tiles() const { return read_tile_records(rtgl_read_adaptive_tiles); }
    // "render until every tile is this clean": a session of masked frames with an adaptive_update() after every check_every of them, until
    // no tile is active (each is at or below `threshold`, a relative RMSE, or holds max_samples samples) or m_quit is set.  Returns the
    // frames rendered; `summary` (if not null) receives the latest summary.
    long render_adaptive(float threshold, uint32_t max_samples, uint32_t min_samples = 16, long check_every = 16, rtgl_adaptive_summary *summary = nullptr)
    {
        rtgl_adaptive_params p;
        rtgl_adaptive_defaults(&p);
        p.threshold = threshold; p.max_samples = max_samples; p.min_samples = min_samples;
        rtgl_adaptive_summary s{};
        long done = 0;
        bool ok = check_every > 0 && adaptive_begin(&p) && adaptive_update(&s);
        while (ok && !m_quit && !s.converged) {
            for (long i = 0; ok && i < check_every; ++i) { ok = adaptive_frame(); if (ok) ++done; }
            ok = ok && adaptive_update(&s);
        }
        if (summary) *summary = s;
        return done;
    }
    // ---- robust accumulation (rtgl_robust_*, include/rtgl_amd.h; extension): the frames dealt round-robin into bucket means, and a resolve
    // that drops the buckets whose luminance disagrees with the others, so that a firefly does not stay in the picture with weight 1/N.
    // robust_begin() opens a session (nullptr: the defaults, buckets 8, flags 0); robust_frame() renders one frame of one sample with the
    // uniforms render() would send, but with frames = 0 and reset_flag = 1 (one rand() per frame; the frame count is not advanced and a
    // pending reset_buffer() stays pending for the next render()), and
    // folds it into the next bucket; robust_accumulate() folds the image as it stands; robust_resolve() writes the trimmed mean (nullptr:
    // the defaults, gain 1, dest 0, flags 0) to the output plane (read_robust()) or, with dest RTGL_ROBUST_DEST_IMAGE, to the accumulation
    // image, which denoise(), tonemap() and save_to_file() then take; robust_end() frees the planes.  Each prints and returns false on failure.
    bool robust_begin(const rtgl_robust_params *params = nullptr)
    {
        if (!m_ctx) return false;
        rtgl_robust_params p;
        rtgl_robust_defaults(&p, nullptr);
        if (params) p = *params;
        const int rc = rtgl_robust_begin(m_ctx, &p);
        check(rc);
        return rc == RTGL_OK;
    }
    bool robust_accumulate()
    {
        if (!m_ctx) return false;
        const int rc = rtgl_robust_accumulate(m_ctx);
        check(rc);
        return rc == RTGL_OK;
    }
    bool robust_frame()
    {
        if (!m_ctx) return false;
        const rtgl_frame_params p = frame_params(0, 1);
        int rc = rtgl_set_frame_params(m_ctx, &p);
        if (rc == RTGL_OK) rc = rtgl_render_frame(m_ctx);
        if (rc == RTGL_OK) record(p);                          // (the frame was rendered, whatever the fold says)
        if (rc == RTGL_OK) rc = rtgl_robust_accumulate(m_ctx);
        check(rc);
        return rc == RTGL_OK;
    }
    bool robust_resolve(const rtgl_robust_resolve_params *params = nullptr)
    {
        if (!m_ctx) return false;
        rtgl_robust_resolve_params p;
        rtgl_robust_defaults(nullptr, &p);
        if (params) p = *params;
        const int rc = rtgl_robust_resolve(m_ctx, &p);
        check(rc);
        return rc == RTGL_OK;
    }
    bool robust_end()
    {
        if (!m_ctx) return false;
        const int rc = rtgl_robust_end(m_ctx);
        check(rc);
        return rc == RTGL_OK;
    }
    // the frames folded since robust_begin(); -1 (and a message) without a session
    long robust_frames() const
    {
        uint32_t n = 0;
        if (!m_ctx) return -1;
        if (rtgl_robust_frames(m_ctx, &n, nullptr) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return -1; }
        return (long)n;
    }
    // the output plane of the latest robust_resolve() with dest RTGL_ROBUST_DEST_BUFFER, RGBA32F, row 0 = bottom, a = the Gini coefficient
    // of the pixel's bucket luminances; empty (and a message) before one
    std::vector<float> read_robust() const
    {
        if (!m_ctx) return {};
        std::vector<float> img((size_t)m_width * rtgl_local_rows(m_ctx) * 4);
        if (rtgl_read_robust_f32(m_ctx, img.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return img;
    }
    // the mean of the frames bucket j holds, RGBA32F
    std::vector<float> read_robust_bucket(uint32_t j) const
    {
        if (!m_ctx) return {};
        std::vector<float> img((size_t)m_width * rtgl_local_rows(m_ctx) * 4);
        if (rtgl_read_robust_bucket_f32(m_ctx, j, img.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return img;
    }
    // "a picture of `frames` samples without its fireflies": robust_begin(), `frames` times robust_frame() (or until m_quit is set), then
    // robust_resolve().  Returns the frames rendered; with to_image the accumulation image holds the picture, otherwise read_robust() gives it.
    long render_robust(long frames, uint32_t buckets = 8, float gain = 1.0f, bool to_image = false)
    {
        rtgl_robust_params p;
        rtgl_robust_resolve_params rp;
        rtgl_robust_defaults(&p, &rp);
        p.buckets = buckets; rp.gain = gain; rp.dest = to_image ? RTGL_ROBUST_DEST_IMAGE : RTGL_ROBUST_DEST_BUFFER;
        long done = 0;
        bool ok = frames > 0 && robust_begin(&p);
        while (ok && !m_quit && done < frames) { ok = robust_frame(); if (ok) ++done; }
        if (ok && done > 0) robust_resolve(&rp);
        return done;
    }
    // ---- robust error estimate (rtgl_robust_error_estimate, include/rtgl_amd.h; extension): how noisy the picture robust_resolve() makes
    // still is, per 16 x 16 tile and for the picture, from the spread of the open session's buckets.  nullptr: its defaults (threshold 0.05,
    // floor 0.01, the resolve's gain 1, quantile_permille 950, flags 0).  Needs as many frames as buckets.  Prints and returns false on failure.
    bool robust_error_estimate(const rtgl_robust_error_params *params = nullptr)
    {
        if (!m_ctx) return false;
        const int rc = rtgl_robust_error_estimate(m_ctx, params);
        check(rc);
        return rc == RTGL_OK;
    }
    // the summary of the session's last robust_error_estimate() (synchronises); all zero (and a message) before the first successful one
    rtgl_error_summary read_robust_error_summary() const
    {
        rtgl_error_summary s{};
        if (m_ctx && rtgl_read_robust_error_summary(m_ctx, &s) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; s = rtgl_error_summary{}; }
        return s;
    }
    // "a picture without its fireflies, this clean": robust_begin(), robust_frame() in rounds of check_every frames with a
    // robust_error_estimate() after each round once the session holds `buckets` frames, until a summary is converged at `threshold` (a
    // relative RMSE per tile, of the picture resolved with `gain`; floor and quantile from `params`, nullptr: the defaults), m_quit is set, a
    // frame is refused or max_frames frames have been rendered; then robust_resolve() with the same gain.  Returns the frames rendered (a
    // refused frame is not counted); `summary` (if not null) receives the latest summary, all zero if no estimate was made.
    long render_robust_until(float threshold, long max_frames, long check_every = 16, uint32_t buckets = 8, float gain = 1.0f, bool to_image = false,
                             const rtgl_robust_error_params *params = nullptr, rtgl_error_summary *summary = nullptr)
    {
        rtgl_robust_params p;
        rtgl_robust_resolve_params rp;
        rtgl_robust_error_params ep;
        rtgl_robust_defaults(&p, &rp);
        rtgl_robust_error_defaults(&ep);
        if (params) ep = *params;
        p.buckets = buckets; rp.gain = gain; rp.dest = to_image ? RTGL_ROBUST_DEST_IMAGE : RTGL_ROBUST_DEST_BUFFER;
        ep.threshold = threshold; ep.gain = gain;
        rtgl_error_summary s{};
        long done = 0;
        bool ok = max_frames > 0 && check_every > 0 && robust_begin(&p);
        while (ok && !m_quit && done < max_frames) {
            const long round = std::min(check_every, max_frames - done);
            for (long k = 0; ok && !m_quit && k < round; ++k) { ok = robust_frame(); if (ok) ++done; }
            if (!ok || done < (long)buckets) continue;
            if (!robust_error_estimate(&ep)) break;
            s = read_robust_error_summary();
            if (s.valid && s.converged) break;
        }
        if (done > 0 && m_ctx) robust_resolve(&rp);
        if (summary) *summary = s;
        return done;
    }
    // ---- robust denoise (rtgl_robust_denoise, include/rtgl_amd.h; extension): the resolve of the open session and the variance-guided filter
    // in one call, the luminance tolerance of every pixel taken from the spread of its own buckets; the result is read with read_denoised()
    // and read_denoise_variance(), or tone-mapped with source 1.  nullptr: its defaults (passes 5, sigma_lum 4, sigma_normal 0.3,
    // sigma_position 0.05, gain 1, demodulate on).  Needs as many frames as buckets and the first-hit planes the parameters use.  The session,
    // the image and the planes are only read.  Prints and returns false on failure.
    bool robust_denoise(const rtgl_robust_denoise_params *params = nullptr)
    {
        if (!m_ctx) return false;
        const int rc = rtgl_robust_denoise(m_ctx, params);
        check(rc);
        return rc == RTGL_OK;
    }
    // ---- robust adaptive sampling (rtgl_robust_adaptive_*, include/rtgl_amd.h; extension): a session whose sample count is per 16 x 16 tile
    // and whose samples go into bucket means: frames trace only the tiles that are still noisy, and fireflies decide neither the picture nor
    // when a tile stops.  It holds its own buffers beside an adaptive and a robust session and does not touch the image.
    // robust_adaptive_begin() opens a session (nullptr: the defaults, buckets 8, threshold 0.05, floor 0.01, gain 1, min_samples 32,
    // max_samples 1024, flags 0); robust_adaptive_frame() renders one sample over the active tiles with the uniforms render() would send (one
    // rand() per frame; the frame count is not advanced and a pending reset_buffer() stays pending for the next render()) and folds it into
    // the bucket of each tile's next sample; robust_adaptive_accumulate() folds the image as it stands; robust_adaptive_update() estimates
    // the tiles whose count has moved, sets the mask and returns the summary; robust_adaptive_resolve() writes the trimmed mean, every pixel
    // with its tile's count (nullptr: the defaults, gain 1, dest 0, flags 0), to the session's output plane (read_robust_adaptive()) or, with
    // dest RTGL_ROBUST_DEST_IMAGE, to the accumulation image; robust_adaptive_end() frees the buffers.  Each prints and returns false on failure.
    bool robust_adaptive_begin(const rtgl_robust_adaptive_params *params = nullptr)
    {
        if (!m_ctx) return false;
        rtgl_robust_adaptive_params p;
        rtgl_robust_adaptive_defaults(&p);
        if (params) p = *params;
        const int rc = rtgl_robust_adaptive_begin(m_ctx, &p);
        check(rc);
        return rc == RTGL_OK;
    }
    bool robust_adaptive_frame() { return masked_frame(rtgl_robust_adaptive_frame); }
    bool robust_adaptive_accumulate()
    {
        if (!m_ctx) return false;
        const int rc = rtgl_robust_adaptive_accumulate(m_ctx);
        check(rc);
        return rc == RTGL_OK;
    }
    bool robust_adaptive_update(rtgl_adaptive_summary *summary = nullptr)
    {
        rtgl_adaptive_summary s{};
        if (!m_ctx) return false;
        const int rc = rtgl_robust_adaptive_update(m_ctx, &s);
        check(rc);
        if (summary) *summary = s;
        return rc == RTGL_OK;
    }
    // the mask, ceil(width / 16) x ceil(height / 16) bytes, row by row, non-zero = active; set: until the next robust_adaptive_update()
    bool robust_adaptive_set_mask(const std::vector<uint8_t> &tiles) { return set_tile_mask(rtgl_robust_adaptive_set_mask, tiles); }
    std::vector<uint8_t> robust_adaptive_get_mask() const { return get_tile_mask(rtgl_robust_adaptive_get_mask); }
    bool robust_adaptive_resolve(const rtgl_robust_resolve_params *params = nullptr)
    {
        if (!m_ctx) return false;
        rtgl_robust_resolve_params p;
        rtgl_robust_defaults(nullptr, &p);
        if (params) p = *params;
        const int rc = rtgl_robust_adaptive_resolve(m_ctx, &p);
        check(rc);
        return rc == RTGL_OK;
    }
    bool robust_adaptive_end()
    {
        if (!m_ctx) return false;
        const int rc = rtgl_robust_adaptive_end(m_ctx);
        check(rc);
        return rc == RTGL_OK;
    }
    // the output plane of the latest robust_adaptive_resolve() with dest RTGL_ROBUST_DEST_BUFFER, RGBA32F, row 0 = bottom, a = the Gini
    // coefficient of the pixel's bucket luminances; empty (and a message) before one
    std::vector<float> read_robust_adaptive() const
    {
        if (!m_ctx) return {};
        std::vector<float> img((size_t)m_width * rtgl_local_rows(m_ctx) * 4);
        if (rtgl_read_robust_adaptive_f32(m_ctx, img.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return img;
    }
    // the mean of the samples bucket j holds, RGBA32F
    std::vector<float> read_robust_adaptive_bucket(uint32_t j) const
    {
        if (!m_ctx) return {};
        std::vector<float> img((size_t)m_width * rtgl_local_rows(m_ctx) * 4);
        if (rtgl_read_robust_adaptive_bucket_f32(m_ctx, j, img.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return img;
    }
    // the session's tile records, row by row; empty (and a message) without a session
    std::vector<rtgl_adaptive_tile> read_robust_adaptive_tiles() const { return read_tile_records(rtgl_read_robust_adaptive_tiles); }
    // "render until every tile of the picture without its fireflies is this clean": a robust adaptive session of masked frames with a
    // robust_adaptive_update() after every check_every of them, until no tile is active (each is at or below `threshold`, a relative RMSE of
    // the picture resolved with `gain`, or holds max_samples samples) or m_quit is set; then robust_adaptive_resolve() with the same gain.
    // min_samples 0: the default.  Returns the frames rendered; `summary` (if not null) receives the latest summary; with to_image the
    // accumulation image holds the picture, otherwise read_robust_adaptive() gives it.
    long render_robust_adaptive(float threshold, uint32_t max_samples, uint32_t min_samples = 0, long check_every = 16, uint32_t buckets = 8, float gain = 1.0f,
                                bool to_image = false, rtgl_adaptive_summary *summary = nullptr)
    {
        rtgl_robust_adaptive_params p;
        rtgl_robust_resolve_params rp;
        rtgl_robust_adaptive_defaults(&p);
        rtgl_robust_defaults(nullptr, &rp);
        p.buckets = buckets; p.threshold = threshold; p.gain = gain; p.max_samples = max_samples;
        if (min_samples) p.min_samples = min_samples;
        rp.gain = gain; rp.dest = to_image ? RTGL_ROBUST_DEST_IMAGE : RTGL_ROBUST_DEST_BUFFER;
        rtgl_adaptive_summary s{};
        long done = 0;
        bool ok = check_every > 0 && robust_adaptive_begin(&p) && robust_adaptive_update(&s);
        const bool begun = ok;
        while (ok && !m_quit && !s.converged) {
            for (long i = 0; ok && i < check_every; ++i) { ok = robust_adaptive_frame(); if (ok) ++done; }
            ok = ok && robust_adaptive_update(&s);
        }
        if (begun) robust_adaptive_resolve(&rp);
        if (summary) *summary = s;
        return done;
    }
    // the history, RGBA32F, row 0 = bottom, a = the history length; empty (and a message) before the first successful temporal_accumulate()
    std::vector<float> read_temporal() const
    {
        if (!m_ctx) return {};
        std::vector<float> img((size_t)m_width * rtgl_local_rows(m_ctx) * 4);
        if (rtgl_read_temporal_f32(m_ctx, img.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return img;
    }
    // the luminance moments {m1, m2, v, n} of the history (rtgl_set_option(context(), "temporal_moments", 1 or 2) before temporal_accumulate()), RGBA32F,
    // row 0 = bottom; empty (and a message) unless the latest successful temporal_accumulate() stored moments
    std::vector<float> read_temporal_moments() const
    {
        if (!m_ctx) return {};
        std::vector<float> img((size_t)m_width * rtgl_local_rows(m_ctx) * 4);
        if (rtgl_read_temporal_moments_f32(m_ctx, img.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return img;
    }
    // The progressive state: the accumulation image and the frame counters the running mean depends on (u_frames, src/renderer.cpp:98).
    // load_state() into a Renderer of the same size continues exactly where save_state() stopped: the next frame is mixed in with
    // weight 1 / (frames + 1) as if the process had never ended.  (u_random continues from the caller's rand() stream, which is not
    // part of the state; scene and camera are the caller's to restore.)
    bool save_state(const std::string &path) const
    {
        const std::vector<float> img = read_image();
        StateHeader h{};
        std::memcpy(h.magic, "RTGLST01", 8);
        h.width = m_width; h.height = (int32_t)(img.size() / 4 / (size_t)std::max(m_width, 1)); h.frames = m_frames; h.time = m_time;
        return write_file(path, std::string(reinterpret_cast<const char *>(&h), sizeof h), img.data(), img.size() * sizeof(float));
    }
    bool load_state(const std::string &path)
    {
        std::ifstream f(path, std::ios::binary);
        StateHeader h{};
        if (!f || !f.read(reinterpret_cast<char *>(&h), sizeof h) || std::memcmp(h.magic, "RTGLST01", 8) != 0) { std::cerr << "Could not read state from " << path << std::endl; return false; }
        if (!m_ctx || h.width != m_width || h.height != rtgl_local_rows(m_ctx)) { std::cerr << "State in " << path << " is " << h.width << "x" << h.height << ", not this renderer's size" << std::endl; return false; }
        std::vector<float> img((size_t)h.width * h.height * 4);
        if (!f.read(reinterpret_cast<char *>(img.data()), (std::streamsize)(img.size() * sizeof(float)))) { std::cerr << "State in " << path << " is truncated" << std::endl; return false; }
        if (rtgl_write_image_f32(m_ctx, img.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return false; }
        m_frames = h.frames; m_time = h.time; m_reset = false;
        return true;
    }

private:
    struct StateHeader { char magic[8]; int32_t width, height, frames; float time; };
    // Portable float map of the RGB channels of an RGBA float image
    bool write_pfm(const std::string &path, const std::vector<float> &img) const
    {
        std::vector<float> rgb(img.size() / 4 * 3);
        for (size_t i = 0; i < img.size() / 4; ++i) { rgb[3 * i] = img[4 * i]; rgb[3 * i + 1] = img[4 * i + 1]; rgb[3 * i + 2] = img[4 * i + 2]; }
        const std::string head = "PF\n" + std::to_string(m_width) + " " + std::to_string(img.size() / 4 / (size_t)std::max(m_width, 1)) + "\n-1.0\n";
        return write_file(path, head, rgb.data(), rgb.size() * sizeof(float));
    }
    static bool write_file(const std::string &path, const std::string &head, const void *data, size_t bytes)
    {
        std::ofstream f(path, std::ios::binary);
        if (f) { f.write(head.data(), (std::streamsize)head.size()); f.write(static_cast<const char *>(data), (std::streamsize)bytes); }
        if (!f) { std::cerr << "Could not write " << path << std::endl; return false; }
        return true;
    }
    // The uniforms of one frame of any kind, marshalled in one place (src/renderer.cpp:96-122): one rand() per call; the caller says what
    // `frames` and `reset_flag` carry.
    rtgl_frame_params frame_params(int frames, int reset_flag)
    {
        rtgl_frame_params p{};
        p.time = m_time;
        p.frames = frames;
        p.samples = m_samples;
        p.max_bounce = static_cast<unsigned int>(m_bounces);
        std::memcpy(p.background, &m_background.x, sizeof p.background);
        p.random = rand();
        p.use_envmap = m_envmap ? (m_use_envmap ? 1 : 0) : 0;
        p.use_dof = m_use_dof ? 1 : 0;
        std::memcpy(p.camera_position, &m_camera.position.x, 12);
        p.camera_fov = glm::radians(m_camera.fov);
        p.camera_aperture = m_camera.aperture;
        p.camera_focal_length = m_camera.focal_length;
        std::memcpy(p.camera_forward, &m_camera.forward.x, 12);
        std::memcpy(p.camera_right, &m_camera.right.x, 12);
        std::memcpy(p.camera_up, &m_camera.up.x, 12);
        p.reset_flag = reset_flag;
        return p;
    }
    // a frame the library took: last_frame_params(), the log if one is set, the count render_until() goes by
    void record(const rtgl_frame_params &p)
    {
        m_last_params = p;
        if (m_params_log) m_params_log->push_back(p);
        ++m_recorded;
    }
    void check(int rc) const { if (rc != RTGL_OK) std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; }
    // ---- what the adaptive_*() and robust_adaptive_*() twins share; `fn` is the library call of the caller's kind
    size_t tile_count() const { return (size_t)((m_width + 15) / 16) * (size_t)((m_height + 15) / 16); }
    bool masked_frame(int (*fn)(rtgl_context *))
    {
        if (!m_ctx) return false;
        const rtgl_frame_params p = frame_params(0, 0);        // (a masked frame ignores frames and reset_flag)
        int rc = rtgl_set_frame_params(m_ctx, &p);
        if (rc == RTGL_OK) rc = fn(m_ctx);
        if (rc == RTGL_OK) record(p);
        check(rc);
        return rc == RTGL_OK;
    }
    bool set_tile_mask(int (*fn)(rtgl_context *, const uint8_t *), const std::vector<uint8_t> &tiles)
    {
        if (!m_ctx || tiles.size() != tile_count()) return false;
        const int rc = fn(m_ctx, tiles.data());
        check(rc);
        return rc == RTGL_OK;
    }
    std::vector<uint8_t> get_tile_mask(int (*fn)(rtgl_context *, uint8_t *)) const
    {
        if (!m_ctx) return {};
        std::vector<uint8_t> tiles(tile_count());
        if (fn(m_ctx, tiles.data()) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return tiles;
    }
    std::vector<rtgl_adaptive_tile> read_tile_records(int (*fn)(rtgl_context *, rtgl_adaptive_tile *, uint32_t *, uint32_t *)) const
    {
        if (!m_ctx) return {};
        std::vector<rtgl_adaptive_tile> tiles(tile_count());
        if (fn(m_ctx, tiles.data(), nullptr, nullptr) != RTGL_OK) { std::cerr << "rtgl: " << rtgl_last_error(m_ctx) << std::endl; return {}; }
        return tiles;
    }

    rtgl_context *m_ctx = nullptr;
    rtgl_frame_params m_last_params{};
    std::vector<rtgl_frame_params> *m_params_log = nullptr;
    long m_recorded = 0;
    std::unique_ptr<CubemapTexture> m_envmap = nullptr;
    int m_bounces = 5;
    unsigned int m_samples = 1;
    Camera m_camera;
    bool m_reset = false;
    bool m_mousedown = false;
    bool m_use_envmap = true;
    bool m_use_dof = true;
    bool m_use_bvh = false;
    glm::vec3 m_background = glm::vec3(0.52f, 0.80f, 0.92f);
};
