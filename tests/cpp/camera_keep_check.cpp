// rt_camera_keep.hpp on the host: when the kept bits of the camera-ray bounce serve a frame, and when that frame may take the lean camera
// bounce.  Built with the sanitizers and run by tests/test_camera_keep.py.
#include "../../raytracer.glsl_amd/csrc/rt_camera_keep.hpp"
#include <cstdio>
#include <limits>

using namespace rt_camera_keep;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static Camera camera()
{
    Camera c{};
    c.use_dof = 1; c.fov = 0.9f; c.aperture = 0.001f; c.focal = 10.0f;
    c.pos[2] = -30.0f; c.forward[2] = 1.0f; c.up[1] = 1.0f; c.right[0] = 1.0f;
    return c;
}
static Frame frame(const Camera &c) { return Frame{true, true, true, true, 2073600u, 32u, 7u, c}; }
static Key key_of(const Frame &f) { return Key{true, f.n0, f.words, f.scene, f.camera}; }

int main()
{
    const Camera c = camera();
    const Frame f = frame(c);
    const Key k = key_of(f);

    // the standing camera: cached, reused, lean
    Decision d = decide(k, f);
    CHECK(d.cached && d.have_bits && d.ro_add > 2.0f * 0.001f && d.sigma_add > 2.0f * 0.001f / 10.0f);
    CHECK(lean(d, 1, false) && !lean(d, 0, false) && !lean(d, 1, true));

    // nothing valid yet, or a failed frame: rebuilt, not lean
    { Key e = k; e.valid = false; d = decide(e, f); CHECK(d.cached && !d.have_bits && !lean(d, 1, false)); }
    // every field of the key
    { Key e = k; e.n0 += 64u; d = decide(e, f); CHECK(d.cached && !d.have_bits); }
    { Key e = k; e.words += 1u; d = decide(e, f); CHECK(d.cached && !d.have_bits); }
    { Key e = k; e.scene += 1u; d = decide(e, f); CHECK(d.cached && !d.have_bits); }
    { Frame g = f; g.room = false; d = decide(k, g); CHECK(d.cached && !d.have_bits); }
    // every field of the camera
    for (int i = 0; i < 16; ++i) {
        Frame g = f;
        float *fields[16] = {&g.camera.fov, &g.camera.aperture, &g.camera.focal, &g.camera.pos[0], &g.camera.pos[1], &g.camera.pos[2], &g.camera.forward[0], &g.camera.forward[1],
                             &g.camera.forward[2], &g.camera.up[0], &g.camera.up[1], &g.camera.up[2], &g.camera.right[0], &g.camera.right[1], &g.camera.right[2], nullptr};
        if (fields[i]) *fields[i] += 0.0009765625f; else g.camera.use_dof = 0;
        d = decide(k, g);
        CHECK(d.cached && !d.have_bits && !lean(d, 1, false));
    }
    { Frame g = f; g.camera.pos[0] = -0.0f; d = decide(k, g); CHECK(!d.have_bits); }      // bytes, not values
    // frames the cache does not cover: everything as without it
    { Frame g = f; g.culled = false; d = decide(k, g); CHECK(!d.cached && !d.have_bits && d.ro_add == 0.0f && d.sigma_add == 0.0f && !lean(d, 1, false)); }
    { Frame g = f; g.single = false; d = decide(k, g); CHECK(!d.cached && !d.have_bits && !lean(d, 1, false)); }
    { Frame g = f; g.enabled = false; d = decide(k, g); CHECK(!d.cached && !d.have_bits && !lean(d, 1, false)); }

    // the jitter bound: none without depth of field, none worth having from a quarter of the focal length on, NaN and huge values refused
    { Frame g = f; g.camera.use_dof = 0; g.camera.aperture = 100.0f; d = decide(key_of(g), g); CHECK(d.cached && d.have_bits && d.ro_add == 0.0f && d.sigma_add == 0.0f); }
    { Frame g = f; g.camera.aperture = 2.5f; d = decide(key_of(g), g); CHECK(!d.cached && !d.have_bits && d.ro_add == 0.0f && d.sigma_add == 0.0f); }
    { Frame g = f; g.camera.aperture = -2.4f; d = decide(key_of(g), g); CHECK(d.cached && d.ro_add > 4.8f && d.sigma_add > 4.8f / 7.6f); }
    { Frame g = f; g.camera.aperture = std::numeric_limits<float>::quiet_NaN(); d = decide(key_of(g), g); CHECK(!d.cached); }
    { Frame g = f; g.camera.focal = std::numeric_limits<float>::infinity(); d = decide(key_of(g), g); CHECK(!d.cached); }
    { Frame g = f; g.camera.pos[1] = 3.0e18f; d = decide(key_of(g), g); CHECK(!d.cached); }
    { Frame g = f; g.camera.pos[1] = std::numeric_limits<float>::quiet_NaN(); d = decide(key_of(g), g); CHECK(!d.cached); }
    // a NaN field of the camera never compares equal: such a camera rebuilds every frame (it cannot be reused by mistake)
    { Frame g = f; g.camera.use_dof = 0; g.camera.fov = std::numeric_limits<float>::quiet_NaN(); d = decide(key_of(g), g); CHECK(d.cached && !d.have_bits); }

    // the direction bound carries the rounding of pos + jitter and pos + dir * focal, which grows with |pos|.  The cameras at which the
    // first version of the bound (2 |a| / (|f| - |a|) * 1.001 + 4e-6) was smaller than the chord the CPU oracle's rays showed between two
    // frames (tests/test_camera_keep_rays.py measures them again): position, aperture, focal, that chord
    {
        const struct { float pos[3], aperture, focal, chord; } far[5] = {{{1.0e4f, 50.0f, -30.0f}, 0.01f, 2.0f, 0.010291f}, {{3.0e4f, 0.0f, -30.0f}, 0.005f, 1.0f, 0.011717f},
            {{1.0e4f, 1.0e4f, 1.0e4f}, 0.004f, 0.5f, 0.017818f}, {{300.0f, 20.0f, -30.0f}, 0.0002f, 0.01f, 0.041532f}, {{5.0e5f, 0.0f, -30.0f}, 0.05f, 0.3f, 0.4299f}};
        for (int i = 0; i < 5; ++i) {
            Camera g = c; g.aperture = far[i].aperture; g.focal = far[i].focal; std::memcpy(g.pos, far[i].pos, sizeof g.pos);
            float ro = 0.0f, sigma = 0.0f;
            const bool ok = widening(g, &ro, &sigma);
            const float first = 2.0f * far[i].aperture / (far[i].focal - far[i].aperture) * 1.001f + 4.0e-6f;
            CHECK(first < far[i].chord);                                   // (what was wrong; the new bound stays within 2.5 of what was seen: r is twice what the argument needs)
            // the last one jitters by 1.6 ulps of its position with a focal length of 10 ulps: no bound under 1 exists, it is refused
            if (i < 4) CHECK(ok && sigma >= far[i].chord && sigma < 2.5f * far[i].chord && ro > 2.0f * far[i].aperture);
            else CHECK(!ok && ro == 0.0f && sigma == 0.0f);
        }
    }
    // both widenings never shrink as the camera moves away from the origin, and a camera far enough out is refused, never under-bounded
    {
        Camera g = c; g.aperture = 0.01f; g.focal = 2.0f;
        float last_ro = 0.0f, last_sigma = 0.0f; bool refused = false;
        for (float p = 0.0f; p < 1.0e9f; p = p * 1.37f + 0.25f) {
            g.pos[0] = p; g.pos[1] = 0.5f * p; g.pos[2] = -30.0f;
            float ro = 0.0f, sigma = 0.0f;
            const bool ok = widening(g, &ro, &sigma);
            if (refused) CHECK(!ok);                                       // once refused, refused further out
            if (!ok) { refused = true; CHECK(ro == 0.0f && sigma == 0.0f); continue; }
            CHECK(ro >= last_ro && sigma >= last_sigma && sigma < 0.5f);
            last_ro = ro; last_sigma = sigma;
        }
        CHECK(refused && last_sigma > 0.02f);
    }
    // the benchmark's camera (C2: aperture 0.001, focal 10, 35 from the origin): its certificates get no looser than rounding needs
    {
        Camera g = c; g.pos[2] = -35.0f;
        float ro = 0.0f, sigma = 0.0f;
        CHECK(widening(g, &ro, &sigma));
        const float first = 2.0f * 0.001f / (10.0f - 0.001f) * 1.001f + 4.0e-6f;
        CHECK(sigma >= first && sigma - first < 1.0e-5f);
    }

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("camera_keep_check: ok\n");
    return 0;
}
