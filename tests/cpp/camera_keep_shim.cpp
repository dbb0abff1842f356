// C entry points over raytracer.glsl_amd/csrc/rt_camera_keep.hpp for tests/test_camera_keep_rays.py and tests/test_camera_keep_inputs.py:
// built with the host compiler alone (the header holds no HIP), loaded with ctypes.  Cameras travel as 16 words laid out like
// rt_camera_keep::Camera; flags as ints.
#include "rt_camera_keep.hpp"

using namespace rt_camera_keep;

static_assert(sizeof(Camera) == 64, "a camera is use_dof, fov, aperture, focal and four vectors: 16 words");

// -> 1 and the two widenings, or 0 (no bound worth having; both widenings 0)
extern "C" int camera_keep_widening(const void *camera, float *ro_add, float *sigma_add)
{
    Camera c;
    std::memcpy(&c, camera, sizeof c);
    return widening(c, ro_add, sigma_add) ? 1 : 0;
}

// key: {valid, n0, words, scene}; frame: {culled, single, enabled, room, n0, words, scene}.  out: {cached, have_bits, lean}; add: {ro_add, sigma_add}
extern "C" void camera_keep_decide(const uint64_t *key, const void *key_camera, const uint64_t *frame, const void *frame_camera, int opt_camera_lean, int aov,
                                   int *out, float *add)
{
    Key k{key[0] != 0, (uint32_t)key[1], (uint32_t)key[2], key[3], Camera{}};
    std::memcpy(&k.camera, key_camera, sizeof k.camera);
    Frame f{frame[0] != 0, frame[1] != 0, frame[2] != 0, frame[3] != 0, (uint32_t)frame[4], (uint32_t)frame[5], frame[6], Camera{}};
    std::memcpy(&f.camera, frame_camera, sizeof f.camera);
    const Decision d = decide(k, f);
    out[0] = d.cached; out[1] = d.have_bits; out[2] = lean(d, opt_camera_lean, aov != 0);
    add[0] = d.ro_add; add[1] = d.sigma_add;
}
