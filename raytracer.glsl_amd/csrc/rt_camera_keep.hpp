// When the keep bits of the camera-ray bounce (rtgl_amd.hip, d_keep0) serve a frame, as plain host C++: no HIP in this header, so that
// the host compiler can build it alone (tests/cpp/camera_keep_check.cpp).  The scan's launch of bounce 0 and the lean camera bounce
// (option "camera_lean") both go by decide(), once per frame, before anything of the frame is enqueued.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace rt_camera_keep {

// what a camera ray depends on besides its pixel and the frame's random word
struct Camera { int32_t use_dof; float fov, aperture, focal; float pos[3], forward[3], up[3], right[3]; };

// may bits computed for the rays of camera `a` serve camera `b`?  The same camera, field for field (bytes: -0 is not 0, NaN is NaN)
inline bool same_camera(const Camera &a, const Camera &b)
{
    return a.use_dof == b.use_dof && a.fov == b.fov && a.aperture == b.aperture && a.focal == b.focal
           && std::memcmp(a.pos, b.pos, sizeof a.pos) == 0 && std::memcmp(a.forward, b.forward, sizeof a.forward) == 0
           && std::memcmp(a.up, b.up, sizeof a.up) == 0 && std::memcmp(a.right, b.right, sizeof a.right) == 0;
}

// The rays of two frames of one camera differ by the depth-of-field jitter only.  Frame k has o_k = fl(pos + j_k), |j_k| <= 1.0001 |a|,
// and d_k = normalize(fl(F - o_k)) with the focal point F = fl(pos + fl(dir f)), the same floats in every frame.  With u = 2^-24 (half an
// ulp of 1), p = |pos| and every sum rounded per component:
//   |o_j - o_k| <= 2.0002 |a| + 2 u (p + |a|)                                          <= ro_add
//   |v_j - v_k| <= |o_j - o_k| + 2 u max|v|  <= 2.0002 |a| + 4 u (p + |f|)             (v = fl(F - o), |v| <= 1.26 |f|)
//   |v_k|       >= |F - pos| - |o_k - pos| - u |v| >= |f| - 1.0001 |a| - 4 u (p + |f|)  (|dir| >= 1 - 3 u)
//   |d_j - d_k| <= |v_j - v_k| / min |v| + the rounding of two normalisations (< 1e-6)
// r = 8 u (p + |f|) takes the place of each 4 u (p + |f|): twice what the argument needs.  Where |f| - |a| < 4 r the quotient bounds
// nothing worth having (a camera whose jitter is a few ulps of its position): refused like an aperture from |f| / 4 on.
// What packet culling adds to a granule's origin radius and direction spread so that its certificates hold for every frame; false: no
// bound worth having (certify every frame's rays).
inline bool widening(const Camera &c, float *ro_add, float *sigma_add)
{
    *ro_add = *sigma_add = 0.0f;
    if (!c.use_dof) return true;                         // the same ray every frame, bit for bit
    const float a = std::fabs(c.aperture), f = std::fabs(c.focal);
    const float pn = std::sqrt(c.pos[0] * c.pos[0] + c.pos[1] * c.pos[1] + c.pos[2] * c.pos[2]);
    if (!(a < 0.25f * f) || !(f < 1.0e18f) || !(pn < 1.0e18f)) return false;     // (NaN included)
    const float r = 4.76837158203125e-7f * (pn + f);     // 8 u (p + |f|)
    if (!(f - a >= 4.0f * r)) return false;
    *ro_add = 2.0f * a * 1.001f + 1.0e-5f * (1.0f + pn);
    *sigma_add = (2.0f * a * 1.001f + r) / (f - a - r) + 4.0e-6f;
    return true;
}

// what the bits in the buffer were computed for (valid: packet_cull_kernel has been enqueued for them and no frame has failed since)
struct Key { bool valid; uint32_t n0, words; uint64_t scene; Camera camera; };

// one frame.  culled: bounce 0 runs packet culling (option "cull"); single: one frame of one sample per set of launches; enabled: the
// reuse is not switched off (RTGL_AMD_NO_CAMERA_KEEP); room: the buffer in place holds the frame's rows
struct Frame { bool culled, single, enabled, room; uint32_t n0, words; uint64_t scene; Camera camera; };

// cached: bounce 0 is culled from the kept-bits buffer, with the packet bounds widened by (ro_add, sigma_add) when they are computed.
// have_bits: ... and the bits in there serve this frame as they are: packet_cull_kernel does not run on bounce 0.
struct Decision { bool cached, have_bits; float ro_add, sigma_add; };

inline Decision decide(const Key &key, const Frame &f)
{
    Decision d = {false, false, 0.0f, 0.0f};
    if (!f.culled || !f.single || !f.enabled) return d;
    if (!widening(f.camera, &d.ro_add, &d.sigma_add)) { d.ro_add = d.sigma_add = 0.0f; return d; }
    d.cached = true;
    d.have_bits = key.valid && f.room && key.n0 == f.n0 && key.words == f.words && key.scene == f.scene && same_camera(key.camera, f.camera);
    return d;
}

// the lean camera bounce: only on a frame that reuses the bits, with the option on and without first-hit planes
inline bool lean(const Decision &d, int opt_camera_lean, bool aov) { return d.cached && d.have_bits && opt_camera_lean != 0 && !aov; }

}  // namespace rt_camera_keep
