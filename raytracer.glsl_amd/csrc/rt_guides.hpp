// rt_guides.hpp -- the guide pass (include/rtgl_amd.h, "guide pass"; rtgl_guides_frame): the camera ray's first hit folded into the
// first-hit planes without a frame.  One lane per slot of queue 0, one pass, no loop: the launch has ceil(n0 / 256) blocks.
//
//   kMesh = false   a scene without triangle visits: this launch is the whole pass
//   kMesh = true    behind generate_rays_kernel (lean form) and the intersect stage of bounce 0, whose merged hit key it reads from
//                   WaveBuffers::best[0]; the ray itself is rebuilt from the slot, as shade_camera_kernel rebuilds it
//
// Everything that decides a bit is an existing device function (camera_slot_pixel, camera_slot_ray, sphere_pass_id, env_lookup,
// aov_write) or, for the choice between the sphere and the mesh hit, the statements of shade_body, in its order.  What a bounce does
// beyond the hit is absent: no continuation of the generator, no material response, no queue append, no compaction, no counter, no
// image.  No LDS, no barrier, no atomic; the only stores are aov_write's, which go through store_through.
#pragma once
#include "rt_wavefront.hpp"

#pragma clang fp contract(off)

namespace rt {

template <bool kMesh>
__global__ void __launch_bounds__(256) guides_kernel(SceneView sc, FrameParams P, ImageView im, const unsigned long long *__restrict__ best, uint32_t n0, AovView aov)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= n0) return;
    int px, py, lrow;
    if (!camera_slot_pixel(im, slot, px, py, lrow)) return;
    PathState s;
    camera_slot_ray(P, im, px, py, s);
    const uint32_t pixel = (uint32_t)lrow * (uint32_t)im.width + (uint32_t)px;
    unsigned long long key = kNoHitKey;
    if (kMesh) key = best[slot];
    Hit h; h.t = kInf; h.material = 0; h.point = h.normal = mk(0.0f, 0.0f, 0.0f);
    uint32_t sphere_id = kNoSphere;
    const bool hit_sphere = sphere_pass_id(sc, s.o, s.d, h, sphere_id);
    const bool hit_mesh = kMesh && key != kNoHitKey;
    if (!hit_sphere && !hit_mesh) {
        f3 bg;
        if (P.use_envmap) bg = env_lookup(sc, s.d);
        else bg = mk(P.background[0], P.background[1], P.background[2]);
        aov_write(sc, aov, pixel, kAovMiss, h, 0u, bg);
        return;
    }
    const float mesh_t = hit_mesh ? __uint_as_float((uint32_t)(key >> 32)) : kInf;
    int kind = kAovTriangle;
    if (h.t < mesh_t) kind = kAovSphere;
    if (!(h.t < mesh_t)) {                                   // a mesh wins a tie with a sphere
        const TriPlane pl = sc.tri_planes[(uint32_t)key];
        h.t = mesh_t; h.point = s.o + s.d * mesh_t; h.normal = mk(pl.nx, pl.ny, pl.nz); h.material = pl.material;
    }
    aov_write(sc, aov, pixel, kind, h, kind == kAovSphere ? sphere_id : (uint32_t)key, mk(0.0f, 0.0f, 0.0f));
}

}  // namespace rt
