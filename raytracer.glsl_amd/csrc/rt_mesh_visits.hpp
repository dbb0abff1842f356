// The mesh loops of find_closest_mesh (:336-341) as plain host C++: no HIP in this header, so that the host compiler can build it alone
// (tests/cpp/mesh_visits_check.cpp).  The loops do not depend on the ray: they run once per upload and leave the (mesh, triangle) pairs
// in test order.
//   * meshes in buffer order; a record is (start, size) in its first two 32-bit words, the other two are never read;
//   * the loop bound is the shader's `offset + count` in 32-bit unsigned arithmetic (:341): a sum that wraps runs the loop over
//     [start, wrapped sum) -- nothing at all when the wrapped sum is not above `start`;
//   * a triangle index at or past the vertex buffer reads three all-zero vertices, whose edge tests (`> 0`, :232-238) can never pass:
//     such an index is no visit.  Indices only grow inside one loop, so a loop ends at min(bound, n_tris) -- no 2^32 iterations.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rt_mesh_visits {

constexpr size_t kMeshStride = 16;

// `meshes`: n_meshes records of 16 bytes.  n_tris: whole triangles of the vertex buffer.  Fills visit_mesh / visit_tri (same length).
inline void expand(const void *meshes, uint32_t n_meshes, uint32_t n_tris, std::vector<uint32_t> &visit_mesh, std::vector<uint32_t> &visit_tri)
{
    visit_mesh.clear(); visit_tri.clear();
    const uint8_t *base = (const uint8_t *)meshes;
    for (uint32_t m = 0; m < n_meshes; ++m) {
        uint32_t start, size;
        memcpy(&start, base + (size_t)m * kMeshStride, 4);
        memcpy(&size, base + (size_t)m * kMeshStride + 4, 4);
        const uint32_t bound = start + size;               // uint32: wraps like the shader's
        const uint32_t end = bound < n_tris ? bound : n_tris;
        for (uint32_t t = start; t < end; ++t) { visit_tri.push_back(t); visit_mesh.push_back(m); }
    }
}

}  // namespace rt_mesh_visits
