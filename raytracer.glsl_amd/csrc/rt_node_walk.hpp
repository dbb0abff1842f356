// The node walk of traverse() (:272-329) as plain host C++: no HIP in this header, so that the host compiler can build it alone
// (tests/cpp/node_walk_shim.cpp).  The walk does not depend on the ray (the AABB cull is compiled out in the reference, :288-292): it
// runs once per node buffer and leaves the sphere indices in test order (`sphere_visits`, rt_device.hpp).
//   * stack of 5 with silently dropped pushes (:113-121), the root is node 0;
//   * a node id past the buffer reads as a childless, empty node; the walk is capped at 65535 pops (llvmpipe's loop cap), so cyclic
//     child links terminate;
//   * the loop bound is the shader's `node.offset + node.count` in 32-bit unsigned arithmetic (:305): a sum that wraps below `offset`
//     runs the loop zero times;
//   * an index past the sphere buffer reads the all-zero sphere.  Testing that record again cannot change a hit (`t < hit.t` is
//     strict), and once an index has left the buffer every later index of the same loop has too (the bound did not wrap), so ONE
//     kNoSphereVisit stands for the rest of that loop.  A loop whose bound lies inside the buffer ends at the bound.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rt_node_walk {

constexpr uint32_t kInvalidNode = 0xFFFFFFFFu;
constexpr uint32_t kNoSphereVisit = 0xFFFFFFFFu;   // == kNoSphere (rt_device.hpp)
constexpr int kStack = 5, kPopCap = 65535;
constexpr size_t kNodeStride = 48;

// `nodes`: n_nodes records of 48 bytes (left, right, offset, count at bytes 32..47).  Fills `visits`; returns false ("too many") as
// soon as the list would exceed max_visits entries.
inline bool walk(const void *nodes, uint32_t n_nodes, uint32_t n_spheres, size_t max_visits, std::vector<uint32_t> &visits)
{
    visits.clear();
    if (n_nodes == 0) return true;
    const uint8_t *base = (const uint8_t *)nodes;
    auto rd = [&](uint32_t node, size_t off) { uint32_t v; memcpy(&v, base + (size_t)node * kNodeStride + off, 4); return v; };
    uint32_t items[kStack] = { 0, 0, 0, 0, 0 };
    int top = 0, pops = 0;
    while (top != -1 && pops < kPopCap) {
        uint32_t id = items[top--];
        pops++;
        uint32_t left = kInvalidNode, right = kInvalidNode, offset = 0, count = 0;
        if (id < n_nodes) { left = rd(id, 32); right = rd(id, 36); offset = rd(id, 40); count = rd(id, 44); }
        if (left != kInvalidNode && top != kStack - 1) items[++top] = left;
        if (right != kInvalidNode && top != kStack - 1) items[++top] = right;
        const uint32_t end = offset + count;               // uint32: wraps like the shader's
        for (uint32_t i = offset; i < end; ++i) {
            const bool inside = i < n_spheres;
            if (visits.size() >= max_visits) return false;
            visits.push_back(inside ? i : kNoSphereVisit);
            if (!inside) break;
        }
    }
    return true;
}

}  // namespace rt_node_walk
