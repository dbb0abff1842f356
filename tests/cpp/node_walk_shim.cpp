// C entry point over raytracer.glsl_amd/csrc/rt_node_walk.hpp for tests/test_scene_fuzz_inputs.py: built with the host compiler alone
// (the header holds no HIP), loaded with ctypes.
#include "rt_node_walk.hpp"

#include <cstring>

// Writes at most `capacity` visits to `out` and returns the length of the list, or -1 for "too many" (more than max_visits).
extern "C" long long node_walk_shim(const void *nodes, uint32_t n_nodes, uint32_t n_spheres, unsigned long long max_visits,
                                    uint32_t *out, unsigned long long capacity)
{
    std::vector<uint32_t> visits;
    if (!rt_node_walk::walk(nodes, n_nodes, n_spheres, (size_t)max_visits, visits)) return -1;
    size_t n = visits.size() < capacity ? visits.size() : (size_t)capacity;
    if (n) memcpy(out, visits.data(), n * sizeof(uint32_t));
    return (long long)visits.size();
}
