// mesh_visits_check.cpp -- the library's expansion of mesh records into triangle visits (raytracer.glsl_amd/csrc/rt_mesh_visits.hpp, what
// rebuild_triangles in rtgl_amd.hip calls), on the host alone.
// Reads record sets from standard input, one per line:   n_tris n_records  start size word2 word3  start size word2 word3 ...
// and answers each with one line:                        n_visits  mesh tri  mesh tri ...
// tests/test_mesh_fuzz_inputs.py builds this with the address and undefined-behaviour sanitizers and compares the answers with the Python
// restatement of the reference's loops (tests/mesh_fuzz_inputs.py, visits()).  Exit status 0: every line was read and answered.
#include "../../raytracer.glsl_amd/csrc/rt_mesh_visits.hpp"

#include <cstdio>

int main()
{
    unsigned long long n_tris, n_records;
    while (scanf("%llu %llu", &n_tris, &n_records) == 2) {
        if (n_tris > 0xFFFFFFFFull || n_records > (1u << 20)) return 2;
        std::vector<uint32_t> words(4 * (size_t)n_records);
        for (size_t i = 0; i < words.size(); ++i) {
            unsigned long long w;
            if (scanf("%llu", &w) != 1 || w > 0xFFFFFFFFull) return 3;
            words[i] = (uint32_t)w;
        }
        std::vector<uint32_t> visit_mesh, visit_tri;
        rt_mesh_visits::expand(words.data(), (uint32_t)n_records, (uint32_t)n_tris, visit_mesh, visit_tri);
        if (visit_mesh.size() != visit_tri.size()) return 4;
        printf("%zu", visit_tri.size());
        for (size_t i = 0; i < visit_tri.size(); ++i) printf(" %u %u", visit_mesh[i], visit_tri[i]);
        printf("\n");
    }
    return feof(stdin) ? 0 : 5;
}
