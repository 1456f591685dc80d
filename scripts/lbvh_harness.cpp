// lbvh_harness.cpp — pt_bvh_build_lbvh (csrc/pt_lbvh_host.cpp) in a program of its own, for sanitizer
// builds on the CPU (tests/test_lbvh_cpu.py):
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined lbvh_harness.cpp ../brown-cs2240-path-tracer_amd/csrc/pt_lbvh_host.cpp
// usage: lbvh_harness triangle_data.f32 bvh_out.f32 [max_leaf] [isolate_emitters]
// Size query, build into a buffer of exactly that size, and the refusal of a buffer one float short.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/pt_hip.h"

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s triangle_data.f32 bvh_out.f32 [max_leaf] [isolate_emitters]\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END);
    std::vector<float> tri((size_t)std::ftell(f) / 4);
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(tri.data(), 4, tri.size(), f) != tri.size()) { std::fprintf(stderr, "short read\n"); return 2; }
    std::fclose(f);
    pt_build_params prm;
    pt_build_defaults(&prm);
    if (argc > 3) prm.max_leaf = (uint32_t)std::atoi(argv[3]);
    if (argc > 4) prm.isolate_emitters = (uint32_t)std::atoi(argv[4]);
    size_t n = 0;
    int rc = pt_bvh_build_lbvh(tri.data(), tri.size(), &prm, nullptr, 0, &n);
    if (rc != PT_OK) { std::printf("rc %d\n", rc); return 1; }
    std::vector<float> bvh(n);
    if (n > 1 && pt_bvh_build_lbvh(tri.data(), tri.size(), &prm, bvh.data(), n - 1, &n) != PT_ERR_INVALID) {
        std::printf("a short buffer was accepted\n");
        return 1;
    }
    rc = pt_bvh_build_lbvh(tri.data(), tri.size(), &prm, bvh.data(), bvh.size(), &n);
    if (rc != PT_OK || n != bvh.size()) { std::printf("rc %d\n", rc); return 1; }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(bvh.data(), 4, bvh.size(), f) != bvh.size()) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::fclose(f);
    std::printf("rc 0 floats %zu\n", n);
    return 0;
}
