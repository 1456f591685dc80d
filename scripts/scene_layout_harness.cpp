// The scene re-encoder on the host (csrc/pt_scene_layout.cpp build_layout / plan_sections): the return
// code and message, then per HostLayout array its length, element size and the 64-bit FNV-1a of its
// bytes (every hashed record is written whole: value-initialised or memset by its builder), the
// scalars, and the device section plan.  tests/test_scene_layout.py compares the output with
// tests/golden/scene_layout.txt, recorded from build_layout as it stood inside the C ABI file.
//   C=brown-cs2240-path-tracer_amd/csrc
//   hipcc -x hip --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -I $C scripts/scene_layout_harness.cpp \
//       $C/pt_scene_layout.cpp $C/pt_leafbvh.cpp $C/pt_leafskip.cpp -o harness
//   ./harness triangle_data.f32 bvh_data.f32 [uid_reverse] [leaf_bvh=N] [leaf_skip=0] [dump_bf]
// dump_bf: after the lines above, the stackless replay tree word by word ("bf i node lm rm" per BfNode in
// visiting order, "bn i lm rm" per narrow one), then the tables those words are made from: "nd i lref rref
// lcnt rcnt" per HostLayout node (a child's node or first record, its entry count or -1 for a node) and
// "uid r u" per record, for tests/test_tree_cpu.py.
// Sanitizer run of every case of the test (host code, on a machine without a GPU): the same line with
//   -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pt_scene_layout.h"

static std::vector<float> read_f32(const char* path) {
    std::vector<float> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / 4);
    if (std::fread(v.data(), 4, v.size(), f) != v.size()) { std::fprintf(stderr, "short read of %s\n", path); std::exit(2); }
    std::fclose(f);
    return v;
}

template <class T>
static void row(const char* name, const std::vector<T>& v) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) { h ^= b[i]; h *= 1099511628211ull; }
    std::printf("%s %zu x %zu %016" PRIx64 "\n", name, v.size(), sizeof(T), h);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s triangle_data.f32 bvh_data.f32 [uid_reverse] [leaf_bvh=N] [leaf_skip=0] [dump_bf]\n", argv[0]); return 2; }
    pt::LayoutOptions opt;
    bool dump_bf = false;
    for (int a = 3; a < argc; ++a) {
        if (!std::strcmp(argv[a], "uid_reverse")) opt.uid_reverse = true;
        else if (!std::strncmp(argv[a], "leaf_bvh=", 9)) opt.leaf_bvh = std::atol(argv[a] + 9);
        else if (!std::strcmp(argv[a], "leaf_skip=0")) opt.leaf_skip = false;
        else if (!std::strcmp(argv[a], "dump_bf")) dump_bf = true;
        else { std::fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
    }
    const std::vector<float> tri = read_f32(argv[1]), bvh = read_f32(argv[2]);
    pt::HostLayout L;
    std::string err;
    const int rc = pt::build_layout(tri.data(), tri.size(), bvh.data(), bvh.size(), opt, L, err);
    std::printf("rc %d\nmsg [%s]\n", rc, err.c_str());
    if (rc != PT_OK) return 0;
    row("nodes", L.nodes); row("tris", L.tris); row("mats", L.mats); row("lights", L.lights); row("lmask", L.lmask);
    row("tnorm", L.tnorm); row("bfnode", L.bfnode); row("bfmap", L.bfmap); row("bfnarrow", L.bfnarrow);
    row("lnodes", L.lnodes); row("lidx", L.lidx); row("ltris", L.ltris); row("pnodes", L.pnodes); row("ptris", L.ptris);
    row("pnorm", L.pnorm); row("lleaves", L.lleaves); row("pre", L.pre); row("leaf_sizes", L.leaf_sizes); row("nalt", L.nalt);
    std::printf("leaf_min %d mb_base %d mailbox %d ntri %d fast_rcp %d\n", L.leaf_min, L.mb_base, (int)L.mailbox, L.ntri,
                (int)L.fast_rcp);
    std::printf("skip probe_tests %" PRIu64 " remainders %" PRIu64 " skipped %" PRIu64 " records %" PRIu64 "\n",
                L.skip.probe_tests, L.skip.remainders, L.skip.skipped, L.skip.records);
    const pt_scene_info& i = L.info;
    std::printf("info nodes %u leaves %u leaf_refs %u max_leaf %u max_stack %u materials %u emissive_tris %u vertices %u "
                "device_bytes %" PRIu64 "\n", i.nodes, i.leaves, i.leaf_refs, i.max_leaf, i.max_stack, i.materials,
                i.emissive_tris, i.vertices, (uint64_t)i.device_bytes);
    const pt::ScenePlan p = pt::plan_sections(L, sizeof(pt_counters));
    std::printf("plan");
    for (int s = 0; s < pt::SEC_COUNT; ++s) std::printf(" %zu+%zu", p.sec[s].off, p.sec[s].bytes);
    std::printf("\nspan_end %zu off_counters %zu total %zu\n", p.span_end, p.off_counters, p.total);
    if (dump_bf) {
        for (size_t k = 0; k < L.bfnode.size(); ++k)
            std::printf("bf %zu %d %016" PRIx64 " %016" PRIx64 "\n", k, L.bfmap[k], (uint64_t)L.bfnode[k].lm, (uint64_t)L.bfnode[k].rm);
        for (size_t k = 0; k < L.bfnarrow.size(); ++k)
            std::printf("bn %zu %016" PRIx64 " %016" PRIx64 "\n", k, (uint64_t)L.bfnarrow[k].lm, (uint64_t)L.bfnarrow[k].rm);
        for (size_t k = 0; k < L.nodes.size(); ++k)
            std::printf("nd %zu %d %d %d %d\n", k, L.nodes[k].lref, L.nodes[k].rref, L.nodes[k].lcnt, L.nodes[k].rcnt);
        for (size_t k = 0; k < L.tris.size(); ++k) std::printf("uid %zu %d\n", k, L.tris[k].uid);
    }
    return 0;
}
