// pt_scene_layout.h — the scene as pt_scene_create uploads it: the reference's packed buffers
// re-encoded into pt_layout.h's records on the host (build_layout), and where each array goes in the
// scene's device allocation (plan_sections).  No HIP runtime call: scripts/scene_layout_harness.cpp
// runs both without a GPU (tests/test_scene_layout.py).
#pragma once
#include <hip/hip_runtime.h>  // pt_layout.h's vector types

#include <string>

#include "../../include/pt_hip.h"
#include "pt_leafbvh.h"

namespace pt {

// leaves of at least this many entries get leaf chunks (option leaf_bvh; the big-leaf threshold):
// exact (tests/test_gpu_leafbvh.py), MedievalBoat +10 % in process; 0 = none
constexpr long kLeafBvhDefault = 128;
// the options pt_scene_create reads (pt_set_option), at their defaults
struct LayoutOptions {
    bool uid_reverse = false;  // mb_uid_order=reverse: mailbox uids numbered backwards (tests)
    long leaf_bvh = kLeafBvhDefault;
    bool leaf_skip = true;     // leaf remainders (pt_leafskip.cpp)
};

struct HostLayout {
    std::vector<Node> nodes;
    std::vector<Tri> tris;
    std::vector<Material> mats;
    std::vector<Light> lights;
    std::vector<uint64_t> lmask;  // mailbox scenes: uid set per leaf, indexed by first record
    std::vector<float4> tnorm;    // vertex-normal mode: 3 per record (SceneView::tnorm)
    std::vector<BfNode> bfnode;   // mailbox scenes with <= 64 internal nodes, <= 63 entries (SceneView::bfnode)
    std::vector<int32_t> bfmap;
    std::vector<BfNode> bfnarrow; // ... of <= 32 internal nodes, <= 32 entries: the narrow payload (SceneView::bfnarrow)
    std::vector<LNode> lnodes;    // leaf BVHs (SceneView::lnodes), and per such leaf (first record, entries, nodes)
    std::vector<int32_t> lidx;
    std::vector<Tri> ltris;       // per chunk slot: its entry's record, lbvh = the entry's position in its leaf
    std::vector<LNode> pnodes;    // the leaf pass's chunks of the pre-resolvable leaves (SceneView::pnodes, PreLeaf c0 / c1)
    std::vector<Tri> ptris;       // per pass chunk slot: its entry's record, lbvh = the entry's position in its leaf
    std::vector<float4> pnorm;    // per pass chunk slot: its entry's unit normal
    std::vector<std::array<int32_t, 3>> lleaves;
    int32_t leaf_min = 0;         // leaves of at least this many entries have one (option leaf_bvh; 0: none)
    std::vector<PreLeaf> pre;     // the kMaxPre largest leaves with their paths (SceneView::pre), largest first
    std::vector<int32_t> leaf_sizes;  // every non-empty leaf's entries, largest first
    std::vector<int2> nalt;       // leaf remainders (SceneView::nalt; empty: none)
    LeafSkipStats skip{};
    int32_t mb_base = 0;          // record of uid 0 (mailbox scenes)
    bool mailbox = false;
    pt_scene_info info{};
    int32_t ntri = 0;
    bool fast_rcp = false;  // SceneView::fast_rcp
};

// Re-encode packer.ts layouts into pt_layout.h.  PT_OK, or PT_ERR_SCENE with
// the reason in err.
int build_layout(const float* tri, size_t tri_len, const float* bvh, size_t bvh_len, const LayoutOptions& opt,
                 HostLayout& L, std::string& err);

// build_layout's materials and light table alone (O(objects + emitters)), for a scene whose tree is
// built elsewhere (pt_scene_create_mesh): the header checked as build_layout checks it, then L.mats,
// L.lights, L.ntri and their pt_scene_info fields.  PT_OK, or PT_ERR_SCENE with the reason in err.
int build_mesh_tables(const float* tri, size_t tri_len, HostLayout& L, std::string& err);

// The scene's device allocation: its sections in upload order.  Those up to SEC_BFNARROW form the
// span kernels stage into LDS ([0, span_end), 16-byte alignment inside it); the counters block
// follows at off_counters; everything starts on 256 bytes otherwise.
enum Section { SEC_NODES, SEC_TRIS, SEC_MATS, SEC_LIGHTS, SEC_LMASK, SEC_BFNODE, SEC_BFMAP, SEC_BFNARROW, SEC_TNORM,
               SEC_LNODES, SEC_LTRIS, SEC_PNODES, SEC_PTRIS, SEC_PNORM, SEC_PRE, SEC_NALT, SEC_COUNT };
struct ScenePlan {
    struct { const void* src; size_t bytes, off; } sec[SEC_COUNT];  // host array, its bytes, its device offset
    size_t span_end, off_counters, total;
};
ScenePlan plan_sections(const HostLayout& L, size_t counters_bytes);

}  // namespace pt
