// pt_build.h — the device LBVH builder (pt_build.hip) as pt_capi_build.hip drives it: the control words
// the kernels leave for the host, the workspace, and the two halves of a build around the one moment the
// host must know sizes.  The tree itself is specified in include/pt_hip.h and nowhere else.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "../../include/pt_hip.h"
#include "pt_layout.h"

namespace pt {

constexpr int kLbvhMaxDepth = PT_LBVH_MAX_DEPTH;
static_assert(kLbvhMaxDepth - 1 < 32, "max_stack = the deepest internal node's depth stays below kStackMax");
// records a mesh may hold: packed sizes and offsets are 32-bit words on the device (38 floats per record bound them)
constexpr uint32_t kBuildMaxRecords = 1u << 26;

enum : uint32_t { BUILD_ERR_INDEX = 1, BUILD_ERR_MATERIAL = 2, BUILD_ERR_NONFINITE = 4 };

// Device control words: zeroed (bounds and ebox preset to the empty box) before a build, read back twice —
// after the sizes are known (build_tree) and after the emission (build_emit).  Floats are held as
// ordered keys (ord_key: the total order of the header, -0 < +0).
struct BuildCtl {
    uint32_t err;            // BUILD_ERR_* bits
    uint32_t nlit;           // flagged records
    uint32_t bounds[6];      // lo (min), hi (max) over the vertex section
    uint32_t ebox[6];        // the emitter leaf's box
    // the layout (k_build_top)
    uint32_t iso;            // 1: emitter root
    uint32_t two_leaf;       // 1: the whole tree is one leaf's worth: a root with two leaves
    uint32_t radix_kept;     // 1: the radix root is an internal node of the tree
    uint32_t radix_off;      // its packed offset and device node number
    uint32_t radix_num;
    uint32_t packed_len;     // floats, bounds included
    uint32_t n_nodes;        // internal nodes of the tree
    // statistics (emission)
    uint32_t max_leaf;
    uint32_t max_depth;      // the deepest internal node's depth (root 1)
    uint32_t edge_nonfinite; // a record's edge length is not finite
    unsigned long long edge_max;  // max |e1| |e2| over the records, a non-negative double's bits
};

// mesh geometry as the kernels read it (device pointer to the uploaded triangle_data)
struct BuildMesh {
    const float* tri;
    uint32_t tri_len;
    uint32_t nverts, nobj;
    uint32_t v_start, i_start, m_start;
    uint32_t T;
    int32_t vn_start, vn_range;
};

struct BuildNodeAux {  // per radix node, stages 6-7
    float box[12];     // child boxes, exact: lmin lmax rmin rmax
    uint32_t size_l, size_r;  // packed floats of the child subtrees
    uint32_t kn_l, kn_r;      // internal nodes in them
};

// the workspace, carved from one allocation (build_carve)
struct BuildWork {
    BuildCtl* ctl;
    unsigned long long *keys, *keys_alt;  // keys: by record, then sorted in place (keys_alt: the passes' other buffer)
    void* sort_tmp;  // the sort's histograms
    size_t sort_bytes;
    int32_t *parent, *first, *last, *split;  // per radix node
    uint8_t* depth;
    BuildNodeAux* aux;
    uint32_t *off, *num;  // packed offset and device node number per internal node of the tree
};
size_t build_sort_bytes(uint32_t T);
// base NULL: only *total, the bytes the workspace needs
BuildWork build_carve(char* base, uint32_t T, size_t sort_bytes, size_t* total = nullptr);

// Stages 1-6 and the layout: everything up to the sizes.  Asynchronous on stream; the host then reads *w.ctl.
int build_tree(const BuildMesh& m, const BuildWork& w, uint32_t max_leaf, bool isolate, hipStream_t stream);
// Stages 7-8: offsets, then the scene's records and the packed floats (packed: ctl.packed_len floats).
int build_emit(const BuildMesh& m, const BuildWork& w, const BuildCtl& layout, uint32_t max_leaf, Node* nodes, Tri* tris,
               float4* tnorm, float* packed, hipStream_t stream);

}  // namespace pt
