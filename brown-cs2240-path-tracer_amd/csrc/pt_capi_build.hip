// pt_capi_build.hip — C ABI (include/pt_hip.h): pt_scene_create_mesh and pt_scene_export_bvh.  Host code
// only; the kernels live in pt_build.hip, the tree's rules in the header.
#include <cmath>
#include <memory>

#include "pt_build.h"
#include "pt_capi_internal.h"

using namespace pt;

namespace {

int32_t wgsl_i32(float f) {
    if (std::isnan(f)) return 0;
    if (f >= 2147483647.0f) return INT32_MAX;
    if (f <= -2147483648.0f) return INT32_MIN;
    return (int32_t)f;
}

// the mesh scene's sections as plan_sections lays a packed scene's out: nodes, records, materials, lights
// (the LDS span), the counters, the vertex normals — then the packed floats
struct MeshPlan {
    size_t nodes, tris, mats, lights, span_end, counters, tnorm, packed, total;
};
MeshPlan plan_mesh(size_t n_nodes, size_t n_tris, size_t n_mats, size_t n_lights, size_t packed_len) {
    MeshPlan p{};
    size_t end = 0;
    auto put = [&](size_t bytes, size_t align) { const size_t at = align_up(end, align); end = at + bytes; return at; };
    p.nodes = put(n_nodes * sizeof(Node), 256);
    p.tris = put(std::max<size_t>(1, n_tris) * sizeof(Tri), 256);
    p.mats = put(n_mats * sizeof(Material), 256);
    p.lights = put(n_lights * sizeof(Light), 256);
    p.span_end = end;
    p.counters = put(sizeof(Counters), 256);
    p.tnorm = put(std::max<size_t>(1, 3 * n_tris) * sizeof(float4), 256);
    p.packed = put(packed_len * sizeof(float), 256);
    p.total = align_up(end, 256);
    return p;
}

int bad_mesh(const char* msg) { return fail(PT_ERR_INVALID, msg); }

}  // namespace

extern "C" {

int pt_scene_create_mesh(const float* triangle_data, size_t triangle_len, const pt_build_params* params, int device,
                         pt_scene** scene_out) {
    if (!triangle_data || !scene_out) return fail(PT_ERR_INVALID, "null argument");
    *scene_out = nullptr;
    pt_build_params prm;
    pt_build_defaults(&prm);
    if (params) prm = *params;
    if (prm.max_leaf < 1 || prm.max_leaf > 8 || prm.isolate_emitters > 1 || prm.profile > 1 || prm.reserved)
        return fail(PT_ERR_INVALID, "build parameters: max_leaf 1..8, isolate_emitters and profile 0 | 1, the reserved word 0");
    mark_hip_touched();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PT_ERR_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(PT_ERR_NODEVICE, "device ordinal out of range");
    // materials and lights on the host; this also checks the header as pt_scene_create does
    HostLayout L;
    std::string err;
    if (build_mesh_tables(triangle_data, triangle_len, L, err) != PT_OK) return fail(PT_ERR_INVALID, err);
    const float* tri = triangle_data;
    BuildMesh m{};
    m.tri_len = (uint32_t)triangle_len;
    m.nverts = (uint32_t)tri[0];
    m.nobj = (uint32_t)tri[1];
    const int64_t v_start = wgsl_i32(tri[2]), i_start = wgsl_i32(tri[3]), m_start = wgsl_i32(tri[4]);
    if (i_start < 16 || i_start > m_start || (m_start - i_start) % 4 != 0 || m_start - i_start < 4)
        return bad_mesh("index section of triangle_data out of range or empty");
    if (m.nverts < 1) return bad_mesh("triangle_data has records but no vertices");
    if ((m_start - i_start) / 4 > (int64_t)kBuildMaxRecords) return bad_mesh("more than 2^26 triangle records");
    m.v_start = (uint32_t)v_start;
    m.i_start = (uint32_t)i_start;
    m.m_start = (uint32_t)m_start;
    m.T = (uint32_t)((m_start - i_start) / 4);
    m.vn_start = wgsl_i32(tri[5]);
    m.vn_range = wgsl_i32(tri[6]);
    const uint32_t T = m.T;

    HIP_TRY(hipSetDevice(device));
    // the scene from the start, so that its profiler can take the build's launches; destroyed on every early return
    std::unique_ptr<pt_scene, void (*)(pt_scene*)> owner(new pt_scene(), pt_scene_destroy);
    pt_scene* s = owner.get();
    s->device = device;
    s->prof_on = prm.profile != 0;
    const ProfScope prof_scope(s);
    // the upload and the workspace: freed when this function returns
    Scratch<float> d_tri;
    Scratch<char> d_work;
    PT_TRY(d_tri.ensure(triangle_len, "triangle_data"));
    m.tri = d_tri.p;
    const size_t sort_bytes = build_sort_bytes(T);
    size_t work_bytes = 0;
    build_carve(nullptr, T, sort_bytes, &work_bytes);
    PT_TRY(d_work.ensure(work_bytes, "build workspace"));
    const BuildWork w = build_carve(d_work.p, T, sort_bytes);
    hipStream_t stream = nullptr;  // the null stream: ordered with the blocking copies below
    HIP_TRY(hipMemcpy(d_tri.p, triangle_data, triangle_len * sizeof(float), hipMemcpyHostToDevice));
    if (build_tree(m, w, prm.max_leaf, prm.isolate_emitters != 0, stream) != PT_OK) return fail(PT_ERR_HIP, "LBVH build launch failed");
    // the first readback: the error word, the flagged count, the bounds, the radix root's sizes
    BuildCtl ctl{};
    BuildNodeAux root{};
    HIP_TRY(hipMemcpy(&ctl, w.ctl, sizeof ctl, hipMemcpyDeviceToHost));
    if (ctl.err & BUILD_ERR_INDEX) return bad_mesh("a triangle record references a vertex out of range");
    if (ctl.err & BUILD_ERR_MATERIAL) return bad_mesh("a triangle record references a material out of range");
    if (ctl.err & BUILD_ERR_NONFINITE) return bad_mesh("a triangle record references a vertex with a non-finite coordinate");
    // the layout of the top (include/pt_hip.h: emitter root, two leaves, or the radix root itself)
    const uint32_t E = (prm.isolate_emitters && ctl.nlit > 0 && ctl.nlit < T) ? ctl.nlit : 0, n = T - E;
    ctl.iso = E ? 1 : 0;
    ctl.two_leaf = (!E && n <= prm.max_leaf) ? 1 : 0;
    ctl.radix_kept = n > prm.max_leaf ? 1 : 0;  // (max_leaf >= 1: at least two keys, above the depth cap)
    if (ctl.radix_kept) HIP_TRY(hipMemcpy(&root, w.aux, sizeof root, hipMemcpyDeviceToHost));
    uint64_t plen;
    if (ctl.iso) {
        ctl.radix_off = 6 + 17 + 17 + 4 * E;
        ctl.radix_num = 1;
        plen = (uint64_t)ctl.radix_off + (ctl.radix_kept ? 17ull + root.size_l + root.size_r : 17ull + 4ull * n);
        ctl.n_nodes = 1 + (ctl.radix_kept ? 1 + root.kn_l + root.kn_r : 0);
    } else if (ctl.two_leaf) {
        plen = 6 + 17 + 17 + 17 + 4ull * n;
        ctl.n_nodes = 1;
    } else {
        ctl.radix_off = 6;
        ctl.radix_num = 0;
        plen = 6 + 17ull + root.size_l + root.size_r;
        ctl.n_nodes = 1 + root.kn_l + root.kn_r;
    }
    if (plen > 0xffffffffull) return fail(PT_ERR_INVALID, "packed tree too large");
    ctl.packed_len = (uint32_t)plen;

    const MeshPlan plan = plan_mesh(ctl.n_nodes, T, L.mats.size(), L.lights.size(), ctl.packed_len);
    PT_TRY(s->d_mem.ensure(plan.total, "scene"));
    char* base = s->d_mem.p;
    auto bail = [&](int code, const char* msg) { return fail(code, msg); };
    if (hipMemcpy(base + plan.mats, L.mats.data(), L.mats.size() * sizeof(Material), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(base + plan.lights, L.lights.data(), L.lights.size() * sizeof(Light), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(base + plan.counters, 0, sizeof(Counters)) != hipSuccess)
        return bail(PT_ERR_HIP, "scene upload failed");
    if (build_emit(m, w, ctl, prm.max_leaf, reinterpret_cast<Node*>(base + plan.nodes), reinterpret_cast<Tri*>(base + plan.tris),
                   reinterpret_cast<float4*>(base + plan.tnorm), reinterpret_cast<float*>(base + plan.packed), stream) != PT_OK)
        return bail(PT_ERR_HIP, "LBVH emission launch failed");
    // the second readback: the statistics
    BuildCtl st{};
    if (hipMemcpy(&st, w.ctl, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) return bail(PT_ERR_HIP, "LBVH readback failed");
    if (st.max_depth >= (uint32_t)kStackMax) return bail(PT_ERR_SCENE, "internal: LBVH deeper than the device traversal stack");

    SceneView& v = s->view;
    v.nodes = reinterpret_cast<const Node*>(base + plan.nodes);
    v.tris = reinterpret_cast<const Tri*>(base + plan.tris);
    v.mats = reinterpret_cast<const Material*>(base + plan.mats);
    v.lights = reinterpret_cast<const Light*>(base + plan.lights);
    v.n_nodes = (int32_t)ctl.n_nodes;
    v.n_tris = (int32_t)T;
    v.n_mats = (int32_t)L.mats.size();
    v.n_lights = L.ntri;
    v.f_ntri = (float)L.ntri;
    v.inv_ntri = 1.0f / (float)L.ntri;
    v.max_stack = (int32_t)st.max_depth;
    // fast_rcp_holds' test on the device's reduction, a hair below its bound: the device's double sqrt may
    // round otherwise than the host's, and the flag must never be set where the host would clear it
    double emax;
    static_assert(sizeof emax == sizeof st.edge_max, "a double's bits");
    std::memcpy(&emax, &st.edge_max, sizeof emax);
    v.fast_rcp = (!st.edge_nonfinite && std::isfinite(emax) && emax < std::ldexp(1.0, 124) * (1.0 - 1e-9)) ? 1 : 0;
    v.off_tris = (uint32_t)plan.tris;
    v.off_mats = (uint32_t)plan.mats;
    v.off_lights = (uint32_t)plan.lights;
    v.off_lmask = (uint32_t)align_up(plan.span_end, 16);
    v.lmask = reinterpret_cast<const uint64_t*>(base + v.off_lmask);  // never read: mailbox 0
    v.mailbox = 0;
    v.tnorm = reinterpret_cast<const float4*>(base + plan.tnorm);
    v.off_bfnode = v.off_bfmap = v.off_bfnarrow = v.off_lmask;
    v.span_bytes = (uint32_t)align_up(plan.span_end, 16);
    s->d_counters = reinterpret_cast<Counters*>(base + plan.counters);
    s->info = L.info;  // materials, emissive_tris, vertices
    s->info.nodes = ctl.n_nodes;
    s->info.leaves = ctl.n_nodes + 1;
    s->info.leaf_refs = T;
    s->info.max_leaf = st.max_leaf;
    s->info.max_stack = st.max_depth;
    s->info.device_bytes = plan.total;
    s->mesh_built = true;
    s->packed_off = plan.packed;
    s->packed_len = ctl.packed_len;
    *scene_out = owner.release();
    return PT_OK;
}

int pt_scene_export_bvh(pt_scene* s, float* bvh_out, size_t bvh_cap, size_t* bvh_len) {
    if (!s || !bvh_len || (bvh_cap && !bvh_out)) return fail(PT_ERR_INVALID, "null argument");
    if (!s->mesh_built) return fail(PT_ERR_INVALID, "the scene was not made by pt_scene_create_mesh");
    const struct { size_t off, len; } e{s->packed_off, s->packed_len};
    if (e.len >= (1u << 24)) return fail(PT_ERR_INVALID, "packed tree of 2^24 floats or more: its f32 offsets are not exact");
    *bvh_len = e.len;
    if (bvh_cap < e.len) return bvh_cap ? fail(PT_ERR_INVALID, "bvh_cap smaller than the packed tree") : (int)PT_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(bvh_out, s->d_mem.p + e.off, e.len * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // extern "C"
