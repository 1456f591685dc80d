// pt_capi.hip — C ABI (include/pt_hip.h): errors, options, the build id, kernel timing, devices and the
// scene's life.  The other entry points: pt_capi_render.hip, _adaptive, _denoise, _query, _selftest, _multi.
// Host code only; kernels live in pt_kernels.hip, the scene's re-encoding in pt_scene_layout.cpp.
#include <algorithm>
#include <cstdio>

#include "pt_capi_internal.h"

using namespace pt;

namespace {

thread_local std::string g_err;

// ---------------------------------------------------------------------------------------------
// Options (pt_set_option): the process-wide table of kernel-selection switches.  Nothing is read
// from the environment; tests and A/B scripts set these explicitly.
// ---------------------------------------------------------------------------------------------
enum OptKind { OPT_BOOL, OPT_INT, OPT_ENUM };
struct OptSpec {
    const char* name;
    OptKind kind;
    const char* choices;  // OPT_ENUM: '|'-separated values
};
constexpr OptSpec kOptSpecs[] = {
    {"kernel", OPT_ENUM, "auto|mega|wavefront|literal"},
    {"trav", OPT_ENUM, "nested|flat1|pred|lean|lean2|lean4|lean8|lean16|lean32"},
    {"lds", OPT_BOOL, nullptr},          {"fastrcp", OPT_BOOL, nullptr},     {"dual", OPT_BOOL, nullptr},
    {"fuse", OPT_BOOL, nullptr},         {"fuse_gen", OPT_BOOL, nullptr},    {"bf", OPT_BOOL, nullptr},
    {"mailbox", OPT_BOOL, nullptr},      {"bf_stackless", OPT_BOOL, nullptr}, {"trace_sparse", OPT_INT, nullptr},
    {"bf_narrow", OPT_BOOL, nullptr},    {"step_addr64", OPT_BOOL, nullptr},
    {"region_perm", OPT_BOOL, nullptr},  {"regen", OPT_INT, nullptr},  {"trace_ring", OPT_INT, nullptr},
    {"parts", OPT_INT, nullptr},         {"sort", OPT_INT, nullptr},
    {"node_bias", OPT_INT, nullptr},     {"node_steps", OPT_INT, nullptr},     {"big_leaf", OPT_INT, nullptr},     {"bf_slots", OPT_INT, nullptr},
    {"leaf_pre", OPT_INT, nullptr},      {"leaf_blocks", OPT_INT, nullptr},  {"leaf_pairs", OPT_INT, nullptr},
    {"pre_ratio", OPT_INT, nullptr},     {"leaf_refine", OPT_BOOL, nullptr},
    {"wf_paths", OPT_INT, nullptr},      {"wf_trace_blocks", OPT_INT, nullptr}, {"trace_watchdog", OPT_INT, nullptr},
    {"leaf_bvh", OPT_INT, nullptr},      {"leaf_walk", OPT_BOOL, nullptr},   {"leaf_pool", OPT_BOOL, nullptr},   {"pool_run", OPT_ENUM, "2|4"},
    {"leaf_skip", OPT_BOOL, nullptr},
    {"mb_uid_order", OPT_ENUM, "forward|reverse"},
    {"reduce", OPT_ENUM, "rccl|ordered"},
    {"denoise_lds", OPT_ENUM, "0|1|2|3|4"},
    {"query_refill", OPT_BOOL, nullptr}, {"query_blocks", OPT_INT, nullptr},
};
static_assert(sizeof(kOptSpecs) / sizeof(kOptSpecs[0]) == kNumOpts, "pt_capi_internal.h kNumOpts");
constexpr int count_choices(const char* c) {
    int n = 1;
    for (; *c; ++c) n += *c == '|';
    return n;
}
// launch_opts takes a trav choice's position for its TravBase
static_assert(kOptSpecs[1].name[0] == 't' && count_choices(kOptSpecs[1].choices) == TRAV_BASE_COUNT, "option trav");

std::mutex g_opt_mu;
std::string g_opt_val[kNumOpts];  // "" = default

int choice_index(const char* choices, const char* v) {
    const size_t n = std::strlen(v);
    int k = 0;
    for (const char* c = choices; *c; ++k) {
        const char* bar = std::strchr(c, '|');
        const size_t len = bar ? (size_t)(bar - c) : std::strlen(c);
        if (len == n && !std::strncmp(c, v, n)) return k;
        c += len + (bar ? 1 : 0);
    }
    return -1;
}

bool opt_valid(const OptSpec& s, const char* v) {
    if (!*v) return false;
    if (s.kind == OPT_BOOL) return !std::strcmp(v, "0") || !std::strcmp(v, "1");
    if (s.kind == OPT_INT) {
        char* end = nullptr;
        const long long x = std::strtoll(v, &end, 10);
        return *end == 0 && x >= 0 && x <= 0x7fffffffLL;
    }
    return choice_index(s.choices, v) >= 0;
}

// Set once any call of this library has touched the HIP runtime (pt_set_hw_queues is then too late).
bool g_hip_touched = false;

}  // namespace

namespace pt {

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

void mark_hip_touched() { g_hip_touched = true; }

int opt_index(const char* name) {
    for (int i = 0; i < kNumOpts; ++i)
        if (!std::strcmp(name, kOptSpecs[i].name)) return i;
    return -1;
}
int opt_choice(const char* name, const char* value) {
    const int i = opt_index(name);
    return i >= 0 && kOptSpecs[i].kind == OPT_ENUM ? choice_index(kOptSpecs[i].choices, value) : -1;
}
Opts opts_snapshot() {
    std::lock_guard<std::mutex> lk(g_opt_mu);
    Opts o;
    for (int i = 0; i < kNumOpts; ++i) o.v[i] = g_opt_val[i];
    return o;
}

}  // namespace pt

extern "C" {

int pt_set_option(const char* name, const char* value) {
    if (!name) return fail(PT_ERR_INVALID, "option name is NULL");
    const int i = opt_index(name);
    if (i < 0) return fail(PT_ERR_INVALID, std::string("unknown option '") + name + "'");
    if (value && !opt_valid(kOptSpecs[i], value))
        return fail(PT_ERR_INVALID, std::string("bad value '") + value + "' for option '" + name + "'");
    std::lock_guard<std::mutex> lk(g_opt_mu);
    g_opt_val[i] = value ? value : "";
    return PT_OK;
}

int pt_get_option(const char* name, char* buf, size_t cap) {
    if (!name || !buf || cap == 0) return fail(PT_ERR_INVALID, "null argument");
    const int i = opt_index(name);
    if (i < 0) return fail(PT_ERR_INVALID, std::string("unknown option '") + name + "'");
    std::lock_guard<std::mutex> lk(g_opt_mu);
    if (g_opt_val[i].size() + 1 > cap) return fail(PT_ERR_INVALID, "buffer too small");
    std::memcpy(buf, g_opt_val[i].c_str(), g_opt_val[i].size() + 1);
    return PT_OK;
}

void pt_reset_options(void) {
    std::lock_guard<std::mutex> lk(g_opt_mu);
    for (auto& v : g_opt_val) v.clear();
}

#ifndef PT_SOURCE_HASH
#define PT_SOURCE_HASH "unknown"
#endif
const char* pt_build_id(void) { return PT_SOURCE_HASH; }

}  // extern "C"

namespace pt {
thread_local KernelProfiler* t_prof = nullptr;

hipEvent_t KernelProfiler::take() {
    hipEvent_t e = nullptr;
    if (!pool.empty()) {
        e = pool.back();
        pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
    }
    return e;
}
void KernelProfiler::start(int kid, hipStream_t st) {
    Rec r{kid, take(), take()};
    if (r.a) hipEventRecord(r.a, st);
    recs.push_back(r);
}
void KernelProfiler::stop(hipStream_t st) {
    if (!recs.empty() && recs.back().b) hipEventRecord(recs.back().b, st);
}
void KernelProfiler::reset() {
    for (auto& r : recs) {
        if (r.a) pool.push_back(r.a);
        if (r.b) pool.push_back(r.b);
    }
    recs.clear();
}
void KernelProfiler::destroy() {
    reset();
    for (auto e : pool) hipEventDestroy(e);
    pool.clear();
}
}  // namespace pt

extern "C" {

int pt_abi_version(void) { return PT_ABI_VERSION; }

int pt_profile_enable(pt_scene* s, int enable) {
    if (!s) return fail(PT_ERR_INVALID, "null scene");
    HIP_TRY(hipSetDevice(s->device));
    s->prof.reset();
    s->prof_on = enable != 0;
    return PT_OK;
}

int pt_profile_select(pt_scene* s, const char* kernel) {
    if (!s) return fail(PT_ERR_INVALID, "null scene");
    if (!kernel) { s->prof.only = -1; return PT_OK; }
    for (int k = 0; k < KID_COUNT; ++k)
        if (!std::strcmp(kernel, kernel_name(k))) { s->prof.only = k; return PT_OK; }
    return fail(PT_ERR_INVALID, "unknown kernel name");
}

int pt_profile_read(pt_scene* s, pt_kernel_time* out, int max_entries, int* n_out) {
    if (!s || !n_out || (max_entries > 0 && !out)) return fail(PT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    pt_kernel_time acc[KID_COUNT] = {};
    // launch intervals relative to the first record's start event (events of one device compare
    // across streams): their union per kernel is its busy time
    std::vector<std::pair<double, double>> iv[KID_COUNT];
    for (const auto& r : s->prof.recs) {
        if (!r.a || !r.b) return fail(PT_ERR_HIP, "profiling event could not be created");
        HIP_TRY(hipEventSynchronize(r.b));
        float ms = 0.0f, t0 = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        HIP_TRY(hipEventElapsedTime(&t0, s->prof.recs.front().a, r.a));
        pt_kernel_time& k = acc[r.kid];
        k.min_ms = k.launches ? std::min(k.min_ms, (double)ms) : (double)ms;
        k.max_ms = k.launches ? std::max(k.max_ms, (double)ms) : (double)ms;
        k.total_ms += ms;
        k.launches++;
        iv[r.kid].emplace_back((double)t0, (double)t0 + (double)ms);
    }
    for (int k = 0; k < KID_COUNT; ++k) {
        std::sort(iv[k].begin(), iv[k].end());
        double busy = 0.0, lo = 0.0, hi = -1.0;
        for (const auto& x : iv[k]) {
            if (x.first > hi) {
                if (hi > lo) busy += hi - lo;
                lo = x.first;
                hi = x.second;
            } else {
                hi = std::max(hi, x.second);
            }
        }
        if (hi > lo) busy += hi - lo;
        acc[k].busy_ms = busy;
    }
    int n = 0;
    for (int k = 0; k < KID_COUNT; ++k) {
        if (!acc[k].launches) continue;
        if (n < max_entries) {
            out[n] = acc[k];
            std::snprintf(out[n].name, sizeof(out[n].name), "%s", kernel_name(k));
        }
        ++n;
    }
    *n_out = std::min(n, std::max(max_entries, 0));
    return PT_OK;
}

const char* pt_last_error(void) { return g_err.c_str(); }

int pt_set_hw_queues(int n) {
    if (n < 1 || n > 32) return fail(PT_ERR_INVALID, "hardware queue count must be in [1, 32]");
    if (g_hip_touched) return fail(PT_ERR_INVALID, "the HIP runtime is already running in this process");
    char v[16];
    std::snprintf(v, sizeof v, "%d", n);
    setenv("GPU_MAX_HW_QUEUES", v, 1);
    return PT_OK;
}

int pt_device_count(int* count_out) {
    if (!count_out) return fail(PT_ERR_INVALID, "count_out is NULL");
    g_hip_touched = true;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count_out = n;
    return PT_OK;
}

int pt_scene_create(const float* triangle_data, size_t triangle_len, const float* bvh_data, size_t bvh_len, int device,
                    pt_scene** scene_out) {
    if (!triangle_data || !bvh_data || !scene_out) return fail(PT_ERR_INVALID, "null argument");
    *scene_out = nullptr;
    g_hip_touched = true;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PT_ERR_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(PT_ERR_NODEVICE, "device ordinal out of range");
    const Opts o = opts_snapshot();
    LayoutOptions lo;
    lo.uid_reverse = o.is("mb_uid_order", "reverse");
    lo.leaf_bvh = o.num("leaf_bvh", lo.leaf_bvh);
    lo.leaf_skip = o.flag("leaf_skip", 1) != 0;
    HostLayout L;
    std::string err;
    const int rc = build_layout(triangle_data, triangle_len, bvh_data, bvh_len, lo, L, err);
    if (rc != PT_OK) return fail(rc, err);
    HIP_TRY(hipSetDevice(device));
    const ScenePlan plan = plan_sections(L, sizeof(Counters));
    pt_scene* s = new pt_scene();
    s->device = device;
    if (const int rc2 = s->d_mem.ensure(plan.total, "scene"); rc2 != PT_OK) { delete s; return rc2; }
    char* base = s->d_mem.p;
    for (const auto& sec : plan.sec)
        if (sec.bytes && hipMemcpy(base + sec.off, sec.src, sec.bytes, hipMemcpyHostToDevice) != hipSuccess) {
            pt_scene_destroy(s);
            return fail(PT_ERR_HIP, "scene upload failed");
        }
    // a section's device address (nullptr where the scene has none of it) and its offset from the nodes
    auto at = [&](Section k, bool have = true) -> const void* { return have ? base + plan.sec[k].off : nullptr; };
    auto off = [&](Section k) { return (uint32_t)plan.sec[k].off; };
    s->view.nodes = static_cast<const Node*>(at(SEC_NODES));
    s->view.tris = static_cast<const Tri*>(at(SEC_TRIS));
    s->view.mats = static_cast<const Material*>(at(SEC_MATS));
    s->view.lights = static_cast<const Light*>(at(SEC_LIGHTS));
    s->view.n_nodes = (int32_t)L.nodes.size();
    s->view.n_tris = (int32_t)L.tris.size();
    s->view.n_mats = (int32_t)L.mats.size();
    s->view.n_lights = L.ntri;
    s->view.f_ntri = (float)L.ntri;
    s->view.inv_ntri = 1.0f / (float)L.ntri;  // intersection-logic.wgsl:284
    s->view.max_stack = (int32_t)L.info.max_stack;
    s->view.fast_rcp = L.fast_rcp ? 1 : 0;
    s->view.node_bias = 0;  // per-pipeline default (launch_wavefront / launch_megakernel)
    s->view.node_steps = 0;  // per-pipeline default (launch_wavefront / launch_megakernel)
    s->view.off_tris = off(SEC_TRIS);
    s->view.off_mats = off(SEC_MATS);
    s->view.off_lights = off(SEC_LIGHTS);
    s->view.off_lmask = off(SEC_LMASK);
    s->view.lmask = static_cast<const uint64_t*>(at(SEC_LMASK));
    s->view.mailbox = L.mailbox ? 1 : 0;
    s->view.tnorm = static_cast<const float4*>(at(SEC_TNORM));
    s->view.vnormals = 0;
    s->view.lnodes = static_cast<const LNode*>(at(SEC_LNODES, !L.lnodes.empty()));
    s->view.ltris = static_cast<const Tri*>(at(SEC_LTRIS, !L.lnodes.empty()));
    s->view.pnodes = static_cast<const LNode*>(at(SEC_PNODES, !L.pnodes.empty()));
    s->view.ptris = static_cast<const Tri*>(at(SEC_PTRIS, !L.pnodes.empty()));
    s->view.pnorm = static_cast<const float4*>(at(SEC_PNORM, !L.pnodes.empty()));
    s->view.nalt = static_cast<const int4*>(at(SEC_NALT, !L.nalt.empty()));
    s->leaf_min = L.leaf_min;
    s->lleaves = L.lleaves;
    s->pre = L.pre;
    if (!L.pre.empty()) {
        s->h_nodes = L.nodes;
        s->h_tris = L.tris;
        s->h_lights.assign(L.lights.begin(), L.lights.begin() + std::min<size_t>(L.lights.size(), L.info.emissive_tris));
    }
    s->leaf_sizes = L.leaf_sizes;
    s->d_pre = static_cast<const PreLeaf*>(at(SEC_PRE, !L.pre.empty()));
    s->view.mb_base = L.mb_base;
    s->view.bfnode = static_cast<const BfNode*>(at(SEC_BFNODE, !L.bfnode.empty()));
    s->view.bfmap = static_cast<const int32_t*>(at(SEC_BFMAP, !L.bfmap.empty()));
    s->view.off_bfnode = off(SEC_BFNODE);
    s->view.off_bfmap = off(SEC_BFMAP);
    s->view.bfnarrow = static_cast<const BfNode*>(at(SEC_BFNARROW, !L.bfnarrow.empty()));
    s->view.off_bfnarrow = off(SEC_BFNARROW);
    s->view.span_bytes = (uint32_t)align_up(plan.span_end, 16);
    s->d_counters = reinterpret_cast<Counters*>(base + plan.off_counters);
    s->info = L.info;
    s->info.device_bytes = plan.total;
    *scene_out = s;
    return PT_OK;
}

void pt_scene_destroy(pt_scene* s) {
    if (!s) return;
    hipSetDevice(s->device);
    if (s->stream) { hipStreamSynchronize(s->stream); hipStreamDestroy(s->stream); }
    orphan_histories(s);
    for (int h = 0; h < kMaxParts; ++h) {
        if (s->ws.aux[h]) { hipStreamSynchronize(s->ws.aux[h]); hipStreamDestroy(s->ws.aux[h]); }
        if (s->ws.join[h]) hipEventDestroy(s->ws.join[h]);
    }
    if (s->ws.fork) hipEventDestroy(s->ws.fork);
    s->prof.destroy();
    delete s;  // the buffers free themselves, on the device set above
}

int pt_scene_set_vertex_normals(pt_scene* s, int enable) {
    if (!s) return fail(PT_ERR_INVALID, "null scene");
    s->view.vnormals = enable ? 1 : 0;
    return PT_OK;
}

int pt_scene_get_info(const pt_scene* s, pt_scene_info* out) {
    if (!s || !out) return fail(PT_ERR_INVALID, "null argument");
    *out = s->info;
    return PT_OK;
}

int pt_scene_check(pt_scene* s) {
    if (!s) return fail(PT_ERR_INVALID, "null scene");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());  // every render of the scene, on whatever stream, has finished
    return take_watchdog(s);
}

}  // extern "C"
