// pt_capi_render.hip — C ABI (include/pt_hip.h): the render entry points (whole image, window, moments,
// rectangle list, single frame, image), the display transform and the readback, with what every render
// shares: the frame parameters, the call's view of the scene and its pipeline, the wavefront's buffers,
// the watchdog.  Host code only.
#include <cmath>
#include <cstdio>
#include <algorithm>

#include "pt_capi_internal.h"

using namespace pt;

namespace pt {

// meta (program-raymarch.ts:79-92) -> FrameParams.  view_half_h uses the pinned tan
// (program-raymarch.wgsl:62); it is uniform, so it is evaluated once here.
// win: the window of the image the call renders (NULL: the whole image); row_pitch: pixels between
// rows of its destination (NULL: the window's width, a dense [h][w][3] buffer).
int make_params(const float* meta, int max_depth, FrameParams& fp, const pt_window* win, const size_t* pitch) {
    if (!meta) return fail(PT_ERR_INVALID, "meta is NULL");
    const float W = meta[0], H = meta[1];
    if (!(W >= 1.0f && H >= 1.0f && W <= 32768.0f && H <= 32768.0f) || W != std::floor(W) || H != std::floor(H))
        return fail(PT_ERR_INVALID, "meta[0..1] must be integral resolutions in [1, 32768]");
    if (max_depth < -1 || max_depth > 1024) return fail(PT_ERR_INVALID, "max_depth out of range");
    std::memset(&fp, 0, sizeof fp);
    fp.W = W; fp.H = H;
    fp.inv_w = meta[8]; fp.inv_h = meta[9];
    fp.aspect = meta[10];
    fp.focal = meta[2];
    fp.view_half_h = (2.0f * meta[2]) * tan_p(meta[3] * 0.5f);
    fp.rr_prob = meta[45];
    for (int i = 0; i < 4; ++i) fp.cam[i] = meta[4 + i];
    for (int i = 0; i < 16; ++i) fp.M[i] = meta[28 + i];
    fp.width = (uint32_t)W; fp.height = (uint32_t)H;
    fp.direct_only = meta[46] > 0.0f ? 1 : 0;
    fp.max_depth = max_depth < 0 ? 16 : max_depth;
    const pt_window whole = {0, 0, fp.width, fp.height};
    const pt_window& w = win ? *win : whole;
    if (w.w < 1 || w.h < 1) return fail(PT_ERR_INVALID, "window: w and h must be at least 1");
    if ((uint64_t)w.x0 + w.w > fp.width || (uint64_t)w.y0 + w.h > fp.height)
        return fail(PT_ERR_INVALID, "window: x0 + w and y0 + h must lie within the image (meta[0..1])");
    const size_t row_pitch = pitch ? *pitch : w.w;
    if (row_pitch < w.w) return fail(PT_ERR_INVALID, "row_pitch is smaller than the window's width");
    if (row_pitch > 0xffffffffull) return fail(PT_ERR_INVALID, "row_pitch out of range");
    fp.win_x0 = w.x0; fp.win_y0 = w.y0; fp.win_w = w.w; fp.win_h = w.h;
    fp.row_pitch = (uint32_t)row_pitch;
    return PT_OK;
}

int check_frames(uint32_t frame0, uint32_t nframes, uint32_t stride) {
    if ((uint64_t)frame0 + (uint64_t)(nframes ? nframes - 1 : 0) * stride >= (1ull << 24))
        return fail(PT_ERR_INVALID, "frame index >= 2^24 (t_k = u32(f32(k)) would round)");
    return PT_OK;
}

// a list render's list as the caller gave it: there, and not empty
static int check_rects(const pt_window* rects, size_t n) {
    if (!rects || !n) return fail(PT_ERR_INVALID, n ? "rects is NULL" : "rects: the list is empty (n must be at least 1)");
    return PT_OK;
}

// the probe of the pre-resolvable leaves (probe_pre_leaves): a 32 x 32 raster (<= 4 Ki queries), at
// most 2^23 triangle tests (MedievalBoat: ~4 k per query, ~30 ms)
constexpr int kPreProbeGrid = 32;
constexpr uint64_t kPreProbeTests = 1ull << 23;

// PT_MODE_* -> pipeline.  A/B overrides (pt_set_option): kernel=literal|mega|wavefront, lds=0|1,
// trav=nested|flat1|pred|lean|lean2|lean4|lean8|lean16|lean32, fastrcp=0|1, ...
// AUTO picks the wavefront pipeline once a call has this many paths: below it the fixed
// cost of its ~2(D+1) launches per batch outweighs its better SIMD utilisation.  Measured per
// scene type (round 2, depth 16, ms megakernel / wavefront): mailbox scenes (the fused kernel)
// gain at every size (CornellBox 128^2 x 1: 1.43 / 0.66), so do scenes with cooperative big
// leaves (MedievalBoat 256^2 x 1: 62 / 35); other scenes from about 2^19 paths (Glossy 512^2 x 1:
// 7.1 / 9.1, 512^2 x 2: 13.1 / 9.6).
constexpr uint64_t kWfAutoMinPaths = 1ull << 19;
// The call's pipeline: option kernel, else the mode, AUTO by the call's paths and the scene (view's
// mailbox and big_leaf > 0)
static bool wants_wavefront(const Opts& o, int mode, uint64_t paths, const SceneView& view) {
    if (o.is("kernel", "wavefront")) return true;
    if (o.is("kernel", "mega") || o.is("kernel", "literal")) return false;
    const uint64_t auto_min = (view.mailbox || view.big_leaf > 0) ? 1 : kWfAutoMinPaths;
    return mode == PT_MODE_WAVEFRONT || (mode == PT_MODE_AUTO && paths >= auto_min);
}

// The call's LaunchOpts: pt_flavour.h's defaults, the pipeline, and whatever pt_set_option overrides
LaunchOpts launch_opts(const Opts& o, int mode, uint64_t paths, const SceneView& view) {
    LaunchOpts lo;
    lo.wavefront = wants_wavefront(o, mode, paths, view);
    lo.literal = o.is("kernel", "literal");
    auto flag = [&](const char* name, bool def) { return o.flag(name, def ? 1 : 0) != 0; };
    lo.lds = flag("lds", lo.lds);
    lo.fuse_gen = flag("fuse_gen", lo.fuse_gen);
    lo.dual = flag("dual", lo.dual);
    lo.region_perm = flag("region_perm", lo.region_perm);
    if (const long p = o.num("parts", 0); p > 0) lo.parts = (int)p;  // 0: the default
    lo.sort = (int)o.num("sort", lo.sort);  // 1 / 8: direction octant; 64: + origin octant; 512: + 4^3 origin cells
    lo.trace_sparse = (int)o.num("trace_sparse", lo.trace_sparse);
    lo.regen = (int)std::max(0L, std::min(1L << 20, o.num("regen", lo.regen)));
    lo.trace_ring = (int)o.num("trace_ring", lo.trace_ring);
    lo.trace_blocks = (int)o.num("wf_trace_blocks", lo.trace_blocks);
    lo.watchdog = (uint32_t)o.num("trace_watchdog", lo.watchdog);
    lo.bf_slots = (int)o.num("bf_slots", lo.bf_slots);
    lo.step_addr64 = flag("step_addr64", lo.step_addr64);
    lo.leaf_blocks = (int)o.num("leaf_blocks", lo.leaf_blocks);
    // | 4: the pair walk's second check of the open chunks with the entries' own normals (option
    // leaf_refine, default on; pt_leafpass.hip)
    lo.leaf_pairs = (int)std::max(0L, std::min(2L, o.num("leaf_pairs", 1))) | (flag("leaf_refine", true) ? 4 : 0);
    const int trav = opt_choice("trav", o.get("trav").c_str());  // the TravBase, in the option's order; -1: the default
    lo.set_flavour_opts(trav, o.flag("fastrcp", -1), o.flag("mailbox", -1), o.flag("bf", -1), o.flag("fuse", -1));
    return lo;
}

// kWfTargetPaths, the paths in flight per wavefront batch: pt_wf_plan.h
constexpr int kBigLeafDefault = 128;
constexpr long kPreRatioDefault = 50;  // shape_view: the leaf pass when >= 50 % of its work is visited

// the radiance of a batch's paths
static int ensure_rad(pt_scene* s, uint64_t paths) {
    const int rc = s->d_rad.ensure_idle(3 * paths, "wavefront radiance");
    s->wf.rad = s->d_rad.p;
    s->wf.rad_cap = s->d_rad.cap / 3;
    return rc;
}

// keys of the pre-resolved big leaves: npre per queue entry of the wavefront buffers
static int ensure_pres(pt_scene* s, int npre) {
    const int rc = s->d_pres.ensure_idle((size_t)npre * s->wf.qcap, "pre-resolved leaf keys");
    s->wf.pres = s->d_pres.p;
    s->wf.pres_stride = s->wf.qcap;
    return rc;
}

static int ensure_wavefront(pt_scene* s, uint64_t paths) {
    if (s->d_wf.p && s->wf.capacity >= paths) return PT_OK;
    if (paths > 0x7fffffffull) return fail(PT_ERR_INVALID, "image too large for one wavefront batch");
    s->wf.capacity = 0;  // until the buffers below stand
    const size_t n = paths;
    const size_t qn = wf_queue_entries(n);  // with the region layout's slack (pt_wf_plan.h)
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    size_t oq[6];
    for (int k = 0; k < 6; ++k) oq[k] = take((k % 3 == 0 ? 32 : 16) * qn);
    const size_t o_p0 = take(16 * qn), o_p1 = take(16 * qn), o_p2 = take(8 * qn), o_hit = take(8 * qn),
                 o_ctl = take(4 * kMaxParts * WF_CTL_WORDS), o_rcnt = take(4 * kMaxParts * 3 * kRegions),
                 o_cam = take(2 * 64 * sizeof(float4));
    PT_TRY(s->d_wf.ensure_idle(off, "wavefront state"));
    char* b = s->d_wf.p;
    auto f4 = [&](size_t o) { return reinterpret_cast<float4*>(b + o); };
    WfBuffers& w = s->wf;
    w.ext = WfQueue{f4(oq[0]), f4(oq[1]), f4(oq[2])};
    w.shd = WfQueue{f4(oq[3]), f4(oq[4]), f4(oq[5])};
    w.sp0 = f4(o_p0); w.sp1 = f4(o_p1);
    w.sp2 = reinterpret_cast<float2*>(b + o_p2);
    w.hitq = reinterpret_cast<int2*>(b + o_hit);
    w.ctl = reinterpret_cast<uint32_t*>(b + o_ctl);
    w.rcnt = reinterpret_cast<uint32_t*>(b + o_rcnt);
    w.camtab = f4(o_cam);
    if (hipMemset(w.ctl, 0, 4 * kMaxParts * WF_CTL_WORDS) != hipSuccess ||
        hipMemset(w.rcnt, 0, 4 * kMaxParts * 3 * kRegions) != hipSuccess)
        return fail(PT_ERR_HIP, "hipMemset wavefront control words");
    if (!s->ws.aux[0]) {
        bool ok = hipEventCreateWithFlags(&s->ws.fork, hipEventDisableTiming) == hipSuccess;
        for (int h = 0; h < kMaxParts && ok; ++h)
            ok = hipStreamCreateWithFlags(&s->ws.aux[h], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&s->ws.join[h], hipEventDisableTiming) == hipSuccess;
        if (!ok) return fail(PT_ERR_HIP, "creating the wavefront's streams");
    }
    PT_TRY(s->h_ctl.ensure(kMaxParts * WF_CTL_WORDS, "wavefront control mirror"));
    w.capacity = (uint32_t)n;
    w.qcap = (uint32_t)qn;
    w.rq = w.rqi = 1;
    w.rad = s->d_rad.p;
    w.rad_cap = s->d_rad.cap / 3;
    return PT_OK;
}

// A trace wave that hit its watchdog (k_wf_trace: kTraceWatchdog iterations or
// kTraceWatchdogTicks) sets ctl[WF_WATCHDOG] and leaves its state in ctl[WF_SNAP..]; later
// launches of the scene skip their work.  The pinned mirror h_ctl receives the control words
// after every wavefront render on its stream; once that copy has landed (the caller synchronised,
// or the blocking calls' own synchronisation) the flag is reported here — by whichever call of
// the scene comes next, megakernel or wavefront — and cleared.  The failure path waits for the
// device first, so no mirror copy still in flight can bring the flag back after the clear and
// report the same failure twice.
// The same for a query wave (pt_query.hip k_query): the flag is the first of the scene's query control
// words, mirrored in h_qctl after every query launch.
static int take_query_watchdog(pt_scene* s) {
    if (!s->h_qctl.p || !__atomic_load_n(&s->h_qctl.p[0], __ATOMIC_ACQUIRE)) return PT_OK;
    HIP_TRY(hipDeviceSynchronize());  // every pending mirror copy of the scene has landed
    uint32_t v[kQueryCtlWords];
    std::memcpy(v, s->h_qctl.p, sizeof v);
    HIP_TRY(hipMemset(s->d_qctl.p, 0, sizeof v));
    std::memset(s->h_qctl.p, 0, sizeof v);
    char msg[256];
    std::snprintf(msg, sizeof(msg),
                  "ray query gave up after its watchdog limit (results invalid); first wave: n=%u nwaves=%u w=%u "
                  "fetched=%u base=%u wv=%u cur=%u in_flight=%u",
                  v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]);
    return fail(PT_ERR_HIP, msg);
}

int take_watchdog(pt_scene* s) {
    if (const int rc = take_query_watchdog(s); rc != PT_OK) return rc;
    uint32_t* const h_ctl = s->h_ctl.p;
    if (!h_ctl) return PT_OK;
    int h = 0;
    while (h < kMaxParts && !__atomic_load_n(&h_ctl[h * WF_CTL_WORDS + WF_WATCHDOG], __ATOMIC_ACQUIRE)) ++h;
    if (h == kMaxParts) return PT_OK;
    HIP_TRY(hipDeviceSynchronize());  // every pending mirror copy of the scene has landed
    uint32_t v[WF_SNAP_WORDS];
    std::memcpy(v, h_ctl + h * WF_CTL_WORDS + WF_SNAP, sizeof v);
    for (int k = 0; k < kMaxParts; ++k)
        HIP_TRY(hipMemset(s->wf.ctl + k * WF_CTL_WORDS + WF_WATCHDOG, 0,
                          (WF_SNAP + WF_SNAP_WORDS - WF_WATCHDOG) * sizeof(uint32_t)));
    std::memset(h_ctl, 0, 4 * kMaxParts * WF_CTL_WORDS);
    char msg[360];
    std::snprintf(msg, sizeof(msg),
                  "wavefront trace gave up after its watchdog limit (result invalid); first wave: count=%u "
                  "nwaves=%u w=%u jl=%u wv=%u nv=%u cur=%u flushed=%u in_flight=%u mask=%08x%08x queue=%u",
                  v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[10], v[9], v[11]);
    return fail(PT_ERR_HIP, msg);
}

// The scene as this call's kernels see it: the scene's view with the per-call choices applied — the
// big-leaf threshold, leaf chunks, the pooled runs' length, leaf remainders, and whether the big
// leaves are resolved before the traversal (for the camera of fp).  paths: the call's, for AUTO's
// choice of pipeline.
int shape_view(pt_scene* s, const Opts& o, const FrameParams& fp, int mode, uint64_t paths, SceneView& view) {
    view = s->view;
    if (o.has("node_bias")) view.node_bias = std::max(1L, o.num("node_bias", 1));  // A/B runs
    if (o.has("node_steps")) view.node_steps = (int32_t)std::max(1L, std::min(8L, o.num("node_steps", 1)));
    // big leaves (lean traversal): a ray reaching a leaf of >= big_leaf entries has it tested by the
    // whole wave (pt_device.h big_turn); default 128 (MedievalBoat 2.3x, in-process A/B; 64 is 1.5 %
    // faster there but 12 % slower on the 1M-triangle synthetic scene, whose many 64..127-entry
    // leaves waste half a cooperative step each); option big_leaf=n sets it, 0 turns big-leaf
    // turns and leaf chunks off
    {
        const long big = o.num("big_leaf", kBigLeafDefault);
        view.big_leaf = (big > 0 && s->info.max_leaf >= (uint32_t)big) ? (int32_t)big : 0;
        // leaf BVHs (built at pt_scene_create, option leaf_bvh): lanes park at every leaf that has
        // chunks and test them chunk by chunk (chunk_turn_multi); option leaf_walk=0 keeps them out (A/B)
        if (big > 0 && s->leaf_min > 0 && o.flag("leaf_walk", 1) != 0)
            view.big_leaf = view.big_leaf > 0 ? std::min<int32_t>(view.big_leaf, s->leaf_min) : s->leaf_min;
        else
            view.lnodes = nullptr;
    }
    // pooled leaf turns (pt_device.h lean_leaf_pool) on every tree (option leaf_pool=0: each lane
    // walks its own pairs).  The run length: 2 on trees of short leaves (< 16 entries: the SAH
    // builder's; Glossy +2.9 %, the boat +16.5 %, 100k +26 %, 1M +29 % over unpooled:
    // profiles/r04am_sah_pool.log — runs of 4 there cost Glossy 3.6 %, r04t_configs.jsonl) and
    // where the leaves reference >= 32 Ki triangles and no leaf is big (100k +12 %, 1M +26 % against
    // runs of 4: r04aa_ab_run.log; 12.5k +3.7 % with node bias 1-2: r04ak_run2_bias.log), else 4
    // (Glossy 5 Ki references, 1k, and the boat — 52 Ki references, but big leaves walked in
    // chunks — are 1-2 % faster with 4); option pool_run=2|4.  Round 6, with four node steps per node
    // turn: runs of 2 on every tree without big leaves (Glossy +5 %, 1k +2.2 %, 12.5k +0.8 % over 4;
    // the boat, whose big leaves go to the leaf pass, -0.7 %: profiles/r06ac_ab_*.log)
    {
        const bool pool = o.flag("leaf_pool", 1) != 0;
        const bool run2 = s->info.max_leaf < 16 || view.big_leaf == 0;
        const long run = o.num("pool_run", run2 ? 2 : 4);
        view.leaf_pool = pool ? (int32_t)run : 0;
    }
    // leaf remainders (pt_device.h lean_node_unit): option leaf_skip=0 keeps them out (A/B); a big-leaf
    // threshold below kLeafSkipMaxLeaf too (a leaf the cooperative turns or the leaf pass take by its
    // first record must keep it)
    if (o.flag("leaf_skip", 1) == 0 || (view.big_leaf > 0 && view.big_leaf < kLeafSkipMaxLeaf)) view.nalt = nullptr;
    // the brute-force replay walks the BfNode tree without a stack (bf_stackless=0: the stack walk; A/B)
    if (o.flag("bf_stackless", 1) == 0) view.bfnode = nullptr;
    // ... and its 32-bit instance where the scene has the narrow payload (bf_narrow=0: the 64-bit one; tests)
    if (o.flag("bf_narrow", 1) == 0 || !view.bfnode) view.bfnarrow = nullptr;
    // big leaves resolved before the traversal (k_wf_leafpass, pt_leafpass.hip; option leaf_pre=0:
    // the cooperative turns and chunk walks inside k_wf_trace): the leaves of >= big_leaf entries, at
    // most kMaxPre of them — with more, the threshold rises above the (kMaxPre + 1)-th largest and
    // the rest are ordinary leaves of the pooled turns
    // The leaf pass resolves a leaf for every ray that passes its box filter; the traversal tests it
    // only for the rays that reach it, and a ray whose closest hit so far is nearer than a box on the
    // leaf's path never does.  Where the filter over-predicts — the boat of CornellBox2's all-meshes
    // scene sits inside the box's walls: 0.33 of the filtered leaf work is visited, 65 against 91.6
    // Msamples/s without the pass (profiles/r05d_auto_ab.log) — the pass costs more than it saves;
    // the boat alone visits 0.99 of it (+30 %).  The choice (option leaf_pre absent or 2) follows the
    // scene's probe (pt_scene::pre_probe, pt_leafbvh.h probe_pre_leaves; CornellBox2 all meshes 0.38,
    // the boat 1.00): the pass when the visited entries are at least pre_ratio % (default
    // kPreRatioDefault) of the filtered ones, each leaf weighted by its entries.  leaf_pre=1 always,
    // 0 never.  (The choice changes the kernels, not the image: both paths are exact.)
    view.npre = 0;
    view.pre = nullptr;
    const long pre_opt = o.num("leaf_pre", 2);
    if (wants_wavefront(o, mode, paths, view) && view.big_leaf > 0 && pre_opt != 0 && !s->pre.empty()) {
        int32_t T = view.big_leaf;
        if (s->leaf_sizes.size() > (size_t)kMaxPre && s->leaf_sizes[kMaxPre] >= T) T = s->leaf_sizes[kMaxPre] + 1;
        int np = 0;
        while (np < (int)s->pre.size() && s->pre[(size_t)np].n >= T) ++np;
        // more big leaves than the table holds: the pass would raise the threshold to T and the big
        // leaves left out (big_leaf <= n < T) would lose their chunk walks and cooperative turns, a
        // cost the probe below does not weigh — AUTO keeps the traversal's own big-leaf machinery then
        // (advisor r05; leaf_pre=1 still forces the pass)
        if (pre_opt != 1 && T > view.big_leaf) np = 0;
        if (np > 0 && pre_opt != 1) {
            std::lock_guard<std::mutex> lk(s->pre_mu);  // held for the probe and for the reading of its result
            ProbeCamera pc{};
            for (int c = 0; c < 3; ++c) pc.cam[c] = fp.cam[c];
            for (int c = 0; c < 16; ++c) pc.M[c] = fp.M[c];
            pc.focal = fp.focal;
            pc.half_h = fp.view_half_h;
            pc.half_w = fp.view_half_h * fp.aspect;
            // probed once per camera: a render whose camera differs from the probe's probes again
            // (advisor r05: the choice is the camera's; both paths give the same bits)
            if (!s->pre_probed || std::memcmp(&pc, &s->pre_cam, sizeof pc) != 0) {
                probe_pre_leaves(s->h_nodes, s->h_tris, s->h_lights, s->pre, pc, kPreProbeGrid, kPreProbeTests,
                                 s->pre_probe);
                s->pre_cam = pc;
                s->pre_probed = true;
            }
            if (s->pre_probe.size() >= (size_t)np) {
                double filt = 0.0, vis = 0.0;
                for (int b = 0; b < np; ++b) {
                    filt += (double)s->pre_probe[(size_t)b][0] * s->pre[(size_t)b].n;
                    vis += (double)s->pre_probe[(size_t)b][1] * s->pre[(size_t)b].n;
                }
                if (filt > 0.0 && vis * 100.0 < filt * (double)o.num("pre_ratio", kPreRatioDefault)) np = 0;
            }
        }
        if (np > 0) {
            // pt_device.h pre_slot finds a leaf's key slot by its first record among the first np table
            // entries, and answers slot 0 for any other: every leaf of >= T entries must be among them
            // (the table is the kMaxPre largest, and T was raised above the (kMaxPre + 1)-th; advisor r05)
            for (size_t k = (size_t)np; k < s->pre.size(); ++k)
                if (s->pre[k].n >= T) return fail(PT_ERR_SCENE, "internal: a leaf of >= big_leaf entries outside the pre-resolved table");
            if (s->leaf_sizes.size() > (size_t)np && s->leaf_sizes[(size_t)np] >= T)
                return fail(PT_ERR_SCENE, "internal: more leaves of >= big_leaf entries than the pre-resolved table holds");
            view.big_leaf = T;
            view.npre = np;
            view.pre = s->d_pre;
            for (int b = 0; b < kMaxPre; ++b) view.pre_rec0[b] = b < np ? s->pre[(size_t)b].rec0 : -1;
        }
    }
    // a remainder stands for its leaf by another first record and count: the leaves the cooperative
    // turns or the leaf pass take (>= big_leaf entries) must have none (every remainder's leaf has
    // fewer than kLeafSkipMaxLeaf entries)
    if (view.nalt != nullptr && view.big_leaf > 0 && view.big_leaf < kLeafSkipMaxLeaf)
        return fail(PT_ERR_SCENE, "internal: leaf remainders with a big-leaf threshold below their largest leaf");
    return PT_OK;
}

// The device table of a list render in the scene's scratch, uploaded on the call's stream: the rows and,
// for the megakernel, its blocks.  The host copies are pageable, so the runtime has read them when
// hipMemcpyAsync returns; the device copy is ordered with the call's launches on its stream.
static int upload_rects(pt_scene* s, const RectPlan& plan, const FrameParams& fp, bool blocks, hipStream_t stream, RectList& rl) {
    const size_t row_bytes = align_up(plan.rows.size() * sizeof(RectRow), 256);
    std::vector<RectBlock> hb;
    if (blocks) {
        if (plan.nblocks > 0x7fffffffull) return fail(PT_ERR_INVALID, "rects: too many 16x16 blocks for one megakernel grid");
        plan_blocks(plan, hb);
    }
    const int rc = s->d_rects.ensure(row_bytes + hb.size() * sizeof(RectBlock), "rectangle table");
    if (rc != PT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_rects.p, plan.rows.data(), plan.rows.size() * sizeof(RectRow), hipMemcpyHostToDevice, stream));
    if (!hb.empty())
        HIP_TRY(hipMemcpyAsync(s->d_rects.p + row_bytes, hb.data(), hb.size() * sizeof(RectBlock), hipMemcpyHostToDevice, stream));
    rl.rows = reinterpret_cast<const RectRow*>(s->d_rects.p);
    rl.blocks = hb.empty() ? nullptr : reinterpret_cast<const RectBlock*>(s->d_rects.p + row_bytes);
    rl.n = (uint32_t)plan.rows.size();
    rl.npix = (uint32_t)plan.npix;
    rl.nblocks = (uint32_t)hb.size();
    rl.fx0 = fp.win_x0;
    rl.fy0 = fp.win_y0;
    return PT_OK;
}

// The wavefront's buffers for a call of nframes frames of npix paths each (a single-frame call: 1): the
// queues and the radiance of one batch, and the keys of the view's pre-resolved leaves
int prepare_wavefront(pt_scene* s, const Opts& o, const SceneView& view, uint64_t npix, uint32_t nframes) {
    // the batch: option wf_paths or the default target in whole pairs of frames, at least two frames,
    // one frame of room more for an odd count (wf_batch_size, pt_wf_plan.h)
    const WfBatchSize bs = wf_batch_size(npix, nframes, o.num("wf_paths", (long)kWfTargetPaths), o.has("wf_paths"));
    int rc2 = ensure_wavefront(s, bs.want);
    // the batch's state (~188 B/path: 12 GB at the 64 M-path target) may not fit beside other
    // allocations: halve it down to one frame per batch before giving up
    for (uint64_t w = bs.want; rc2 == PT_ERR_NOMEM && w > bs.floor;)
        rc2 = ensure_wavefront(s, w = std::max<uint64_t>(w / 2, bs.floor));
    if (rc2 != PT_OK) return rc2;
    rc2 = ensure_rad(s, s->wf.capacity);
    if (rc2 != PT_OK) return rc2;
    if (view.npre > 0) {
        if ((rc2 = ensure_pres(s, view.npre)) != PT_OK) return rc2;
    } else {
        s->wf.pres = nullptr;
    }
    return PT_OK;
}

// d_out: the window's first pixel, rows row_pitch pixels apart (win NULL: the whole image); d_m2
// (nullable, accumulating calls): the second moments, laid out like d_out.  rects (nullable,
// accumulating calls): the call renders these nrects rectangles of the window instead of all of it
// (pt_render_rects: win is its frame) — "paths per frame" is then the list's pixels everywhere below
int render_impl(pt_scene* s, const float* meta, uint32_t frame0, uint32_t nframes, uint32_t stride, int max_depth,
                int mode, bool accum, float* d_out, Counters* d_cnt, hipStream_t stream, const pt_window* win,
                const size_t* pitch, float* d_m2, const pt_window* rects, size_t nrects) {
    FrameParams fp{};
    int rc = make_params(meta, max_depth, fp, win, pitch);
    if (rc != PT_OK) return rc;
    RectPlan plan;
    const bool list = rects != nullptr || nrects != 0;
    if (list) {
        std::string err;
        if ((rc = plan_rects(win, fp.width, fp.height, rects, nrects, plan, err)) != PT_OK) return fail(rc, err);
    }
    if (mode != PT_MODE_AUTO && mode != PT_MODE_MEGAKERNEL && mode != PT_MODE_WAVEFRONT)
        return fail(PT_ERR_INVALID, "unknown mode");
    if (accum) PT_TRY(check_frames(frame0, nframes, stride));
    HIP_TRY(hipSetDevice(s->device));
    if (nframes == 0) return PT_OK;
    const uint64_t npix = list ? plan.npix : (uint64_t)fp.win_w * fp.win_h;  // paths per frame: the list's or the window's
    ProfScope prof_scope(s);
    const Opts o = opts_snapshot();
    // a lens camera (pt_scene_set_camera): the wavefront pipeline with camera paths from the generate
    // kernel, whatever the mode and the options kernel, fuse_gen and regen say — as a ray list's
    // (pt_query_radiance); nothing else of the call changes
    LensCam lens;
    const LensCam* const cam = scene_camera(s, lens);
    if (cam) mode = PT_MODE_WAVEFRONT;
    WfCall c;
    if ((rc = c.open(s, o, fp, mode, npix, accum ? nframes : 1)) != PT_OK) return rc;
    if (cam) {
        c.lo.wavefront = true;
        c.lo.literal = false;
    }
    RectList rl{};
    if (list && (rc = upload_rects(s, plan, fp, !c.lo.wavefront, stream, rl)) != PT_OK) return rc;
    if (c.lo.wavefront)
        return c.run(s, o, fp, list ? PathSource(rl, cam, d_m2) : PathSource(cam, d_m2), frame0, stride, accum,
                     d_out, d_cnt, stream);
    HIP_TRY(launch_megakernel(c.lo, c.view, fp, frame0, nframes, stride, accum, d_cnt != nullptr, d_out, d_cnt, stream, d_m2,
                              list ? &rl : nullptr));
    return PT_OK;
}

int WfCall::open(pt_scene* s, const Opts& o, const FrameParams& fp, int mode, uint64_t paths_per_frame, uint32_t frames) {
    npix = paths_per_frame;
    nframes = frames;
    PT_TRY(shape_view(s, o, fp, mode, npix * nframes, view));
    lo = launch_opts(o, mode, npix * nframes, view);
    return take_watchdog(s);
}

int WfCall::run(pt_scene* s, const Opts& o, const FrameParams& fp, const PathSource& src, uint32_t frame0, uint32_t stride,
                bool accum, float* d_out, Counters* d_cnt, hipStream_t stream) const {
    PT_TRY(prepare_wavefront(s, o, view, npix, nframes));
    HIP_TRY(launch_wavefront(lo, view, fp, s->wf, src, frame0, nframes, stride, accum, d_cnt != nullptr, d_out, d_cnt, stream,
                             s->ws));
    HIP_TRY(hipMemcpyAsync(s->h_ctl.p, s->wf.ctl, 4 * kMaxParts * WF_CTL_WORDS, hipMemcpyDeviceToHost, stream));
    return PT_OK;
}

int query_call(pt_scene* s, const PathSource& src, size_t n, uint32_t sample0, uint32_t nsamples, float rr_prob,
               int32_t direct_only, int32_t max_depth, float* d_accum, Counters* d_cnt, hipStream_t stream) {
    HIP_TRY(hipSetDevice(s->device));
    ProfScope prof_scope(s);
    Opts o = opts_snapshot();
    o.v[opt_index("kernel")] = "wavefront";
    if (o.num("leaf_pre", 2) != 1) o.v[opt_index("leaf_pre")] = "0";
    FrameParams fp{};
    fp.rr_prob = rr_prob;
    fp.direct_only = direct_only != 0 ? 1 : 0;
    fp.max_depth = max_depth;
    fp.width = fp.win_w = fp.row_pitch = (uint32_t)n;
    fp.height = fp.win_h = 1;
    WfCall c;
    PT_TRY(c.open(s, o, fp, PT_MODE_WAVEFRONT, n, nsamples));
    return c.run(s, o, fp, src, sample0, 1, true, d_accum, d_cnt, stream);
}

}  // namespace pt

extern "C" {

int pt_render_window_async(pt_scene* s, const float meta[48], const pt_window* win, uint32_t frame0, uint32_t nframes,
                           uint32_t frame_stride, int max_depth, int mode, float* d_accum, size_t row_pitch,
                           pt_counters* d_counters, void* stream) {
    if (!s || !d_accum || !meta) return fail(PT_ERR_INVALID, "null argument");
    return render_impl(s, meta, frame0, nframes, frame_stride, max_depth, mode, true, d_accum,
                       reinterpret_cast<Counters*>(d_counters), static_cast<hipStream_t>(stream), win, &row_pitch);
}

int pt_render_async(pt_scene* s, const float meta[48], uint32_t frame0, uint32_t nframes, uint32_t frame_stride,
                    int max_depth, int mode, float* d_accum, pt_counters* d_counters, void* stream) {
    if (!s || !d_accum) return fail(PT_ERR_INVALID, "null argument");
    return render_impl(s, meta, frame0, nframes, frame_stride, max_depth, mode, true, d_accum,
                       reinterpret_cast<Counters*>(d_counters), static_cast<hipStream_t>(stream));
}

// The blocking render calls' body: the window's accumulators from the host (pt_render_image: zeroed;
// a frame, accumulate false: neither), the render, the results back to the host — accum, or rgba
// (nullable: the tone-mapped image instead), m2 and counters (nullable) — one synchronisation, and
// the watchdog (a trace wave that hit kTraceWatchdog left a flag, cleared here).
// rects (nullable): a list render of the window (pt_render_rects: win is its frame) — the list is
// checked before anything is copied, so a rejected call leaves the host buffers alone.
static int render_blocking(pt_scene* s, const float* meta, const pt_window* win, uint32_t frame0, uint32_t nframes,
                           uint32_t stride, int max_depth, int mode, bool accumulate, float* accum, float* m2,
                           uint8_t* rgba, pt_counters* counters, const pt_window* rects = nullptr, size_t nrects = 0) {
    FrameParams fp{};
    PT_TRY(make_params(meta, max_depth, fp, win));
    if (rects != nullptr || nrects != 0) {  // planned and checked here, before anything is copied
        RectPlan plan;
        std::string err;
        if (const int rc = plan_rects(win, fp.width, fp.height, rects, nrects, plan, err); rc != PT_OK) return fail(rc, err);
    }
    const size_t npix = (size_t)fp.win_w * fp.win_h, n = 3 * npix, bytes = n * sizeof(float);
    Blocking b(s, counters);
    PT_TRY(b.device());
    PT_TRY(s->d_accum.ensure(n, "accumulator"));
    if (m2) PT_TRY(s->d_m2.ensure(n, "second moments"));
    PT_TRY(b.open());
    if (rgba) PT_TRY(s->d_rgba.ensure(4 * npix, "image"));
    // the accumulator: zero for an image, the caller's when accumulating, neither for a single frame
    if (rgba) PT_TRY(b.zero(s->d_accum.p, bytes));
    else if (accumulate) PT_TRY(b.in(s->d_accum.p, accum, bytes));
    if (m2) PT_TRY(b.in(s->d_m2.p, m2, bytes));
    PT_TRY(render_impl(s, meta, frame0, nframes, stride, max_depth, mode, accumulate, s->d_accum.p, b.d_cnt(), s->stream, win,
                       nullptr, m2 ? s->d_m2.p : nullptr, rects, nrects));
    if (rgba) {
        PT_TRY(pt_tonemap_async(s, s->d_accum.p, npix, nframes, s->d_rgba.p, s->stream));
        PT_TRY(b.out(rgba, s->d_rgba.p, 4 * npix));
    } else {
        PT_TRY(b.out(accum, s->d_accum.p, bytes));
    }
    if (m2) PT_TRY(b.out(m2, s->d_m2.p, bytes));
    return b.finish(Blocking::kWatchdog);
}

int pt_render(pt_scene* s, const float meta[48], uint32_t frame0, uint32_t nframes, uint32_t frame_stride,
              int max_depth, int mode, float* accum, pt_counters* counters) {
    return pt_render_window(s, meta, nullptr, frame0, nframes, frame_stride, max_depth, mode, accum, counters);
}

int pt_render_window(pt_scene* s, const float meta[48], const pt_window* win, uint32_t frame0, uint32_t nframes,
                     uint32_t frame_stride, int max_depth, int mode, float* accum, pt_counters* counters) {
    if (!s || !accum || !meta) return fail(PT_ERR_INVALID, "null argument");
    return render_blocking(s, meta, win, frame0, nframes, frame_stride, max_depth, mode, true, accum, nullptr, nullptr, counters);
}

int pt_render_moments_async(pt_scene* s, const float meta[48], const pt_window* win, uint32_t frame0, uint32_t nframes,
                            uint32_t frame_stride, int max_depth, int mode, float* d_accum, float* d_m2,
                            size_t row_pitch, pt_counters* d_counters, void* stream) {
    if (!s || !d_accum || !d_m2 || !meta) return fail(PT_ERR_INVALID, "null argument");
    return render_impl(s, meta, frame0, nframes, frame_stride, max_depth, mode, true, d_accum,
                       reinterpret_cast<Counters*>(d_counters), static_cast<hipStream_t>(stream), win, &row_pitch, d_m2);
}

int pt_render_moments(pt_scene* s, const float meta[48], const pt_window* win, uint32_t frame0, uint32_t nframes,
                      uint32_t frame_stride, int max_depth, int mode, float* accum, float* m2, pt_counters* counters) {
    if (!s || !accum || !m2 || !meta) return fail(PT_ERR_INVALID, "null argument");
    return render_blocking(s, meta, win, frame0, nframes, frame_stride, max_depth, mode, true, accum, m2, nullptr, counters);
}

int pt_render_rects_async(pt_scene* s, const float meta[48], const pt_window* frame, const pt_window* rects, size_t n,
                          uint32_t frame0, uint32_t nframes, uint32_t frame_stride, int max_depth, int mode, float* d_accum,
                          float* d_m2, size_t row_pitch, pt_counters* d_counters, void* stream) {
    if (!s || !d_accum || !meta) return fail(PT_ERR_INVALID, "null argument");
    PT_TRY(check_rects(rects, n));
    return render_impl(s, meta, frame0, nframes, frame_stride, max_depth, mode, true, d_accum,
                       reinterpret_cast<Counters*>(d_counters), static_cast<hipStream_t>(stream), frame, &row_pitch, d_m2,
                       rects, n);
}

int pt_render_rects(pt_scene* s, const float meta[48], const pt_window* frame, const pt_window* rects, size_t n,
                    uint32_t frame0, uint32_t nframes, uint32_t frame_stride, int max_depth, int mode, float* accum,
                    float* m2, pt_counters* counters) {
    if (!s || !accum || !meta) return fail(PT_ERR_INVALID, "null argument");
    PT_TRY(check_rects(rects, n));
    return render_blocking(s, meta, frame, frame0, nframes, frame_stride, max_depth, mode, true, accum, m2, nullptr, counters,
                           rects, n);
}

int pt_selftest_rect_plan(const pt_window* frame, uint32_t W, uint32_t H, const pt_window* rects, size_t n,
                          uint64_t* first_out, uint64_t* npix_out) {
    RectPlan plan;
    std::string err;
    const int rc = plan_rects(frame, W, H, rects, n, plan, err);
    if (rc != PT_OK) return fail(rc, err);
    for (size_t k = 0; first_out && k < n; ++k) first_out[k] = plan.rows[k].first;
    if (npix_out) *npix_out = plan.npix;
    return PT_OK;
}

int pt_frame_async(pt_scene* s, const float meta[48], uint32_t t, int max_depth, float* d_radiance, void* stream) {
    if (!s || !d_radiance) return fail(PT_ERR_INVALID, "null argument");
    return render_impl(s, meta, t, 1, 1, max_depth, PT_MODE_AUTO, false, d_radiance, nullptr,
                       static_cast<hipStream_t>(stream));
}

int pt_frame(pt_scene* s, const float meta[48], uint32_t t, int max_depth, float* radiance) {
    return pt_frame_window(s, meta, nullptr, t, max_depth, radiance);
}

int pt_frame_window(pt_scene* s, const float meta[48], const pt_window* win, uint32_t t, int max_depth, float* radiance) {
    if (!s || !radiance || !meta) return fail(PT_ERR_INVALID, "null argument");
    return render_blocking(s, meta, win, t, 1, 1, max_depth, PT_MODE_AUTO, false, radiance, nullptr, nullptr, nullptr);
}

int pt_tonemap_async(pt_scene* s, const float* d_accum, size_t npix, uint32_t sample_runs, uint8_t* d_rgba,
                     void* stream) {
    if (!s || !d_accum || !d_rgba || sample_runs == 0) return fail(PT_ERR_INVALID, "null argument or zero sample_runs");
    HIP_TRY(hipSetDevice(s->device));
    ProfScope prof_scope(s);
    HIP_TRY(launch_tonemap(d_accum, npix, sample_runs, d_rgba, static_cast<hipStream_t>(stream)));
    return PT_OK;
}

int pt_readback_async(pt_scene* s, const float* d_src, size_t n, float* h_dst, void* stream) {
    if (!s) return fail(PT_ERR_INVALID, "null scene");
    if (n == 0) return PT_OK;
    if (!d_src || !h_dst) return fail(PT_ERR_INVALID, "null argument");
    if (((uintptr_t)d_src | (uintptr_t)h_dst) & 15u) return fail(PT_ERR_INVALID, "buffers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(s->device));
    void* hd = nullptr;  // pinned host memory: its address in the device's view
    if (hipHostGetDevicePointer(&hd, h_dst, 0) != hipSuccess || !hd) {
        (void)hipGetLastError();
        return fail(PT_ERR_INVALID, "h_dst is not pinned (page-locked) host memory");
    }
    HIP_TRY(launch_readback(d_src, static_cast<float*>(hd), n, static_cast<hipStream_t>(stream)));
    return PT_OK;
}

int pt_render_image(pt_scene* s, const float meta[48], uint32_t frame0, uint32_t nframes, uint32_t frame_stride,
                    int max_depth, int mode, uint8_t* rgba, pt_counters* counters) {
    if (!s || !rgba || !meta) return fail(PT_ERR_INVALID, "null argument");
    if (nframes == 0) return fail(PT_ERR_INVALID, "nframes == 0 (the image divides by the sample count)");
    return render_blocking(s, meta, nullptr, frame0, nframes, frame_stride, max_depth, mode, true, nullptr, nullptr, rgba, counters);
}

int pt_tonemap(const float* acc, size_t npix, uint32_t sample_runs, uint8_t* rgba) {
    if (!acc || !rgba || sample_runs == 0) return fail(PT_ERR_INVALID, "null argument or zero sample_runs");
    auto to_int32 = [](double v) -> int32_t {  // ECMAScript ToInt32
        if (!std::isfinite(v)) return 0;
        double m = std::fmod(std::trunc(v), 4294967296.0);
        if (m < 0) m += 4294967296.0;
        return (int32_t)(uint32_t)m;
    };
    auto u8 = [](int32_t v) -> uint8_t { return v < 0 ? 0 : (v > 255 ? 255 : (uint8_t)v); };
    for (size_t i = 0; i < npix; ++i) {
        const double r = (double)acc[3 * i] / sample_runs, g = (double)acc[3 * i + 1] / sample_runs,
                     b = (double)acc[3 * i + 2] / sample_runs;
        const double lum = (r + g + b) / 3.0;
        const double f = std::pow(lum / (lum + 1.0), 0.01);
        rgba[4 * i] = u8(to_int32(r * f * 255.0));
        rgba[4 * i + 1] = u8(to_int32(g * f * 255.0));
        rgba[4 * i + 2] = u8(to_int32(b * f * 255.0));
        rgba[4 * i + 3] = 255;
    }
    return PT_OK;
}

}  // extern "C"
