// pt_flavour.h — the kernel flavours: what the `int TRAV` template parameter of the traversal, trace and
// step kernels means, which flavours are instantiated, and how the launch options and the scene
// select one.  The only place that compares a flavour id with a number.  It also holds LaunchOpts,
// the whole per-call option block with its defaults (the selectors take it; the other fields shape
// the launches).  No HIP types: host tools include it alone (scripts/flavour_select_harness.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PT_FLV_HD __host__ __device__
#else
#define PT_FLV_HD
#endif

namespace pt {

// Base flavours (option trav, in this order): nested loops (trace), flattened with per-lane branches
// (trav_step), flattened and predicated (trav_step_pred), lean (trav_step_lean) with K = 1, 2, 4, 8,
// 16, 32 triangle tests per leaf turn.
enum TravBase : int {
    TRAV_NESTED = 0, TRAV_FLAT, TRAV_PRED, TRAV_LEAN, TRAV_LEAN2, TRAV_LEAN4, TRAV_LEAN8, TRAV_LEAN16, TRAV_LEAN32,
    TRAV_BASE_COUNT
};
// A flavour id is a family's offset + the base (the brute-force families have none) + kFlvFast when
// 1/det comes from rcp_rn (scenes with SceneView::fast_rcp).  The numbers are part of the kernels'
// mangled names: profiles name them.
enum TravFamily : int {
    FLV_PLAIN = 0,      // the base flavour alone
    FLV_MAILBOX = 100,  // mailboxed lean<K> (SceneView::mailbox scenes; trav_step_mb)
    FLV_BIG = 160,      // lean<K> with big leaves in step (cooperative turns / chunk walks)
    FLV_PRE = 260,      // lean<K> with the big leaves resolved before the traversal (k_wf_leafpass)
    FLV_BF = 300,       // brute force + replay (k_wf_trace_bf)
    FLV_FUSED = 400,    // brute force + replay fused with the shading (k_wf_step_bf)
};
constexpr int kFlvFast = 10;

PT_FLV_HD constexpr int flavour(TravFamily fam, int base, bool fast) {
    return (int)fam + (fam >= FLV_BF ? 0 : base) + (fast ? kFlvFast : 0);
}
PT_FLV_HD constexpr bool flv_brute_force(int t) { return t >= FLV_BF; }  // both brute-force kernels
PT_FLV_HD constexpr bool flv_fused(int t) { return t >= FLV_FUSED; }
PT_FLV_HD constexpr bool flv_pre(int t) { return t >= FLV_PRE && t < FLV_BF; }
PT_FLV_HD constexpr bool flv_big(int t) { return t >= FLV_BIG && t < FLV_BF; }  // in step or pre-resolved
PT_FLV_HD constexpr bool flv_mailbox(int t) { return t >= FLV_MAILBOX && t < FLV_BIG; }
PT_FLV_HD constexpr bool flv_fast(int t) { return ((t / kFlvFast) & 1) != 0; }
PT_FLV_HD constexpr int flv_base(int t) { return flv_brute_force(t) ? -1 : t % kFlvFast; }
// the flavours whose traversal state is TravLean (the lean and the mailboxed steps)
PT_FLV_HD constexpr bool flv_lean_state(int t) { return flv_brute_force(t) || flv_base(t) >= TRAV_LEAN; }
// trav_step_lean's flavours: only they pool leaf turns or walk chunks
PT_FLV_HD constexpr bool flv_lean(int t) { return !flv_brute_force(t) && !flv_mailbox(t) && flv_base(t) >= TRAV_LEAN; }
// triangle tests per leaf turn of a lean or mailboxed flavour
PT_FLV_HD constexpr int flv_lean_k(int t) { return 1 << (flv_base(t) - TRAV_LEAN); }
// the traversal flavours that have a 256-entry-ring instance (the defaults: lean16 + fast rcp, with
// and without big leaves); the others always use 128
PT_FLV_HD constexpr bool flv_big_ring(int t) { return flv_lean(t) && flv_base(t) == TRAV_LEAN16 && flv_fast(t); }

static_assert(flavour(FLV_PLAIN, TRAV_LEAN16, true) == 17, "the wavefront's default traversal");
static_assert(flavour(FLV_BIG, TRAV_LEAN16, true) == 177 && flavour(FLV_PRE, TRAV_LEAN16, true) == 277, "... with big leaves");
static_assert(flavour(FLV_FUSED, 0, true) == 410 && flavour(FLV_BF, 0, false) == 300, "mailbox scenes' default");
static_assert(flavour(FLV_PLAIN, TRAV_LEAN4, true) == 15 && flavour(FLV_BIG, TRAV_LEAN4, true) == 175, "the megakernel's default");
static_assert(flavour(FLV_MAILBOX, TRAV_LEAN32, true) == 118 && flv_mailbox(118) && flv_fast(118) && flv_lean_k(118) == 32, "");
static_assert(flv_lean(17) && flv_lean(177) && flv_lean(277) && !flv_lean(117) && !flv_lean(2) && !flv_lean(410), "");
static_assert(flv_big(165) && flv_big(277) && flv_pre(265) && !flv_pre(177) && !flv_big(118) && !flv_big(300), "");
static_assert(flv_big_ring(17) && flv_big_ring(177) && flv_big_ring(277) && !flv_big_ring(7) && !flv_big_ring(117) &&
                  !flv_big_ring(16) && !flv_big_ring(410), "");
static_assert(flv_lean_k(15) == 4 && flv_lean_k(3) == 1 && !flv_fast(165) && flv_fast(275) && flv_lean_state(310), "");

// The instantiated flavours of each pipeline (X(id) per flavour; the launchers expand them for both
// LDS values).  Megakernel: k_regen.  Wavefront: k_wf_trace / k_wf_trace_pre / k_wf_trace_bf / k_wf_step_bf.
#define PT_MEGA_FLAVOURS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(13) X(14) X(15) X(175)
#define PT_WF_FLAVOURS(X)                                                   \
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(13) X(14) X(15) X(16) X(17) X(18) \
    X(300) X(310) X(400) X(410)                                             \
    X(105) X(106) X(107) X(115) X(116) X(117) X(118)                        \
    X(165) X(166) X(167) X(175) X(176) X(177)                               \
    X(265) X(266) X(267) X(275) X(276) X(277)
#define PT_FLV_IS(T) || t == T
constexpr bool mega_instantiated(int t) { return false PT_MEGA_FLAVOURS(PT_FLV_IS); }
constexpr bool wf_instantiated(int t) { return false PT_WF_FLAVOURS(PT_FLV_IS); }
#undef PT_FLV_IS

// hit slots per lane of the brute-force kernels (pt_wf_bf.hip: a ray with more hits recomputes the rest)
constexpr int kBfSlots = 8;

// Kernel selection, with every default resolved (pt_capi.hip launch_opts fills it from the option
// table; pt_set_option overrides are for tests and A/B runs).
struct LaunchOpts {
    bool wavefront = false;  // wavefront pipeline (pt_wavefront.hip: the driver; the kernels in pt_wf_*.hip)
    bool literal = false;    // k_mega: the reference's control flow
    bool lds = true;         // stage the scene in LDS when it fits
    // traversal base flavour.  Wavefront: lean16 (measured best on gfx950, scripts/perf_variants.py);
    // megakernel: lean4 (+ node bias 8 + fast reciprocal, measured at 1024^2 64 spp: 848 vs 611 for
    // lean2 with majority turns and the division)
    int trav = TRAV_LEAN4;
    bool fast_rcp = true;    // rcp_rn for 1/det where SceneView::fast_rcp says it is exact
    bool mailbox = true;     // mailboxed lean traversal where SceneView::mailbox allows it
    // wavefront, mailbox scenes: the brute-force + replay kernels instead of a traversal (an explicit
    // trav option turns it off: set_flavour_opts)
    bool bf = true;
    bool fuse = true;        // bf trace fused with the shading (k_wf_step_bf)
    bool fuse_gen = true;    // fused kernel: the first launch makes the camera paths (false: k_wf_generate)
    bool dual = true;        // wavefront batch split in parts on their own streams: +15 % measured (in-process A/B)
    int parts = 2;           // ... that many (1..kMaxParts)
    // traversal pipeline: survivors grouped per shade block by direction octant and origin cell (0 off,
    // 8, 64, 512 keys = 8 octants x 4^3 cells: CornellBox-Glossy +4.7 % with 64 keys, +1.2 % more with
    // 512, MedievalBoat unchanged, in-process A/B)
    int sort = 512;
    int bf_slots = kBfSlots; // brute-force kernels: hit slots per lane (fewer: tests of the recompute path)
    bool step_addr64 = false;  // fused kernel: the 64-bit addressing instance whatever the part's size (tests)
    int trace_blocks = 0;    // traversal / step kernels: cap on the grid (tests): 0 = occupancy-derived
    // k_wf_trace narrows its windows when 32-entry ones would keep < 1/n of the waves busy (0 off;
    // 4 in-process A/B: MedievalBoat +16 %, Glossy and the synthetic scenes +-0.5 %)
    int trace_sparse = 4;
    // k_wf_step_bf: camera batches dealt to regions by a permutation (WfBuffers::rq): a block's 8 waves
    // serve 8 neighbouring regions, which in row order hold neighbouring batches — at 4096^2, 512
    // neighbouring pixels of one row on one CU; permuted, batches far apart: 4096^2 2475 -> 2679
    // Msamples/s, 1024^2 and Mirror unchanged (profiles/r03h_ab_region_perm.txt)
    bool region_perm = true;
    int trace_ring = 0;      // k_wf_trace's hit ring: 0 auto, 128 or 256
    uint32_t watchdog = 0;   // k_wf_trace iterations before a wave gives up (tests of the failure report): 0 = kTraceWatchdog
    int leaf_blocks = 0;     // k_wf_leafpass grid (A/B): 0 = occupancy-derived
    int leaf_pairs = 5;      // k_wf_leafpass walks chunked leaves by (ray, chunk) pairs (option leaf_pairs; | 4: leaf_refine)
    // fused kernel: camera batches per region admitted by every extension launch (streaming
    // regeneration; 0: all at once — it measured 4.5 % slower in the bench, twice: DESIGN.md §7)
    int regen = 0;

    // The five options that pick a flavour, as the option table holds them (< 0: unset, the default
    // stays), once `wavefront` is set.  trav_opt unset = the pipeline's default base; an explicit
    // base flavour keeps the traversal kernels on mailbox scenes too (no brute force).
    constexpr void set_flavour_opts(int trav_opt, int fastrcp_opt, int mailbox_opt, int bf_opt, int fuse_opt) {
        if (fastrcp_opt >= 0) fast_rcp = fastrcp_opt != 0;
        if (mailbox_opt >= 0) mailbox = mailbox_opt != 0;
        if (bf_opt >= 0) bf = bf_opt != 0;
        if (fuse_opt >= 0) fuse = fuse_opt != 0;
        trav = trav_opt >= 0 ? trav_opt : wavefront ? (int)TRAV_LEAN16 : (int)TRAV_LEAN4;
        if (trav_opt >= 0) bf = false;
    }
};

// Options + scene facts -> flavour id.  fast_rcp, mailbox: SceneView's; big_leaf: SceneView::big_leaf
// > 0; pre_table: the scene's table of pre-resolved leaves holds its big leaves and the key buffer
// exists.  The launchers answer hipErrorInvalidValue for an id their pipeline does not instantiate.
constexpr int select_wavefront(const LaunchOpts& lo, bool fast_rcp, bool mailbox, bool big_leaf, bool pre_table) {
    const int base = lo.trav == TRAV_NESTED ? (int)TRAV_FLAT : lo.trav;  // always a flattened traversal
    const bool fast = lo.fast_rcp && fast_rcp;
    const bool lean_k = base >= TRAV_LEAN4;  // the flavours that have mailboxed and big-leaf forms
    const bool mb = lo.mailbox && mailbox;
    if (mb && lo.bf) return flavour(lo.fuse ? FLV_FUSED : FLV_BF, 0, fast);
    if (mb && lean_k) return flavour(FLV_MAILBOX, base, fast);
    // lean<4..16> on scenes with big leaves: cooperative turns, or the leaf pass when it can run
    if (big_leaf && lean_k && base <= TRAV_LEAN16) return flavour(pre_table ? FLV_PRE : FLV_BIG, base, fast);
    return flavour(FLV_PLAIN, base, fast && base >= TRAV_LEAN);
}
constexpr int select_megakernel(const LaunchOpts& lo, bool fast_rcp, bool /*mailbox*/, bool big_leaf, bool /*pre_table*/) {
    const int base = lo.trav > TRAV_LEAN4 ? (int)TRAV_LEAN4 : lo.trav;  // k_regen has no wider leaf turns
    const bool fast = lo.fast_rcp && fast_rcp && base >= TRAV_LEAN;
    // cooperative big-leaf turns: lean4 with the fast reciprocal only
    return flavour(big_leaf && base == TRAV_LEAN4 && fast ? FLV_BIG : FLV_PLAIN, base, fast);
}

}  // namespace pt
