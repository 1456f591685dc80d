// pt_wf_bf.hip — brute force + replay for mailbox scenes (at most 64 distinct leaf entries): the
// closest-hit kernel k_wf_trace_bf and the fused step kernel k_wf_step_bf, which traces, shades and
// compacts in one launch.  Owns bf_replay_stackless, bf_closest, k_wf_camtab, the two kernels with
// bf_step_batch, their LDS size, the choice of the narrow, the 64-bit-address and the GEN instances,
// last_bf_width / last_step_addr and the diagnostic builds' pt_phase_stats_read; exports bf_stage and
// launch_camtab (pt_wf_stage.h) for the brute-force flavours of PT_WF_FLAVOURS.
#include <atomic>

#include "pt_wf_queue.h"
#include "pt_wf_stage.h"

namespace pt {

#if PT_PHASE_STATS
__device__ unsigned long long g_phase_stats[2][PH_COUNT][3];
#endif

// Brute force + replay: the closest-hit kernel for mailbox scenes (SceneView::mailbox: at most
// 64 distinct leaf entries, e.g. every Cornell box).  The reference's traversal (and the
// mailboxed one, trav_step_mb) tests ~19 of CornellBox's 36 distinct entries per query, in an
// order and number that differ from lane to lane, so SIMT lanes idle in each other's leaf
// loops (~30 % of the issued test slots do work).  Here a wave takes 64 queue entries at once
// and
//   phase 1  runs the triangle test of EVERY distinct entry u for all 64 rays in lockstep
//            (wave-uniform loop; the record is uniform, read through the scalar cache), keeping
//            per ray the set of entries hit and the t of the first kBfSlots hits (LDS);
//   phase 2  replays the reference's traversal per ray — node steps, exit-distance pruning,
//            the mailboxed leaf pairs of trav_step_mb — where a leaf entry costs a mask test
//            and, for entries that hit, a lookup of its t instead of a triangle test.
// Exact: a triangle test is a pure function of (ray, record), so phase 1 computes the same t
// (and hit predicate) the traversal would, and phase 2 applies them in the mailboxed order
// with the same strict-< update, tie-break and pruning; tests of entries the traversal never
// reaches have no effect.  A ray with more than `nslots` (<= kBfSlots, pt_flavour.h) hits recomputes the rest on demand.
__device__ __forceinline__ TriRec load_tri_scalar(const Tri* tris, int i) {
    // uniform index: constant address space, so the record comes through s_load (no VGPRs)
    const __attribute__((address_space(4))) float* f = (const __attribute__((address_space(4))) float*)(tris + i);
    return TriRec{make_float4(f[0], f[1], f[2], f[3]), make_float4(f[4], f[5], f[6], f[7]), f[8]};
}

// Phase 2 without a stack (SceneView::bfnode; scenes of <= 64 internal nodes, <= 63 entries).
// The reference's traversal visits nodes depth first, right child before left (a node with both
// children to visit keeps the left one on its stack), and a child's visit is decided when its
// parent is visited (the exit-distance test against the closest t at that moment).  With the
// internal nodes numbered in that visiting order (pre-order, right subtree first; pt_capi.hip
// build_layout), the node the stack walk takes next is always the smallest-numbered node
// decided but not yet visited: a stacked left child of an ancestor comes after everything below
// that ancestor's right child, and the current node's children come after it but before every
// stacked node.  So a 64-bit set of pending nodes walked by ctz replaces the stack, visiting the
// same nodes in the same order with the same decisions: the same leaf pairs, resolved exactly as
// in the stack walk below (mailbox set, phase 1's t, strict < with the pair's tie-break).
__device__ __forceinline__ bool mb_first_node(const SceneView& sc, int node, bool li, bool ri, int a, int b) {
    const int4 d = reinterpret_cast<const int4*>(sc.nodes)[4 * node + 3];
    const int na = (li & (d.z >= 0)) ? d.z : 0;
    const int nt = na + ((ri & (d.w >= 0)) ? d.w : 0);
    for (int k = 0; k < nt; ++k) {
        const int u = sc.tris[k < na ? d.x + k : d.y + (k - na)].uid;
        if (u == a || u == b) return u == a;
    }
    return false;
}

//
// NARROW (scenes of <= 32 entries and <= 32 internal nodes: SceneView::bfnarrow, e.g. CornellBox): the
// same walk with every set — hits, tested, pend, the leaf sets — in one 32-bit register instead of
// a pair, and with a pruning the narrow payload allows: a child's low word is the set of entries
// beneath it (pt_layout.h), and the walk takes a child only if that set still holds a hit of this
// ray that no leaf has resolved yet, (low & hits & ~tested) != 0.  Exact: visiting a subtree without
// such a hit only adds entries to `tested` that are no hits, or hits already in it, and the only
// reader of `tested` is rh = m & ~tested & hits — so the visit changes neither best, best_t, bcur
// nor any later rh; the nodes it would have queued lie inside that subtree, and the pending set
// orders the others by their numbers whatever else it holds, so they are visited in the same order
// with the same best_t at each decision.  A pruned leaf child holds neither entry of a tie the pair
// resolves (both are unresolved hits), so mb_first_node scans to the same answer without it.  The
// child's box test is issued only when some lane of the wave takes that child (wave vote).
template <bool FAST_RCP, bool NARROW = false>
__device__ __forceinline__ int bf_replay_stackless(const SceneView& sc, const Ray& r, bool active,
                                                   std::conditional_t<NARROW, uint32_t, uint64_t> hits,
                                                   float tmin, const float* slot, int nslots, float& t_out PH_PARAM) {
    if constexpr (NARROW) {
        uint32_t pend = active ? 1u : 0u;  // pre-order node 0 = the root
        uint32_t tested = 0;
        int best = -1;
        float best_t = -1.0f;
        while (wave_any(pend != 0)) {
            if (pend != 0) {
                PH_ITER(PH_REPLAY);
                const int n = (int)__builtin_ctz(pend);
                pend &= pend - 1;
                const BfNode& bn = sc.bfnarrow[n];
                const uint32_t lset = (uint32_t)bn.lm, lhi = (uint32_t)(bn.lm >> 32);
                const uint32_t rset = (uint32_t)bn.rm, rhi = (uint32_t)(bn.rm >> 32);
                const uint32_t open = hits & ~tested;  // hits no leaf has resolved yet
                const bool lneed = (lset & open) != 0, rneed = (rset & open) != 0;
                float ld = 0.0f, rd = 0.0f;
                if (__builtin_amdgcn_ballot_w64(lneed) != 0)  // wave-uniform
                    ld = ray_box(r, bn.lmin[0], bn.lmin[1], bn.lmin[2], bn.lmax[0], bn.lmax[1], bn.lmax[2]);
                if (__builtin_amdgcn_ballot_w64(rneed) != 0)
                    rd = ray_box(r, bn.rmin[0], bn.rmin[1], bn.rmin[2], bn.rmax[0], bn.rmax[1], bn.rmax[2]);
                const bool li = lneed & (0.0f < ld), ri = rneed & (0.0f < rd);
                const bool lint = lhi != 0, rint = rhi != 0;
                const uint32_t m = ((li & !lint) ? lset : 0u) | ((ri & !rint) ? rset : 0u);
                uint32_t rh = m & open;
                tested |= m;
                bool bcur = false;  // the best came from this leaf pair
                while (rh) {
                    PH_ITER(PH_RLEAF);
                    const int u = (int)__builtin_ctz(rh);
                    rh &= rh - 1;
                    const int k = __popc(hits & ((1u << u) - 1u));
                    const int rec = sc.mb_base + u;
                    float t;
                    if (k < nslots) t = slot[64 * k];
                    else tri_hit<FAST_RCP>(sc.tris, rec, r, t);  // a hit, so the same t as phase 1
                    bool take = (best_t < 0.0f) | (t < best_t);
                    if ((t == best_t) & bcur) take = mb_first_node(sc, sc.bfmap[n], li, ri, u, best - sc.mb_base);
                    best_t = take ? t : best_t;
                    best = take ? rec : best;
                    bcur |= take;
                }
                if (best_t == tmin) {
                    pend = 0;
                } else {
                    const bool tl = (li & lint) && !((best_t > 0.0f) & (ld > best_t));
                    const bool tr = (ri & rint) && !((best_t > 0.0f) & (rd > best_t));
                    pend |= (tl ? 1u << (lhi & 31u) : 0u) | (tr ? 1u << (rhi & 31u) : 0u);
                }
            }
        }
        t_out = best_t;
        return best;
    } else {
    constexpr uint64_t kInner = 1ull << 63;
    uint64_t pend = active ? 1ull : 0ull;  // pre-order node 0 = the root
    uint64_t tested = 0;
    int best = -1;
    float best_t = -1.0f;
    while (wave_any(pend != 0)) {
        if (pend != 0) {
            PH_ITER(PH_REPLAY);
            const int n = (int)__builtin_ctzll(pend);
            pend &= pend - 1;
            const BfNode& bn = sc.bfnode[n];
            const float ld = ray_box(r, bn.lmin[0], bn.lmin[1], bn.lmin[2], bn.lmax[0], bn.lmax[1], bn.lmax[2]);
            const float rd = ray_box(r, bn.rmin[0], bn.rmin[1], bn.rmin[2], bn.rmax[0], bn.rmax[1], bn.rmax[2]);
            const bool li = 0.0f < ld, ri = 0.0f < rd;
            const bool lint = (bn.lm & kInner) != 0, rint = (bn.rm & kInner) != 0;
            const uint64_t m = ((li & !lint) ? bn.lm : 0ull) | ((ri & !rint) ? bn.rm : 0ull);
            uint64_t rh = m & ~tested & hits;
            tested |= m;
            bool bcur = false;  // the best came from this leaf pair
            while (rh) {
                PH_ITER(PH_RLEAF);
                const int u = (int)__builtin_ctzll(rh);
                rh &= rh - 1;
                const int k = __popcll(hits & ((1ull << u) - 1));
                const int rec = sc.mb_base + u;
                float t;
                if (k < nslots) t = slot[64 * k];
                else tri_hit<FAST_RCP>(sc.tris, rec, r, t);  // a hit, so the same t as phase 1
                bool take = (best_t < 0.0f) | (t < best_t);
                if ((t == best_t) & bcur) take = mb_first_node(sc, sc.bfmap[n], li, ri, u, best - sc.mb_base);
                best_t = take ? t : best_t;
                best = take ? rec : best;
                bcur |= take;
            }
            if (best_t == tmin) {
                pend = 0;
            } else {
                const bool tl = (li & lint) && !((best_t > 0.0f) & (ld > best_t));
                const bool tr = (ri & rint) && !((best_t > 0.0f) & (rd > best_t));
                pend |= (tl ? 1ull << (uint32_t)(bn.lm & 63u) : 0ull) | (tr ? 1ull << (uint32_t)(bn.rm & 63u) : 0ull);
            }
        }
    }
    t_out = best_t;
    return best;
    }  // !NARROW
}

// Camera batches (CAM: every ray of the batch starts at the camera, fp.cam — the fused kernel's GEN
// launch): the parts of the triangle test that depend on the origin and the entry only — s = o - v0,
// s x e1 and e2 . (s x e1) — are the same for every camera ray, so k_wf_camtab computes them once
// per render per entry, with the same functions in the same order (so the same bits), and phase 1
// reads them through the scalar cache: camtab[2u] = (s, e2 . (s x e1)), camtab[2u + 1] = (s x e1, 0).
__global__ void k_wf_camtab(SceneView sc, FrameParams fp, float4* camtab) {
    const int u = (int)threadIdx.x;
    if (u >= sc.n_tris - sc.mb_base) return;
    const TriRec tr = load_tri(sc.tris, sc.mb_base + u);
    const f3 v0 = mk(tr.a.x, tr.a.y, tr.a.z), e1 = mk(tr.a.w, tr.b.x, tr.b.y), e2 = mk(tr.b.z, tr.b.w, tr.c);
    const f3 o = mk(fp.cam[0], fp.cam[1], fp.cam[2]);  // camera_ray's origin
    const f3 sv = o - v0;
    const f3 sce1 = cross(sv, e1);
    camtab[2 * u] = make_float4(sv.x, sv.y, sv.z, dot(e2, sce1));
    camtab[2 * u + 1] = make_float4(sce1.x, sce1.y, sce1.z, 0.0f);
}

// Closest hit of the 64 rays of one batch (lane = ray; `valid` false lanes give no hit):
// phase 1 + phase 2 above.  Returns the record (or -1) and its t in t_out.
// NARROW (never with COUNT; the caller's scene has SceneView::bfnarrow): the set of entries hit in 32
// bits, and the 32-bit replay.
template <bool FAST_RCP, bool COUNT, bool CAM = false, bool NARROW = false>
__device__ __forceinline__ int bf_closest(const SceneView& sc, const Tri* gtris, const Ray& r, bool valid, float* slot,
                                          int nslots, const LStack32& stack, Counters& c, float& t_out,
                                          const float4* camtab PH_PARAM) {
    const int U = sc.n_tris - sc.mb_base;
    // phase 1: every distinct entry against all 64 rays.  The test is tri_hit's arithmetic cut
    // after u: when no lane passes the det and u tests (the early-out chain of
    // ray-triangle-intersection.wgsl:15-24) the rest cannot make a hit and is skipped for the wave
    static_assert(!(NARROW && COUNT), "the counting instances keep the 64-bit sets");
    using Set = std::conditional_t<NARROW, uint32_t, uint64_t>;
    Set hits = 0;
    int nh = 0;
    const uint64_t vmask = __builtin_amdgcn_ballot_w64(valid);  // loop-invariant part of phase 1's vote
    float tmin = 3.0e38f;  // smallest t of any entry this ray hits
    for (int u = 0; u < U; ++u) {
        PH_ITER(PH_P1);
        const TriRec tr = load_tri_scalar(gtris, sc.mb_base + u);
        const f3 v0 = mk(tr.a.x, tr.a.y, tr.a.z), e1 = mk(tr.a.w, tr.b.x, tr.b.y), e2 = mk(tr.b.z, tr.b.w, tr.c);
        float4 ca = make_float4(0, 0, 0, 0);
        if constexpr (CAM) {
            const __attribute__((address_space(4))) float* f = (const __attribute__((address_space(4))) float*)(camtab + 2 * u);
            ca = make_float4(f[0], f[1], f[2], f[3]);
        }
        const f3 rce2 = cross(r.d, e2);
        const float det = dot(e1, rce2);
        const float inv_det = FAST_RCP ? rcp_rn(det) : 1.0f / det;
        const f3 sv = CAM ? mk(ca.x, ca.y, ca.z) : r.o - v0;
        const float bu = inv_det * dot(sv, rce2);
        const bool ok_det = !(det > -1e-8f && det < 1e-8f), ok_lo = !(bu < 0.0f), ok_hi = !(bu > 1.0f);
        const bool ok_u = valid & ok_det & ok_lo & ok_hi;
        // the vote as SGPR masks of the single compares (one ballot of the combined bool costs
        // two VALU slots per entry: v_cndmask + v_cmp)
        if ((vmask & __builtin_amdgcn_ballot_w64(ok_det) &
             __builtin_amdgcn_ballot_w64(ok_lo) & __builtin_amdgcn_ballot_w64(ok_hi)) == 0)
            continue;  // wave-uniform
        PH_ITER(PH_P1FULL);
        f3 sce1;
        float tn;
        if constexpr (CAM) {
            const __attribute__((address_space(4))) float* f = (const __attribute__((address_space(4))) float*)(camtab + 2 * u + 1);
            sce1 = mk(f[0], f[1], f[2]);
            tn = ca.w;
        } else {
            sce1 = cross(sv, e1);
            tn = dot(e2, sce1);
        }
        const float bv = inv_det * dot(r.d, sce1);
        const float t = inv_det * tn;
        const bool h = ok_u & !(bv < 0.0f) & !(bu + bv > 1.0f) & (t > 1e-8f);
        if (h) {
            if (nh < nslots) slot[64 * nh] = t;
            ++nh;
            hits |= (Set)1 << u;
            tmin = t < tmin ? t : tmin;  // = fminf here (t > 1e-8, never NaN) without its two canonicalising v_max
        }
    }
    // phase 2: the mailboxed traversal, leaf entries resolved from phase 1.  Without counters a
    // ray stops as soon as its closest t equals tmin: no later entry has a smaller t, and an
    // equal one can only win inside the pair just resolved (strict-< across pairs) — so the
    // result is final; a ray that hits nothing at all is final at once.  The counting build
    // (COUNT) walks on, to count the reference's work.
#if PT_PHASE_STATS
    {
        const uint64_t t1 = ph_now();
        pa.v[PH_P1][0] += t1 - pa.v[PH_COUNT][0];  // (the slot holds phase 1's start: set by the caller)
        pa.v[PH_COUNT][0] = t1;
    }
#endif
    if constexpr (NARROW)
        return bf_replay_stackless<FAST_RCP, true>(sc, r, valid && hits != 0, hits, tmin, slot, nslots, t_out PH_PASS);
    if constexpr (!COUNT) {
        if (sc.bfnode) {  // wave-uniform: the stackless walk (bf_replay_stackless)
            return bf_replay_stackless<FAST_RCP>(sc, r, valid && hits != 0, hits, tmin, slot, nslots, t_out PH_PASS);
        }
    }
    TravLean s;
    trav_init(s, valid && (COUNT || hits != 0));
    while (wave_any(!trav_finished(s))) {
        if (!trav_finished(s)) {
            mb_node_unit<COUNT>(sc, r, s, c);
            uint64_t rh = s.rem & hits;
            while (rh) {
                const int u = (int)__builtin_ctzll(rh);
                rh &= rh - 1;
                const int k = __popcll(hits & ((1ull << u) - 1));
                const int rec = sc.mb_base + u;
                float t;
                if (k < nslots) t = slot[64 * k];
                else tri_hit<FAST_RCP>(sc.tris, rec, r, t);  // a hit, so the same t as phase 1
                bool take = (s.best_t < 0.0f) | (t < s.best_t);
                if ((t == s.best_t) & ((s.fl & TF_BCUR) != 0)) take = mb_first(sc, s, u, s.best - sc.mb_base);
                s.best_t = take ? t : s.best_t;
                s.best = take ? rec : s.best;
                s.fl |= take ? TF_BCUR : 0;
            }
            s.rem = 0;
            s.fl &= ~TF_LEAF;
            if (!COUNT && s.best_t == tmin) s.fl |= TF_DONE;
            else lean_decide(s, stack);
        }
    }
    t_out = s.best_t;
    return s.best;
}

// LDS of the bf kernels: per-lane stacks, then per wave kBfSlots x 64 hit slots, then the scene
struct BfLds {
    LStack32 stack;
    float* slot;
    char* scene;
};
__device__ __forceinline__ BfLds bf_lds(char* smem, const SceneView& sc) {
    BfLds l;
    l.stack = LStack32::make(smem, blockDim.x);
    char* slot_base = smem + (uint32_t)sc.max_stack * blockDim.x * 4u;
    l.slot = reinterpret_cast<float*>(slot_base) + (threadIdx.x / 64u) * (kBfSlots * 64) + lane_id();  // slot k: slot[64k]
    l.scene = slot_base + (blockDim.x / 64u) * (kBfSlots * 64 * 4);
    return l;
}

template <bool LDS, bool FAST_RCP, bool COUNT>
__global__ __launch_bounds__(kTraceBlock) void k_wf_trace_bf(SceneView sc, WfBuffers wb, int in_q, Counters* cnt_out, int nslots) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const BfLds l = bf_lds(smem, sc);
    const uint32_t lane = lane_id();
    if (blockIdx.x == 0 && threadIdx.x == 0) wb.ctl[in_q ? WF_COUNT0 : WF_COUNT1] = 0;  // shade's output count
    const uint32_t count = wb.ctl[WF_WATCHDOG] ? 0u : wb.ctl[in_q ? WF_COUNT1 : WF_COUNT0];
    const Tri* gtris = sc.tris;  // global records for phase 1
    if (LDS) stage_scene_lds(sc, l.scene);
    const uint32_t nwaves = gridDim.x * (blockDim.x / 64);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64);
    const uint32_t nb = (count + 63) / 64;
    const float4* q = in_q ? wb.shd.ray : wb.ext.ray;
    Counters c = {};
    for (uint32_t b = w; b < nb; b += nwaves) {  // batches of 64 entries, interleaved over waves
        const uint32_t e = b * 64 + lane;
        const bool valid = e < count;
        uint32_t p;
        const Ray r = unpack_ray(valid ? q[2 * (size_t)e] : make_float4(0, 0, 0, 1),
                                 valid ? q[2 * (size_t)e + 1] : make_float4(0, 0, 0, 0), p);
        float t;
#if PT_PHASE_STATS
        PhaseAcc pa{};
#endif
        const int rec = bf_closest<FAST_RCP, COUNT>(sc, gtris, r, valid, l.slot, nslots, l.stack, c, t, nullptr PH_PASS);
        if (valid) wb.hitq[e] = make_int2(rec, __builtin_bit_cast(int, t));
    }
    if (COUNT) flush_counters(c, cnt_out);
}

// One batch of 64 entries of queue `in` (EXT: extension rays, else shadow rays) at entries
// rbase + b * 64 + lane (valid: b * 64 + lane < count): bf_closest, then the path logic of
// k_wf_shade (pt_path.h, so the same bits) in the same wave — the hit never goes through HBM
// and the ray record is read once — and the survivors appended to region rbase of the other
// queue at offsets from `append(n)` (wave-uniform: called by lane 0, result broadcast).
// GEN (the first extension launch, k_wf_step_bf's GEN): the batch's camera paths are made here
// instead of read from the queue — path p = (b * R + region) * 64 + lane, k_wf_generate's
// layout — and packed into the very words store_entry would have written, so everything after
// reads the same bits as from the queue (the queue write and read of the camera rays saved).
// Camera batches: region rg's k-th camera batch is the 64 paths (k * R + rg) * 64 + lane < P.
struct GenArgs {
    uint32_t frame0, stride, fbase, R, rg, P;
    bool raw_salt;
};
// k_wf_step_bf's arguments as they lie in its kernarg segment (each at its natural alignment, in order)
struct StepKernArgs {
    SceneView sc;
    FrameParams fp;
    WfBuffers wb;
    int it;
    Counters* cnt_out;
    int nslots;
    uint32_t frame0, stride, fbase, P;
    bool raw_salt;
    uint32_t q;
};
// The queue pointers the batch needs after the trace, read again from the kernarg segment (scalar
// loads at the use) instead of held in SGPRs across phase 1, where they were spilled to VGPR lanes.
// The asm keeps the loads behind the trace and inside the batch loop.
__device__ __forceinline__ void step_reload_queues(WfBuffers& w) {
    const __attribute__((address_space(4))) char* ka =
        (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const __attribute__((address_space(4))) WfBuffers* k =
        (const __attribute__((address_space(4))) WfBuffers*)(ka + offsetof(StepKernArgs, wb));
    w.ext.ray = k->ext.ray; w.ext.q2 = k->ext.q2; w.ext.q3 = k->ext.q3;
    w.shd.ray = k->shd.ray; w.shd.q2 = k->shd.q2; w.shd.q3 = k->shd.q3;
    w.sp0 = k->sp0; w.sp2 = k->sp2; w.rad = k->rad;
}
// genk (GEN instances; wave-uniform): >= 0 makes this batch camera batch genk of the region
// instead of queue batch b (the first launch); -1 reads the queue.
// CAM: the batch's rays are camera rays (a fresh batch of the first launch: bf_closest's table)
// A32: the queue arrays and `rad` by 32-bit byte offsets (q_at; the host launches these instances
// when step_addr32_ok holds for the part, pt_step_addr.h)
template <bool EXT, bool FAST_RCP, bool COUNT, bool GEN = false, bool CAM = GEN, bool NARROW = false, bool A32 = false,
          class Append>
__device__ __forceinline__ void bf_step_batch(const SceneView& sc, const Tri* gtris, const FrameParams& fp,
                                              const WfBuffers& wb, size_t rbase, uint32_t b, uint32_t count,
                                              const BfLds& l, int nslots, Counters& c, Append append,
                                              const GenArgs& gen, int64_t genk PH_PARAM) {
#if PT_PHASE_STATS
    const uint64_t t0 = ph_now();
#endif
    const WfQueue& in = EXT ? wb.ext : wb.shd;
    const uint32_t lane = lane_id();
    const bool fresh = GEN && genk >= 0;
    const uint32_t pg = fresh ? ((uint32_t)genk * gen.R + gen.rg) * 64 + lane : 0u;
    const bool valid = fresh ? pg < gen.P : b * 64 + lane < count;
    // the lane's entry (< qcap, a uint32_t) and its words' places in the input queue's arrays
    const uint32_t e = (uint32_t)rbase + ((valid && !fresh) ? b * 64 + lane : 0);
    const float4* const in_ray = ray_at<A32>(in.ray, e);
    const float4* const in_q2 = q_at<A32>(in.q2, e);
    const float4* const in_q3 = q_at<A32>(in.q3, e);
    float4 a0 = make_float4(0, 0, 0, 1), a1 = make_float4(0, 0, 0, 0);
    float4 c2 = make_float4(0, 0, 0, 0), d3 = c2;
    if (fresh) {
        if (valid) {
            uint32_t x, y, f;
            const uint32_t pid = slot_path(pg, fp, x, y, f);  // pg: the generation slot
            const uint32_t tt = gen.raw_salt ? gen.frame0 : (uint32_t)(float)(gen.frame0 + (gen.fbase + f) * gen.stride);
            PathState g;
            const Ray gr = path_begin(fp, x, y, tt, g);
            a0 = make_float4(gr.o.x, gr.o.y, gr.o.z, gr.d.x);
            a1 = make_float4(gr.d.y, gr.d.z, __builtin_bit_cast(float, pid), __builtin_bit_cast(float, pack_dspec(g)));
            c2 = make_float4(g.L.x, g.L.y, g.L.z, __builtin_bit_cast(float, g.seed));
            d3 = make_float4(g.beta.x, g.beta.y, g.beta.z, 0.0f);
            if (COUNT) { c.samples++; c.ext_queries++; }
        }
    } else if (EXT) {
        a0 = in_ray[0];
        a1 = in_ray[1];
        if (!valid) { a0 = make_float4(0, 0, 0, 1); a1 = make_float4(0, 0, 0, 0); }
    }
    uint32_t p;
    Ray r;
    if (EXT || fresh) {
        r = unpack_ray<FAST_RCP>(a0, a1, p);
    } else {  // packed shadow entry (store_shadow_packed): the origin from the shading point (its
              // words are read again after the trace, from cache, rather than held across it)
        // (loaded by every lane — an invalid lane's e is the region's first entry, inside the arrays — and
        // then replaced: loads under `valid` cost a branch each and their addresses 64-bit VALU)
        a0 = in_ray[0];
        float4 h3 = *in_q3, n4 = *q_at<A32>(wb.sp0, e);
        a1 = in_ray[1];  // the path state: below
        c2 = *in_q2;
        if (!valid) { a0 = make_float4(0, 0, 1, 0); h3 = make_float4(0, 0, 0, 0); n4 = h3; }
        r = unpack_shadow_ray<FAST_RCP>(a0, h3, n4, p);
    }
    // the path state is loaded before the trace and arrives while it runs (+1.3 %)
    if (!fresh && EXT) { c2 = *in_q2; d3 = *in_q3; }
    float t;
#if PT_PHASE_STATS
    {
        const uint64_t t1 = ph_now();
        pa.v[PH_LOAD][0] += t1 - t0;
        pa.v[PH_COUNT][0] = t1;  // phase 1's start, for bf_closest
    }
#endif
    // CAM: a camera batch (the first launch reads no queue: genk >= 0 throughout)
    const int rec = bf_closest<FAST_RCP, COUNT, CAM, NARROW>(sc, gtris, r, valid, l.slot, nslots, l.stack, c, t, wb.camtab PH_PASS);
#if PT_PHASE_STATS
    uint64_t t3 = ph_now();
    pa.v[PH_REPLAY][0] += t3 - pa.v[PH_COUNT][0];
    PH_ITER(PH_SHADE);  // the lanes entering the path logic (all of the batch's)
#endif
    bool more = false;
    PathState ps;
    WfBuffers wk = wb;  // the buffers as used from here on
    step_reload_queues(wk);
    if (valid) {
        if (EXT) {
            unpack_dspec(__builtin_bit_cast(uint32_t, a1.w), ps);
            ps.L = mk(c2.x, c2.y, c2.z);
            ps.seed = __builtin_bit_cast(uint32_t, c2.w);
            ps.beta = mk(d3.x, d3.y, d3.z);
            more = path_after_ext(sc, rec, t, r, ps);
            if (more && COUNT) c.shadow_queries++;
        } else {  // packed shadow entry
            unpack_dspec(__builtin_bit_cast(uint32_t, a1.x), ps);
            ps.L = mk(a1.y, a1.z, a1.w);
            ps.seed = __builtin_bit_cast(uint32_t, c2.x);
            ps.beta = mk(c2.y, c2.z, c2.w);
            // the shading point again (through the re-read pointers, which the compiler cannot match
            // with the loads before the trace: read from cache here, not held across the trace)
            const float4 h3 = *q_at<A32>(wk.shd.q3, e), n4 = *q_at<A32>(wk.sp0, e);
            ps.hp = mk(h3.x, h3.y, h3.z);
            ps.mat_id = __builtin_bit_cast(int, h3.w);
            const float2 w2 = *q_at<A32>(wk.sp2, e);
            ps.hn = mk(n4.x, n4.y, n4.z);
            ps.wi = mk(n4.w, w2.x, w2.y);
            more = path_after_shadow(sc, fp, rec, t, r, ps);
            if (more && COUNT) c.ext_queries++;
        }
        if (!more) {
            float* o = A32 ? q_at<true>(wk.rad, 3 * p) : wk.rad + 3 * (size_t)p;
            o[0] = ps.L.x; o[1] = ps.L.y; o[2] = ps.L.z;
        }
    }
#if PT_PHASE_STATS
    {
        const uint64_t t4 = ph_now();
        pa.v[PH_SHADE][0] += t4 - t3;
        t3 = t4;
    }
#endif
    const uint64_t keep = __ballot(more);
    if (keep) {  // wave-uniform
        uint32_t base = 0;
        if (lane == 0) base = append((uint32_t)__popcll(keep));
        base = __shfl(base, 0, 64);
        if (more) {
            PH_ITER(PH_APPEND);
            const uint32_t j = (uint32_t)rbase + base + rank_below(keep);
            if (EXT) store_shadow_packed<A32>(wk, j, r, p, ps);
            else store_entry<A32>(wk.ext, j, r, p, ps);
        }
    }
#if PT_PHASE_STATS
    pa.v[PH_APPEND][0] += ph_now() - t3;
#endif
}

// Trace + shade in one launch per iteration (mailbox scenes): queues are cut
// into wb.nreg regions (64-path batches dealt round-robin: camera batch j to region j mod nreg);
// the waves w ≡ r (mod nreg) serve region r of the input and append to region r of the output,
// one atomicAdd per wave and batch on that region's counter (a counter shared by all waves
// serialises at one memory channel, and each wave waits for its add: measured 2x slower).  A
// region's output never exceeds its input, so every region holds its paths through all
// bounces.  Iteration `it` reads the counts of slot it % 3, appends to slot (it + 1) % 3 and
// zeroes slot (it + 2) % 3 for iteration it + 1 (iteration it - 1 read that slot and it - 2
// wrote it, both finished: stream order).
// amdgpu_waves_per_eu(8): the path logic pushed the kernel to 75 VGPRs (6 waves/SIMD); capped
// at 64 it keeps 8 waves/SIMD with no VGPR spills (a few SGPR spills to VGPR lanes): +7 %
// GEN: the first launch makes the camera paths itself (bf_step_batch GEN; replaces
// k_wf_generate): region counts in closed form, the output counts zeroed by the host.
// GEN 2 (option regen = q): streaming regeneration — every extension launch j = it / 2 also admits
// the region's camera batches j q .. (j + 1) q - 1 behind its queued survivors, so the launches stay
// full until the camera batches run out (the host launches 2 (ceil(max camera batches / q) +
// max_depth) iterations).  Those launches mix queued and camera batches: no camera table.
// GEN | 4 (kStepNarrow): the narrow instance — 32-bit sets in phase 1 and the replay
// (bf_replay_stackless NARROW), launched by the host for scenes with SceneView::bfnarrow.  The width
// rides in GEN so that the kernel keeps its five template arguments (profile tools read them by
// position).
// GEN | 8 (kStepAddr64): the instance that addresses the queues with 64-bit indices, launched for a
// part whose arrays pass 4 GiB (step_addr32_ok false; option step_addr64 forces it: tests); the
// instances without it use 32-bit byte offsets (q_at).  The same body, the same bits.
constexpr int kStepNarrow = 4;
constexpr int kStepAddr64 = 8;
template <bool EXT, bool LDS, bool FAST_RCP, bool COUNT, int GENW = 0>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_wf_step_bf(SceneView sc, FrameParams fp, WfBuffers wb, int it,
                                                           Counters* cnt_out, int nslots, uint32_t frame0,
                                                           uint32_t stride, uint32_t fbase, uint32_t P, bool raw_salt,
                                                           uint32_t q) {
    constexpr int GEN = GENW & 3;
    constexpr bool NARROW = (GENW & kStepNarrow) != 0;
    constexpr bool A32 = (GENW & kStepAddr64) == 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const BfLds l = bf_lds(smem, sc);
    const uint32_t nwaves = gridDim.x * (blockDim.x / 64);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64);
    const uint32_t R = wb.nreg;  // <= nwaves (host)
    const uint32_t rg = w % R, g = w / R, G = (nwaves - rg + R - 1) / R;
    if (g == 0 && lane_id() == 0) wb.rcnt[((it + 2) % 3) * kRegions + rg] = 0;
    const uint32_t nbat = (P + 63) / 64;
    const uint32_t tg = (uint32_t)((uint64_t)rg * wb.rq % R);  // region rg's camera batches: tg, tg + R, ...
    const uint32_t ncam = tg < nbat ? (nbat - tg + R - 1) / R : 0u;
    uint32_t count, nqb, nnew = 0, k0 = 0;
    if constexpr (GEN == 1) {  // the first launch: every camera batch of region rg
        const uint32_t last = tg + (ncam - 1) * R;
        count = ncam == 0 ? 0u : ncam * 64 - ((last == nbat - 1 && (P & 63)) ? 64 - (P & 63) : 0u);
        if (w == 0 && lane_id() == 0) { wb.ctl[WF_COUNT0] = P; wb.ctl[WF_COUNT1] = 0; }
        nqb = 0;
        nnew = ncam;
    } else if constexpr (GEN == 2) {  // queued survivors (none in the first launch), then admissions
        count = it == 0 ? 0u : wb.rcnt[(it % 3) * kRegions + rg];
        nqb = (count + 63) / 64;
        k0 = (uint32_t)(it / 2) * q;
        nnew = ncam > k0 ? min(q, ncam - k0) : 0u;
        if (it == 0 && w == 0 && lane_id() == 0) { wb.ctl[WF_COUNT0] = P; wb.ctl[WF_COUNT1] = 0; }
    } else {
        count = wb.rcnt[(it % 3) * kRegions + rg];
        nqb = (count + 63) / 64;
    }
    uint32_t* out_count = &wb.rcnt[((it + 1) % 3) * kRegions + rg];
    const Tri* gtris = sc.tris;  // global records for phase 1
    if (LDS) stage_scene_lds(sc, l.scene);
    const uint32_t nb = nqb + nnew;
    const GenArgs ga{frame0, stride, fbase, R, tg, P, raw_salt};
    Counters c = {};
#if PT_PHASE_STATS
    PhaseAcc pa{};
#endif
    for (uint32_t b = g; b < nb; b += G)  // this region's batches, interleaved over its waves
        bf_step_batch<EXT, FAST_RCP, COUNT, GEN != 0, GEN == 1, NARROW, A32>(sc, gtris, fp, wb, (size_t)rg * wb.rstride, b, count, l,
                                                                nslots, c, [&](uint32_t n) { return atomicAdd(out_count, n); },
                                                                ga, b < nqb ? (int64_t)-1 : (int64_t)(k0 + b - nqb) PH_PASS);
    if (COUNT) flush_counters(c, cnt_out);
#if PT_PHASE_STATS
    if (!COUNT && lane_id() == 0) {
        pa.v[PH_COUNT][0] = 0;  // (the scratch slot)
        for (int ph = 0; ph < PH_COUNT; ++ph)
            for (int f = 0; f < 3; ++f) atomicAdd(&g_phase_stats[EXT ? 1 : 0][ph][f], (unsigned long long)pa.v[ph][f]);
    }
#endif
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static std::atomic<int> g_bf_width{0};
int last_bf_width() { return g_bf_width.load(); }
static std::atomic<int> g_step_addr{0};
int last_step_addr() { return g_step_addr.load(); }

hipError_t launch_camtab(const SceneView& sc, const FrameParams& fp, float4* camtab, hipStream_t stream) {
    if (sc.n_tris - sc.mb_base > 64) return hipErrorInvalidValue;  // mailbox scenes: <= 64 entries
    hipLaunchKernelGGL(k_wf_camtab, dim3(1), dim3(64), 0, stream, sc, fp, camtab);
    return hipSuccess;
}

template <bool LDS, bool FAST, bool COUNT>
static hipError_t bf_launch(const WfStage& sg, const WfCall& c, const WfPart& pt, int it, WfStepKind, uint32_t) {
    PT_LAUNCH(KID_WF_TRACE, pt.st, (k_wf_trace_bf<LDS, FAST, COUNT>), dim3(c.blocks), dim3(kTraceBlock), sg.lds, pt.st, sg.sc,
              pt.w, it & 1, c.cnt, c.bf_slots);
    return hipSuccess;
}

// Trace + shade in one launch: k_wf_step_bf<E, .., G> in its narrow instance (kStepNarrow) when the
// stage has one for G — uncounted, scene in LDS, the scene has the narrow payload (pt_capi.hip: <= 32
// entries and nodes, stackless replay and bf_narrow on), and no GEN 2 instance is narrow — with 32-bit
// queue offsets while the part's arrays allow them (pt_step_addr.h), else the 64-bit instance
// (kStepAddr64); option step_addr64 forces that one (tests)
template <bool E, int G, bool LDS, bool FAST, bool COUNT>
static void step_launch_as(const WfStage& sg, const WfCall& c, const WfPart& pt, int it, uint32_t regen_q) {
    const bool addr32 = !c.lo.step_addr64 && step_addr32_ok(pt.w.qcap, pt.P);
    auto kern = addr32 ? k_wf_step_bf<E, LDS, FAST, COUNT, G> : k_wf_step_bf<E, LDS, FAST, COUNT, G | kStepAddr64>;
    bool narrow = false;
    if constexpr (LDS && !COUNT && G != 2) {
        narrow = sg.narrow;
        if (narrow)
            kern = addr32 ? k_wf_step_bf<E, LDS, FAST, COUNT, G | kStepNarrow>
                          : k_wf_step_bf<E, LDS, FAST, COUNT, G | kStepNarrow | kStepAddr64>;
    }
    PT_LAUNCH(KID_WF_STEP, pt.st, kern, dim3(c.blocks), dim3(kTraceBlock), sg.lds, pt.st, sg.sc, c.fp, pt.w, it, c.cnt, c.bf_slots,
              c.frame0, c.stride, pt.fbase, pt.P, !c.accum, regen_q);
    g_bf_width = narrow ? 32 : (!COUNT && sg.sc.bfnode) ? 64 : 0;
    g_step_addr = addr32 ? 32 : 64;
}
template <bool LDS, bool FAST, bool COUNT>
static hipError_t step_launch(const WfStage& sg, const WfCall& c, const WfPart& pt, int it, WfStepKind kind, uint32_t regen_q) {
    switch (kind) {
        case WF_STEP_ADMIT: step_launch_as<true, 2, LDS, FAST, COUNT>(sg, c, pt, it, regen_q); break;
        case WF_STEP_GEN: step_launch_as<true, 1, LDS, FAST, COUNT>(sg, c, pt, it, regen_q); break;
        case WF_STEP_EXT: step_launch_as<true, 0, LDS, FAST, COUNT>(sg, c, pt, it, regen_q); break;
        case WF_STEP_SHADOW: step_launch_as<false, 0, LDS, FAST, COUNT>(sg, c, pt, it, regen_q); break;
    }
    return hipSuccess;
}

template <bool LDS, bool FAST, bool COUNT>
static void bf_instance(WfStage& sg) {
    sg.kernel = sg.fused ? (const void*)k_wf_step_bf<false, LDS, FAST, COUNT> : (const void*)k_wf_trace_bf<LDS, FAST, COUNT>;
    sg.launch = sg.fused ? step_launch<LDS, FAST, COUNT> : bf_launch<LDS, FAST, COUNT>;
    sg.narrow = sg.fused && LDS && !COUNT && sg.sc.bfnode && sg.sc.bfnarrow;
}

bool bf_stage(int trav, bool lds, bool count, const SceneView& sc_in, WfStage& sg) {
    if (!flv_brute_force(trav) || !wf_instantiated(trav)) return false;
    SceneView& sc = sg.sc = sc_in;
    // The brute-force kernels without counters replay without a stack when the scene has the BfNode
    // tree (bf_replay_stackless): no per-lane stack in their LDS (CornellBox: 14 KB of a 512-thread
    // block's 43 KB, so 4 blocks fit a CU's 160 KB instead of 3 — 8 waves per SIMD instead of 6).
    if (!count && sc.bfnode) sc.max_stack = 0;
    if (sc.node_bias <= 0) sc.node_bias = 4;  // (the traversal's turn policy, pt_wf_trace.hip: as every
    if (sc.node_steps <= 0) sc.node_steps = 4;  // flavour without pooled runs of 2)
    sg.fused = flv_fused(trav);
    sg.ring = kHitRing;
    sg.run2 = sc.leaf_pool == 2;
    // per-lane stacks, then per wave kBfSlots x 64 hit slots, then the scene (bf_lds)
    sg.lds = (size_t)sc.max_stack * kTraceBlock * 4 + (kTraceBlock / 64) * ((size_t)kBfSlots * 64 * 4) + (lds ? sc.span_bytes : 0);
    const bool fast = flv_fast(trav);
    if (lds) {
        if (fast) count ? bf_instance<true, true, true>(sg) : bf_instance<true, true, false>(sg);
        else count ? bf_instance<true, false, true>(sg) : bf_instance<true, false, false>(sg);
    } else {
        if (fast) count ? bf_instance<false, true, true>(sg) : bf_instance<false, true, false>(sg);
        else count ? bf_instance<false, false, true>(sg) : bf_instance<false, false, false>(sg);
    }
    return true;
}

}  // namespace pt

#if PT_PHASE_STATS
// diagnostic builds only (not in include/pt_hip.h): the fused kernel's per-phase sums since the last
// reset, [EXT][phase][cycles, iterations, lanes] as 2 x PH_COUNT x 3 u64 (scripts/phase_stats.py)
extern "C" int pt_phase_stats_read(unsigned long long* out, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -4;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(pt::g_phase_stats), sizeof(pt::g_phase_stats)) != hipSuccess) return -4;
    if (reset) {
        static const unsigned long long zero[2][pt::PH_COUNT][3] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pt::g_phase_stats), zero, sizeof zero) != hipSuccess) return -4;
    }
    return 0;
}
#endif

