// pt_wf_trace.hip — the windowed traversal of a wavefront queue: k_wf_trace and, with the big leaves
// resolved before it (FLV_PRE: launch_leafpass, pt_leafpass.hip), k_wf_trace_pre.  Owns wf_trace_body and
// the two kernels, their LDS size, the choice of hit ring and pooled-run instance, the per-instance
// defaults of node_bias / node_steps, and the diagnostic builds' pt_trace_stats_read; exports trace_stage
// (pt_wf_stage.h) for every flavour of PT_WF_FLAVOURS that is not brute force.
#include "pt_occupancy.h"
#include "pt_wf_queue.h"
#include "pt_wf_stage.h"

namespace pt {

#if PT_TRACE_STATS
__device__ unsigned long long g_trace_stats[2][TS_COUNT][3];  // [shadow queue][kind][cycles, turns, lanes]
#endif

// Per-wave LDS staging for k_wf_trace: the current window of 32 queued rays and a ring of
// hit records.  Keeping both in LDS takes every global load and store out of the traversal
// loop: on gfx9 loads and stores share the wave's in-order vmcnt, so a per-lane global store
// (or prefetch) in the loop makes the next use of any loaded register wait for it.
constexpr uint32_t kWinRays = 32;
// the hit ring, kHitRing or kHitRingMax entries: pt_wf_plan.h
// window ids of the windows between the last flushed and the prefetched one: the ring holds
// RING / kWinRays windows, plus the one in registers (a compile-time size per kernel instance: a
// ring size read at run time measured 10 % slower on the deep synthetic trees)
__host__ __device__ constexpr uint32_t win_tab(uint32_t ring) { return 2 * ring / kWinRays > 8 ? 2 * ring / kWinRays : 8; }
static_assert(win_tab(kHitRingMax) >= kHitRingMax / kWinRays + 2, "wtab must name every window the ring can hold");
static_assert(win_tab(kHitRing) >= kHitRing / kWinRays + 2, "wtab must name every window the ring can hold");
// per wave: the window's rays, the hit ring, the window ids, and 64 keys — one per lane for
// lean_leaf_pool's pooled leaf turns, the first kMultiRays for chunk_turn_multi's shared walks
__host__ __device__ constexpr uint32_t stage_bytes(uint32_t ring) { return kWinRays * 32 + ring * 8 + win_tab(ring) * 4; }
// after the waves' stages, when the scene needs them (pooled leaf turns or leaf chunks: keys_on),
// 64 keys per wave — one per lane for lean_leaf_pool, the first kMultiRays for chunk_turn_multi
constexpr uint32_t kKeyBytes = 64 * 8;
// Only the lean flavours pool leaf turns or walk chunks (trav_step_lean; not the mailboxed nor the
// flattened ones), so only their instances reserve the keys (advisor r04: every instance did)
template <int TRAV>
__host__ __device__ inline bool keys_on(const SceneView& sc) {
    return flv_lean(TRAV) && (sc.leaf_pool != 0 || sc.lnodes != nullptr);
}
// LDS of k_wf_trace per block (blocks of kTraceBlock, pt_wf_stage.h): the lanes' traversal stacks
// (max_stack entries of 4 B) and per wave stage_bytes(ring): trace_lds below

// Work split: the queue is cut into windows of 32 entries; wave w of N takes windows w, w+N,
// w+2N, ... (interleaving, not contiguous chunks, because queue order is spatially coherent —
// camera rays in pixel order, survivors compacted block by block — so a contiguous chunk is an
// image region whose cost differs systematically from the others).  Inside a wave, its j-th
// window's entries have the wave-local sequence numbers 32j .. 32j+31, which index the hit ring;
// wtab keeps the ids of the windows between the last written back and the prefetched one.
// No occupancy attribute: the big-leaf instances take 71 VGPRs (7 waves per SIMD); forcing
// amdgpu_waves_per_eu(7) made them 72 and 11 % slower on the 100k synthetic scene (in process,
// profiles/r03m_ab_trace_occ.log).
// sparse (option trace_sparse=n): when windows of wr entries would keep fewer than 1/n of the waves
// busy (the last depths), windows of wr / 2 .. 1 entries spread the queue over more waves, so each
// wave's traversal is the slowest of fewer rays.  A window still takes kWinRays sequence numbers
// (ring and flush bookkeeping unchanged); only its queue span is wr.
template <bool LDS, int TRAV, bool COUNT, uint32_t RING, int PRUN>
__device__ __forceinline__ void wf_trace_body(SceneView sc, WfBuffers wb, int in_q, Counters* cnt_out, uint32_t watchdog,
                                              int sparse) {
    constexpr uint32_t nring = RING, kWinTab = win_tab(RING);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LStack32 stack = LStack32::make(smem, blockDim.x);
    char* stage_base = smem + (uint32_t)sc.max_stack * 4u * blockDim.x;
    char* stage = stage_base + (threadIdx.x / 64u) * stage_bytes(nring);
    float4* wray = reinterpret_cast<float4*>(stage);               // [kWinRays][2]
    int2* ring = reinterpret_cast<int2*>(stage + kWinRays * 32);   // [RING]
    uint32_t* wtab = reinterpret_cast<uint32_t*>(stage + kWinRays * 32 + RING * 8);  // [kWinTab] window ids
    char* key_base = stage_base + (blockDim.x / 64u) * stage_bytes(nring);
    const uint32_t key_bytes = keys_on<TRAV>(sc) ? (blockDim.x / 64u) * kKeyBytes : 0u;
    sc.lkeys = key_bytes ? reinterpret_cast<uint64_t*>(key_base + (threadIdx.x / 64u) * kKeyBytes) : nullptr;
    sc.pres = wb.pres;  // this part's pre-resolved big leaves (FLV_PRE; k_wf_leafpass)
    sc.pres_stride = wb.pres_stride;
    if (blockIdx.x == 0 && threadIdx.x == 0) wb.ctl[in_q ? WF_COUNT0 : WF_COUNT1] = 0;  // shade's output count
    const uint32_t count = wb.ctl[WF_WATCHDOG] ? 0u : wb.ctl[in_q ? WF_COUNT1 : WF_COUNT0];  // gave up: skip
    // the wave index is uniform: readfirstlane keeps everything derived from it in SGPRs
    const uint32_t nwaves = gridDim.x * (blockDim.x / 64);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64);
    uint32_t wr = kWinRays;
    if (sparse > 0)
        while (wr > 1 && (uint64_t)count * (uint32_t)sparse < (uint64_t)nwaves * wr) wr >>= 1;
    const uint32_t nwin = (count + wr - 1) / wr;
    if (LDS) stage_scene_lds(sc, key_base + key_bytes);
    const uint32_t lane = lane_id();
    constexpr uint32_t kNone = 0xffffffffu;
    uint32_t nstatic = 0;
    auto fetch = [&]() {  // this wave's next window (wave-uniform), or kNone
        const uint64_t wid = (uint64_t)(nstatic++) * nwaves + w;
        return wid < nwin ? (uint32_t)wid : kNone;
    };
    auto wcount = [&](uint32_t wid) { return min(wr, count - wid * wr); };
    const uint32_t w0 = fetch();
    if (w0 == kNone) return;  // wave-uniform: nothing for this wave
    uint32_t wcur = w0, wnx = kNone;  // ids of window jl (handed out now) and of the one in flight
    // lanes 0..31 load the first halves of a window's ray records, lanes 32..63 the second
    const uint32_t wl = lane & (kWinRays - 1), half = lane / kWinRays;
    const float4* q = in_q ? wb.shd.ray : wb.ext.ray;
    Counters c = {};
    // local window jl (id wtab[jl % kWinTab]) sits in LDS; window jl + 1 is in flight in registers
    uint32_t jl = 0, wv = wcount(w0);
    if (lane == 0) wtab[0] = w0;
    if (wl < wv) wray[2 * wl + half] = q[2 * (size_t)(w0 * wr + wl) + half];
    uint32_t nv = 0;
    float4 na = make_float4(0, 0, 0, 0);
    {
        const uint32_t w1 = fetch();
        wnx = w1;
        if (w1 != kNone) {
            nv = wcount(w1);
            if (lane == 0) wtab[1] = w1;
            if (wl < nv) na = q[2 * (size_t)(w1 * wr + wl) + half];
        }
    }
    uint32_t cur = 0;      // sequence number of the next entry to hand out (in window jl)
    uint32_t flushed = 0;  // sequence numbers below this are written back to wb.hitq
    uint32_t sq = 0, p = 0;
    bool has = false;
    Ray r;
    r.o = r.d = r.inv = mk(0.0f, 0.0f, 0.0f);
    typename TravSel<TRAV>::type s;
    trav_init(s, false);
    const uint64_t t_start = wall_clock64();
#if PT_TRACE_STATS
    uint64_t tl0 = __builtin_amdgcn_s_memtime();
#endif
    for (uint32_t guard = 0;; ++guard) {
#if PT_TRACE_STATS
        {
            const uint64_t tl1 = __builtin_amdgcn_s_memtime();
            if (guard) ts_add(c, TS_LOOP, tl1 - tl0, (uint64_t)__popcll(__ballot(has)));
            tl0 = tl1;
        }
#endif
        // every wave reaches an exit: after kTraceWatchdog iterations or kTraceWatchdogTicks of
        // wall clock it reports instead of hanging (and later launches of the render skip)
        if (guard == watchdog ||
            ((guard & 1023u) == 1023u && wall_clock64() - t_start > kTraceWatchdogTicks)) {
            const uint64_t hm = __ballot(has);
            if (lane == 0) {
                atomicOr(&wb.ctl[WF_WATCHDOG], 1u);
                if (atomicCAS(&wb.ctl[WF_SNAP_CLAIM], 0u, 1u) == 0u) {
                    const uint32_t v[WF_SNAP_WORDS] = {count, nwaves, w, jl, wv, nv, cur, flushed,
                                                       (uint32_t)__popcll(hm), (uint32_t)hm, (uint32_t)(hm >> 32),
                                                       (uint32_t)in_q, 0u, 0u, 0u, 0u};
                    for (int i = 0; i < WF_SNAP_WORDS; ++i) wb.ctl[WF_SNAP + i] = v[i];
                }
            }
            break;
        }
        // write back every window whose entries are all handed out and traced (coalesced)
        while (flushed < (jl + 1) * kWinRays) {
            const uint32_t jf = flushed / kWinRays;
            const bool handed = jf < jl || cur == jl * kWinRays + wv;
            if (!handed || wave_any(has && sq < flushed + kWinRays)) break;
            const uint32_t wf = wtab[jf % kWinTab];
            const uint32_t fv = wcount(wf);
            if (lane < fv) wb.hitq[wf * wr + lane] = ring[(flushed + lane) & (nring - 1)];
            flushed += kWinRays;
        }
        // hand the next entries to idle lanes (wave-uniform control)
        const uint64_t need = __ballot(!has);
#if PT_TRACE_STATS
        if (need && cur == jl * kWinRays + wv) {  // idle lanes and the window handed out: why no next one?
            if (nv > 0 && (jl + 2) * kWinRays - flushed > nring) ts_add(c, TS_BLOCKED, 0, (uint64_t)__popcll(need));
            else if (nv == 0) ts_add(c, TS_STARVED, 0, (uint64_t)__popcll(need));
        }
#endif
        if (need) {
            if (cur == jl * kWinRays + wv && nv > 0 && (jl + 2) * kWinRays - flushed <= nring) {
                if (wl < nv) wray[2 * wl + half] = na;  // next window, if the hit ring has room
                ++jl;
                wv = nv;
                cur = jl * kWinRays;
                nv = 0;
                wcur = wnx;
                const uint32_t wn = fetch();
                wnx = wn;
                if (wn != kNone) {
                    nv = wcount(wn);
                    if (lane == 0) wtab[(jl + 1) % kWinTab] = wn;
                    if (wl < nv) na = q[2 * (size_t)(wn * wr + wl) + half];
                }
            }
            const uint32_t wend = jl * kWinRays + wv;
            if (cur < wend) {
                const uint32_t k = cur + rank_below(need);
                if (!has && k < wend) {
                    const uint32_t o = k - jl * kWinRays;
                    r = unpack_ray(wray[2 * o], wray[2 * o + 1], p);
                    sq = k;
                    trav_init(s, true);
                    if constexpr (flv_pre(TRAV)) s.qi = wcur * wr + o;  // its queue entry
                    has = true;
                }
                cur = min(cur + (uint32_t)__popcll(need), wend);
            }
        }
        if (!wave_any(has)) {
            if (nv == 0 && cur == jl * kWinRays + wv && flushed >= (jl + 1) * kWinRays) break;  // all done
            continue;  // ring full with nothing in flight: the flush above frees it
        }
#if PT_TRACE_STATS
        if (!trav_advance<TRAV, COUNT, true, PRUN>(sc, r, s, stack, c)) ts_add(c, TS_NONE, 0, 0);
#else
        trav_advance<TRAV, COUNT, true, PRUN>(sc, r, s, stack, c);
#endif
        if (has && trav_finished(s)) {
            ring[sq & (nring - 1)] = make_int2(s.best, __builtin_bit_cast(int, s.best_t));
            has = false;
        }
    }
    if (COUNT) flush_counters(c, cnt_out);
#if PT_TRACE_STATS
    if (!COUNT && lane == 0)
        for (int k = 0; k < TS_COUNT; ++k)
            for (int f = 0; f < 3; ++f) atomicAdd(&g_trace_stats[in_q ? 1 : 0][k][f], (unsigned long long)c.ts[k][f]);
#endif
}
template <bool LDS, int TRAV, bool COUNT, uint32_t RING = kHitRing, int PRUN = 4>
__global__ __launch_bounds__(kTraceBlock) void k_wf_trace(SceneView sc, WfBuffers wb, int in_q, Counters* cnt_out,
                                                          uint32_t watchdog, int sparse) {
    wf_trace_body<LDS, TRAV, COUNT, RING, PRUN>(sc, wb, in_q, cnt_out, watchdog, sparse);
}
// The instances with pre-resolved big leaves (FLV_PRE): held to 80 VGPRs, 6 waves per SIMD
// (83 unconstrained: 5 waves)
#ifndef PT_TRACE_PRE_WAVES
#define PT_TRACE_PRE_WAVES 6
#endif
template <bool LDS, int TRAV, bool COUNT, uint32_t RING = kHitRing, int PRUN = 4>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(PT_TRACE_PRE_WAVES, 8))) void k_wf_trace_pre(
    SceneView sc, WfBuffers wb, int in_q, Counters* cnt_out, uint32_t watchdog, int sparse) {
    wf_trace_body<LDS, TRAV, COUNT, RING, PRUN>(sc, wb, in_q, cnt_out, watchdog, sparse);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// the kernel of a flavour (pt_flavour.h)
template <bool LDS, int TRAV, bool COUNT, uint32_t RING = kHitRing, int PRUN = 4>
constexpr auto trace_kernel() {
    if constexpr (flv_pre(TRAV)) return k_wf_trace_pre<LDS, TRAV, COUNT, RING, PRUN>;
    else return k_wf_trace<LDS, TRAV, COUNT, RING, PRUN>;
}
// the k_wf_trace instances with a 256-entry ring and with pooled runs of 2 (SceneView::leaf_pool
// == 2): the default flavours (flv_big_ring), uncounted (the others pool runs of 4: the same bits and counts)
template <int TRAV, bool COUNT>
constexpr bool has_variants() { return flv_big_ring(TRAV) && !COUNT; }
template <bool LDS, int TRAV, bool COUNT>
static auto trace_instance(uint32_t ring, bool run2) {
    if constexpr (has_variants<TRAV, COUNT>()) {
        if (ring == kHitRingMax)
            return run2 ? trace_kernel<LDS, TRAV, COUNT, kHitRingMax, 2>() : trace_kernel<LDS, TRAV, COUNT, kHitRingMax>();
        if (run2) return trace_kernel<LDS, TRAV, COUNT, kHitRing, 2>();
    }
    (void)ring;
    (void)run2;
    return trace_kernel<LDS, TRAV, COUNT>();
}
template <bool LDS, int TRAV>
static size_t trace_lds(const SceneView& sc, uint32_t ring) {
    const size_t span = LDS ? sc.span_bytes : 0;
    return (size_t)sc.max_stack * 4 * kTraceBlock + (kTraceBlock / 64) * (stage_bytes(ring) + (keys_on<TRAV>(sc) ? kKeyBytes : 0)) + span;
}
static size_t max_block_lds() {
    static const size_t v = [] {
        int dev = 0, x = 0;
        hipGetDevice(&dev);
        hipDeviceGetAttribute(&x, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
        return (size_t)x;
    }();
    return v;
}

// launch `it` of a part: the big leaves first (k_wf_leafpass) for FLV_PRE, then the stage's instance
template <bool LDS, int TRAV, bool COUNT>
static hipError_t trace_launch(const WfStage& sg, const WfCall& c, const WfPart& pt, int it, WfStepKind, uint32_t) {
    const int in_q = it & 1;  // the queue the trace kernels read
    if constexpr (flv_pre(TRAV))
        HIP_RETURN_IF(launch_leafpass(sg.sc, pt.w, in_q, flv_fast(TRAV), c.lo.leaf_blocks, c.lo.leaf_pairs, pt.st));
    PT_LAUNCH(KID_WF_TRACE, pt.st, (trace_instance<LDS, TRAV, COUNT>(sg.ring, sg.run2)), dim3(c.blocks), dim3(kTraceBlock), sg.lds,
              pt.st, sg.sc, pt.w, in_q, c.cnt, c.watchdog, c.sparse);
    return hipSuccess;
}

template <bool LDS, int TRAV, bool COUNT>
static bool trace_stage_t(const SceneView& sc_in, const LaunchOpts& lo, WfStage& sg) {
    if constexpr (flv_brute_force(TRAV)) {
        return false;  // pt_wf_bf.hip's
    } else {
        SceneView& sc = sg.sc = sc_in;
        sg.fused = false;
        sg.narrow = false;
        sg.ring = kHitRing;
        sg.run2 = sc.leaf_pool == 2;  // pooled runs of 2 (the has_variants instances)
        // turn policy of the lean traversal: 4 since the queues are grouped by coherence keys (in process:
        // Glossy +2.5 %, boat +1 %, 1M synthetic +1.8 % over 8; 1 = majority: -13 % in round 1); 1 for the
        // instances that pool runs of 2 (100k +5.2 %, 1M +5.3 % over 4, both orders:
        // profiles/r04ai_node_bias.log; with runs of 4 the bias is within noise, r04z_ab_node_bias.log).
        // Chosen from the instance launched (advisor r04: the counted and non-default flavours pool runs
        // of 4 whatever sc.leaf_pool says)
        if (sc.node_bias <= 0) sc.node_bias = (sg.run2 && has_variants<TRAV, COUNT>()) ? 1 : 4;
        // node steps per node turn: 4 (in process over 1, same bits: Glossy +4.4 %, Glossy SAH +4.1 %, the boat
        // +4.1 %, boat SAH +10.3 %, synthetic 1k +3.2 %, 100k +1.5 %; 3/6/8 within or below; r06g/r06h_ab_*.log)
        if (sc.node_steps <= 0) sc.node_steps = 4;
        if constexpr (has_variants<TRAV, COUNT>()) {  // the ring (wf_ring, pt_wf_plan.h)
            const size_t l1 = trace_lds<LDS, TRAV>(sc, kHitRing), l2 = trace_lds<LDS, TRAV>(sc, kHitRingMax);
            int occ_big = 0, occ_small = 0;
            if (wf_ring_by_occupancy(lo.trace_ring, l2, max_block_lds())) {
                occ_big = occupancy_blocks((const void*)trace_instance<LDS, TRAV, COUNT>(kHitRingMax, sg.run2), kTraceBlock, l2);
                occ_small = occupancy_blocks((const void*)trace_instance<LDS, TRAV, COUNT>(kHitRing, sg.run2), kTraceBlock, l1);
            }
            sg.ring = wf_ring(lo.trace_ring, l2, max_block_lds(), occ_big, occ_small);
        }
        sg.lds = trace_lds<LDS, TRAV>(sc, sg.ring);
        sg.kernel = (const void*)trace_instance<LDS, TRAV, COUNT>(sg.ring, sg.run2);
        sg.launch = trace_launch<LDS, TRAV, COUNT>;
        return true;
    }
}

bool trace_stage(int trav, bool lds, bool count, const SceneView& sc, const LaunchOpts& lo, WfStage& sg) {
#define PT_STAGE(T)                                                                                                      \
    case T:                                                                                                         \
        return lds ? (count ? trace_stage_t<true, T, true>(sc, lo, sg) : trace_stage_t<true, T, false>(sc, lo, sg)) \
                   : (count ? trace_stage_t<false, T, true>(sc, lo, sg) : trace_stage_t<false, T, false>(sc, lo, sg));
    switch (trav) { PT_WF_FLAVOURS(PT_STAGE) }
#undef PT_STAGE
    return false;
}

}  // namespace pt

#if PT_TRACE_STATS
// diagnostic builds only: k_wf_trace's turn statistics since the last reset, [queue][kind][cycles,
// turns, lanes] as 2 x TS_COUNT x 3 u64 (scripts/trace_stats.py)
extern "C" int pt_trace_stats_read(unsigned long long* out, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -4;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(pt::g_trace_stats), sizeof(pt::g_trace_stats)) != hipSuccess) return -4;
    if (reset) {
        static const unsigned long long zero[2][pt::TS_COUNT][3] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pt::g_trace_stats), zero, sizeof zero) != hipSuccess) return -4;
    }
    return 0;
}
#endif
