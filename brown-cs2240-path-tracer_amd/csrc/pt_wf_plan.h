// pt_wf_plan.h — the plan of a wavefront call: how large a batch is, how its frames are dealt to parts,
// how the fused kernel's queues are cut into regions, which launches streaming regeneration needs, and
// the clamps of the small options.  Integers in, plain structs of integers out: the arithmetic that
// launch_wavefront (pt_wavefront.hip) and prepare_wavefront / ensure_wavefront (pt_capi_render.hip) act
// on, and nothing else.  Host only, standard C++ (constexpr only, so it also compiles into the device
// units that include pt_kernels.h); no HIP types: scripts/wf_plan_harness.cpp includes it alone and
// tests/test_wf_plan_cpu.py pins it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "pt_flavour.h"

namespace pt {

constexpr uint32_t kRegions = 512;
// queue slack (entries per part = 64 * this): regions of R <= kRegions hold ceil(batches / R)
// 64-entry batches each
constexpr uint32_t kQueueSlackRegions = 4096;
constexpr int kMaxParts = 4;  // parts of a wavefront batch on their own streams (LaunchOpts::parts)
// paths in flight per wavefront batch (kWfBytesPerPath = 188 B of queue state per path: 64 M
// paths ~ 12 GB of the 288 GB, plus the queue slack of the region layout).  Every batch ends in
// launch tails that carry few paths at low occupancy (the last depths); a larger batch pays them
// for more samples: CornellBox 1024^2 x 256 +6 % at 64 M over 8 M, CornellBox-Glossy +28 %
// (probe of option wf_paths)
constexpr uint64_t kWfTargetPaths = 64ull << 20;
// k_wf_trace's hit ring: 128 or 256 entries (a power of two, a multiple of kWinRays, >= 2 windows), chosen
// per launch (wf_ring): a larger ring lets a wave take new windows while more of its earlier
// windows' stragglers still trace (Glossy: 64 entries -15 %, 256 +4.3 % in process,
// profiles/r03k_ab_ring*.log), but its LDS can cost a block per CU (the boat: 3 -> 2 blocks, -2.4 %)
constexpr uint32_t kHitRing = 128;
constexpr uint32_t kHitRingMax = 256;

// ---- batch size (prepare_wavefront) ----

// The paths a call's batch should hold (`want`) and where the out-of-memory halving stops (`floor`: one
// frame per batch), for nframes frames of npix > 0 paths each.  target_opt: option wf_paths, or
// kWfTargetPaths when it is unset (forced: it is set).
struct WfBatchSize { uint64_t want, floor; };
constexpr WfBatchSize wf_batch_size(uint64_t npix, uint32_t nframes, long target_opt, bool forced) {
    // the target in whole pairs of frames (a batch's two parts take whole frames each): 4096^2
    // holds 4 frames (67 M paths), not 2 of the 3.8 that 64 M would hold
    const uint64_t target0 = (uint64_t)std::max(1L, target_opt);  // A/B
    const uint64_t pairs = (target0 + 2 * npix - 1) / (2 * npix) * (2 * npix);
    const uint64_t target = forced || pairs > 0x7fffffffull ? target0 : pairs;
    // at least two frames per batch when the call has two (images above the target, e.g.
    // 4096^2): the batch's parts run on their own streams and overlap (+29 % at 4096^2)
    const uint64_t all = npix * nframes;
    const uint64_t two = 2 * npix <= 0x7fffffffull ? 2 * npix : npix;
    // a call that fits the target runs as one batch: its two parts take whole frames each, so
    // an odd frame count gets one frame of room more (5 frames: 3 + 2, not batches of 4 and 1)
    const uint64_t all_even = nframes > 1 && (nframes & 1) ? all + npix : all;
    return {std::max<uint64_t>(std::min<uint64_t>(all, two), std::min<uint64_t>(all_even, target)),
            std::min<uint64_t>(all, npix)};
}
// queue arrays carry slack so that each part can be cut into up to kRegions regions of a whole
// number of 64-entry batches holding all its paths (k_wf_step_bf)
constexpr size_t wf_queue_entries(size_t capacity) { return capacity + 2 * (size_t)kQueueSlackRegions * 64; }

// ---- parts and frames per batch ----

// The batch in `parts` parts on as many streams when a part holds at least a frame: one
// part's kernel fills the others' launch tails and boundaries (and, with separate trace and
// shade kernels, a VALU-bound trace runs beside an HBM-bound shade).  Halved while a part would hold
// less than a frame (so parts = 3 falls to 1).
constexpr int wf_parts(bool dual, int parts, bool streams, uint32_t nframes, uint32_t capacity, uint32_t npix) {
    int np = dual && streams ? std::max(1, std::min(kMaxParts, parts)) : 1;
    while (np > 1 && (nframes < (uint32_t)np || capacity / np < npix)) np /= 2;
    return np;
}
// frames per batch
constexpr uint32_t wf_batch_frames(int np, uint32_t nframes, uint32_t capacity, uint32_t npix) {
    return np * std::max<uint32_t>(1, std::min<uint32_t>((nframes + np - 1) / np, (uint32_t)(capacity / np / npix)));
}
// Part h of np of a batch: its frames f0 .. f0 + frames of the batch, its paths, and where its state
// starts — queue entries from h * (qcap / np), radiance from rad_off floats (so the parts' radiance is
// contiguous in frame order), control words from h * WF_CTL_WORDS, region counts from h * 3 * kRegions
// (h = the part's index in WfBatchPlan::part) — with the capacity and queue entries of one part.
struct WfPartPlan {
    uint32_t f0, frames, paths;
    size_t rad_off, entry_off;
    uint32_t capacity, qcap;
};
struct WfBatchPlan {
    int n;
    WfPartPlan part[kMaxParts];
};
// frames of a batch of Fb dealt to the parts in contiguous runs
constexpr WfBatchPlan wf_deal(uint32_t Fb, int np, uint32_t npix, uint32_t capacity, uint32_t qcap) {
    WfBatchPlan b = {};
    uint32_t f0 = 0;
    for (int h = 0; h < np && f0 < Fb; ++h) {
        const uint32_t fh = std::min<uint32_t>((Fb + np - 1) / np, Fb - f0);
        WfPartPlan& p = b.part[b.n++];
        p.f0 = f0;
        p.frames = fh;
        p.paths = fh * npix;
        p.rad_off = (size_t)f0 * npix * 3;
        p.entry_off = (size_t)h * (qcap / np);
        p.capacity = capacity / np;
        p.qcap = qcap / np;
        f0 += fh;
    }
    return b;
}

// ---- regions of the fused kernel (k_wf_step_bf) ----

// R regions for a grid of `blocks` blocks of waves_per_block waves, and the permutation (q, qi):
// region_perm: region r takes camera batches r q mod R (q ~ 0.618 R, coprime with R), so
// the 8 waves of a block (8 neighbouring regions) work on batches far apart in the image
struct WfRegions { uint32_t R, q, qi; };
constexpr WfRegions wf_regions(int blocks, uint32_t waves_per_block, bool region_perm) {
    const uint32_t R = std::min<uint32_t>(kRegions, (uint32_t)blocks * waves_per_block);
    uint32_t q = 1, qi = 1;
    if (region_perm && R > 2) {
        auto gcd = [](uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; };
        // (at least 2: floor(0.618 R) is 1 at R = 3 alone, where q = 1 would be the identity; no grid has 3
        // regions — R is a multiple of the block's waves — and every other R keeps its q)
        q = std::max<uint32_t>(2, (uint32_t)(R * 0.6180339887498949));
        while (gcd(q, R) != 1) ++q;
        qi = 1;
        while ((uint64_t)q * qi % R != 1) ++qi;  // R <= 512
    }
    return {R, q, qi};
}
// entries per region of a part: R * rstride >= paths of the part (qcap slack)
constexpr uint32_t wf_region_stride(uint32_t part_qcap, uint32_t R) { return part_qcap / R / 64 * 64; }

// ---- streaming regeneration (option regen; fused kernel, camera paths made in the kernel) ----

// q camera batches per region admitted by each extension launch (0: the plain first launch); cam = the
// most camera batches of any region; iters: the launches per part of the batch
struct WfRegen { uint32_t q, cam; int iters; };
constexpr WfRegen wf_regen(bool fgen, int regen, const WfBatchPlan& b, uint32_t R, int max_depth) {
    WfRegen g = {0, 0, 2 * (max_depth + 1)};
    if (fgen && regen > 0) {
        for (int h = 0; h < b.n; ++h) {
            const uint32_t nbat = (b.part[h].paths + 63) / 64;
            g.cam = std::max(g.cam, (nbat + R - 1) / R);
        }
        g.q = (uint32_t)regen;
        if (g.q < g.cam)  // J admitting launches, the last admission's paths need max_depth + 1 more
            g.iters = 2 * ((int)((g.cam + g.q - 1) / g.q) + max_depth);
        else
            g.q = 0;  // one launch admits them all: the plain first launch
    }
    return g;
}
// What launch `it` of a part is.  Odd launches read the shadow queue; an even one reads the extension
// queue and is plain, the fused kernel's first launch that makes every camera path (GEN 1), or one that
// admits the next q camera batches per region behind its queued survivors (GEN 2).  The first three are
// k_wf_step_bf's GEN values.
enum WfStepKind : int { WF_STEP_EXT = 0, WF_STEP_GEN = 1, WF_STEP_ADMIT = 2, WF_STEP_SHADOW = 3 };
constexpr WfStepKind wf_step_kind(const WfRegen& g, bool fgen, int it) {
    if (g.q > 0 && (it & 1) == 0 && (uint32_t)(it / 2) * g.q < g.cam) return WF_STEP_ADMIT;
    if (fgen && it == 0) return WF_STEP_GEN;
    return (it & 1) == 0 ? WF_STEP_EXT : WF_STEP_SHADOW;
}

// ---- small clamps ----

// option sort: the shade kernel's coherence keys, 0 (off), 8, 64 or 512
constexpr int wf_sort_bins(int sort) { return sort > 0 ? (sort >= 512 ? 512 : sort >= 64 ? 64 : 8) : 0; }
constexpr int wf_trace_sparse(int trace_sparse) { return std::max(0, std::min(trace_sparse, 1 << 20)); }
// option bf_slots < kBfSlots: tests of the recompute path
constexpr int wf_bf_slots(int bf_slots) { return std::min(kBfSlots, bf_slots); }
// k_wf_trace's instance: the 256-entry hit ring when its extra 8 KB per block cost no block per
// CU (option trace_ring: 128 / 256 forces one).  lds_big: the block's LDS with the large ring; max_lds:
// the block limit; occ_big, occ_small: the resident blocks of the two instances, read only when
// wf_ring_by_occupancy says the choice is theirs (the caller need not ask the runtime otherwise).
constexpr bool wf_ring_by_occupancy(int trace_ring, size_t lds_big, size_t max_lds) {
    return lds_big <= max_lds && trace_ring != (int)kHitRingMax && trace_ring <= 0;
}
constexpr uint32_t wf_ring(int trace_ring, size_t lds_big, size_t max_lds, int occ_big, int occ_small) {
    const bool fits = lds_big <= max_lds && (trace_ring == (int)kHitRingMax || (trace_ring <= 0 && occ_big >= occ_small));
    return fits ? kHitRingMax : kHitRing;
}

}  // namespace pt
