// Stand-alone driver of the wavefront call's plan (csrc/pt_wf_plan.h): batch size, parts and frames per
// batch, the fused kernel's regions, streaming regeneration and the small clamps.  Standard C++, no GPU, no
// library; the header alone.
//
// usage: wf_plan_harness < COMMANDS   -> one line of integers per command line
// (tests/test_wf_plan_cpu.py restates the formulas and checks the invariants):
//   batch NPIX NFRAMES TARGET FORCED                      -> want floor queue_entries(want)
//   deal DUAL PARTS STREAMS NFRAMES CAPACITY NPIX QCAP    -> np F, then per batch "B fb Fb n" and per part
//                                                            "P f0 frames paths rad_off entry_off capacity qcap"
//   regions BLOCKS WAVES_PER_BLOCK PERM PART_QCAP         -> R q qi rstride
//   regen FGEN REGEN R MAX_DEPTH PATHS...                 -> q cam iters, then the kind of each launch
//   clamps SORT TRACE_SPARSE BF_SLOTS                     -> sort_bins trace_sparse bf_slots
//   ring OPT LDS_BIG MAX_LDS OCC_BIG OCC_SMALL            -> by_occupancy ring
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pt_wf_plan.h"

using namespace pt;

// a few facts at compile time: the default call of two samples, and parts = 3
static_assert(wf_batch_size(1 << 20, 2, (long)kWfTargetPaths, false).want == 2u << 20, "two frames: one batch");
static_assert(wf_parts(true, 2, true, 2, 2u << 20, 1 << 20) == 2 && wf_batch_frames(2, 2, 2u << 20, 1 << 20) == 2, "two parts");
static_assert(wf_parts(true, 3, true, 16, 1u << 24, 1 << 20) == 3 && wf_parts(true, 3, true, 2, 1u << 24, 1 << 20) == 1, "3 -> 1");
static_assert(wf_regions(1024, 8, false).R == kRegions && wf_regions(2, 8, true).R == 16, "R = min(kRegions, waves)");
static_assert(wf_sort_bins(63) == 8 && wf_sort_bins(64) == 64 && wf_sort_bins(1 << 20) == 512 && wf_sort_bins(-1) == 0, "");

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        std::vector<long long> a;
        for (long long v; in >> v;) a.push_back(v);
        auto need = [&](size_t n) {
            if (a.size() >= n) return true;
            std::fprintf(stderr, "too few arguments: %s\n", line.c_str());
            return false;
        };
        if (cmd == "batch") {
            if (!need(4)) return 2;
            const WfBatchSize b = wf_batch_size((uint64_t)a[0], (uint32_t)a[1], (long)a[2], a[3] != 0);
            std::printf("%" PRIu64 " %" PRIu64 " %zu\n", b.want, b.floor, wf_queue_entries((size_t)b.want));
        } else if (cmd == "deal") {
            if (!need(7)) return 2;
            const uint32_t nframes = (uint32_t)a[3], cap = (uint32_t)a[4], npix = (uint32_t)a[5], qcap = (uint32_t)a[6];
            const int np = wf_parts(a[0] != 0, (int)a[1], a[2] != 0, nframes, cap, npix);
            const uint32_t F = wf_batch_frames(np, nframes, cap, npix);
            std::printf("%d %u", np, F);
            for (uint32_t fb = 0; fb < nframes; fb += F) {
                const uint32_t Fb = std::min(F, nframes - fb);
                const WfBatchPlan b = wf_deal(Fb, np, npix, cap, qcap);
                std::printf(" B %u %u %d", fb, Fb, b.n);
                for (int h = 0; h < b.n; ++h) {
                    const WfPartPlan& p = b.part[h];
                    std::printf(" P %u %u %u %zu %zu %u %u", p.f0, p.frames, p.paths, p.rad_off, p.entry_off, p.capacity, p.qcap);
                }
            }
            std::printf("\n");
        } else if (cmd == "regions") {
            if (!need(4)) return 2;
            const WfRegions r = wf_regions((int)a[0], (uint32_t)a[1], a[2] != 0);
            std::printf("%u %u %u %u\n", r.R, r.q, r.qi, wf_region_stride((uint32_t)a[3], r.R));
        } else if (cmd == "regen") {
            if (!need(5) || a.size() > 4 + (size_t)kMaxParts) return 2;
            WfBatchPlan b = {};
            for (size_t k = 4; k < a.size(); ++k) b.part[b.n++].paths = (uint32_t)a[k];
            const bool fgen = a[0] != 0;
            const WfRegen g = wf_regen(fgen, (int)a[1], b, (uint32_t)a[2], (int)a[3]);
            std::printf("%u %u %d", g.q, g.cam, g.iters);
            for (int it = 0; it < g.iters; ++it) std::printf(" %d", (int)wf_step_kind(g, fgen, it));
            std::printf("\n");
        } else if (cmd == "clamps") {
            if (!need(3)) return 2;
            std::printf("%d %d %d\n", wf_sort_bins((int)a[0]), wf_trace_sparse((int)a[1]), wf_bf_slots((int)a[2]));
        } else if (cmd == "ring") {
            if (!need(5)) return 2;
            std::printf("%d %u\n", wf_ring_by_occupancy((int)a[0], (size_t)a[1], (size_t)a[2]) ? 1 : 0,
                        wf_ring((int)a[0], (size_t)a[1], (size_t)a[2], (int)a[3], (int)a[4]));
        } else if (!cmd.empty()) {
            std::fprintf(stderr, "unknown command: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
