// pt_wf_stage.h — what the wavefront's kernel units export to its driver (launch_wavefront,
// pt_wavefront.hip): plain launch functions, and for the trace / step kernels a WfStage — a few numbers
// and one launch function — so that the driver never names a kernel's template parameters.  Host only.
#pragma once
#include "pt_kernels.h"

namespace pt {

#define HIP_RETURN_IF(expr)                      \
    do {                                         \
        const hipError_t e_ = (expr);            \
        if (e_ != hipSuccess) return e_;         \
    } while (0)

constexpr uint32_t kTraceBlock = 512;  // 8 waves share one LDS copy of the scene
// Shade blocks are 1024 threads so that compaction takes one atomicAdd per 1024 entries: all
// atomics on the queue counter serialise at one memory channel, and one per wave (131k per
// 8M-path batch) cost more than the shading itself.
constexpr uint32_t kShadeBlock = 1024;

// one part of a batch: its buffers, first frame, paths and stream
struct WfPart { WfBuffers w; uint32_t fbase, P; hipStream_t st; };

// what every launch of a call shares
struct WfCall {
    const FrameParams& fp;
    const LaunchOpts& lo;
    uint32_t frame0, stride;
    bool accum;
    Counters* cnt;
    int blocks;         // the persistent grid of the trace and step kernels
    uint32_t watchdog;  // k_wf_trace: iterations before a wave gives up
    int sparse, bf_slots;
};

// The trace (or fused trace + shade) stage of a call's flavour, made by the unit that owns the
// flavour's kernels.
struct WfStage {
    SceneView sc;        // the scene as the stage's (and the shade) kernels take it
    bool fused;          // launch() shades as well: no k_wf_shade, regions in the queues
    const void* kernel;  // the occupancy of this instance at `lds` sizes the persistent grid
    size_t lds;          // dynamic LDS of the stage's launches
    // launch `it` of a part (kind: wf_step_kind, pt_wf_plan.h; regen_q: WfRegen::q of the batch)
    hipError_t (*launch)(const WfStage& sg, const WfCall& c, const WfPart& pt, int it, WfStepKind kind, uint32_t regen_q);
    uint32_t ring;       // the owning unit's choice of instance: k_wf_trace's hit ring and pooled runs of 2,
    bool run2, narrow;   // the fused kernel's 32-bit sets
};
// false: not a flavour of the unit's, or not instantiated (PT_WF_FLAVOURS)
bool trace_stage(int trav, bool lds, bool count, const SceneView& sc, const LaunchOpts& lo, WfStage& sg);  // pt_wf_trace.hip
bool bf_stage(int trav, bool lds, bool count, const SceneView& sc, WfStage& sg);                           // pt_wf_bf.hip
// the camera batches' table (k_wf_camtab) for the fused kernel's GEN launches; mailbox scenes: <= 64 entries
hipError_t launch_camtab(const SceneView& sc, const FrameParams& fp, float4* camtab, hipStream_t stream);  // pt_wf_bf.hip

// k_wf_shade after launch `it` of a part (pt_wf_shade.hip)
void launch_shade(const SceneView& sc, const WfCall& c, const WfPart& pt, int it, bool count, int sort_bins);

// A part's first-vertex paths, and a batch's radiance (Fb frames of npix paths; sbase: the call's sample
// index of the first) added to `out`, by the source's kind (pt_wf_source.hip; the table in pt_kernels.h)
void launch_generate(const PathSource& src, const WfCall& c, const WfPart& pt, bool count);
void launch_accum(const PathSource& src, const FrameParams& fp, const float* rad, uint32_t npix, uint32_t sbase, uint32_t Fb,
                  bool accum, float* out, hipStream_t stream);

}  // namespace pt
