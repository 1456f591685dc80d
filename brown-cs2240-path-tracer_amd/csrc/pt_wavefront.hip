// pt_wavefront.hip — wavefront path tracer for gfx950 (the north-star design).
//
// A batch of P = F*W*H paths (F frames of the image) lives in HBM as DENSE queues of
// entries that carry the ray AND the path state (WfQueue, pt_kernels.h: 64 B per entry,
// +40 B of shading point in the shadow queue).  Survivors are compacted into the other
// queue every iteration, so every kernel streams its queue coalesced and nothing is
// gathered by path index (the radiance of a finished path is the only scatter).  Each
// iteration runs:
//   k_wf_trace   closest-hit traversal of the queue.  Persistent waves, each owning a
//                contiguous chunk of the queue (no atomics).  Rays arrive in LDS windows of
//                32 records (the next window in flight in registers) and hits leave through
//                an LDS ring written back one coalesced window at a time, so the traversal
//                loop issues no global memory operation; a lane takes its next ray the
//                moment its traversal ends.  Traversal is trav_step_lean (per-lane stack in
//                LDS, scene in LDS when it fits).
//   k_wf_shade   the path logic after that traversal (path_after_ext / path_after_shadow,
//                pt_path.h) and compaction of the surviving paths into the next queue with
//                __ballot + mbcnt (one atomicAdd per wave).
// All paths of a batch start together, so a queue holds only extension rays or only
// shadow rays and the two alternate.  k_wf_generate writes the camera rays; k_wf_accum adds
// the batch's finished radiance into the accumulator in frame order, which keeps the result
// bit-identical to the reference's host accumulation.
//
// This unit is the driver alone, launch_wavefront: host code that knows no kernel's template parameters.
// The arithmetic of a call — parts, frames per batch, regions, regeneration, clamps — is pt_wf_plan.h's;
// the kernels live by stage in pt_wf_source.hip (generate, accumulate), pt_wf_trace.hip (k_wf_trace),
// pt_wf_bf.hip (the brute-force and fused step kernels) and pt_wf_shade.hip, over the entry helpers of
// pt_wf_queue.h, and reach the driver through pt_wf_stage.h.
#include "pt_occupancy.h"
#include "pt_path.h"  // GATHER_*, CAM_*
#include "pt_wf_stage.h"

namespace pt {

// Part h of a batch as the plan cuts it (WfPartPlan): queue entries from p.entry_off, radiance from
// p.rad_off floats, control words from h * WF_CTL_WORDS, region counts from h * 3 * kRegions.
static WfBuffers wb_part(const WfBuffers& wb, int h, const WfPartPlan& p) {
    WfBuffers v = wb;
    const size_t e = p.entry_off;
    for (WfQueue* q : {&v.ext, &v.shd}) { q->ray += 2 * e; q->q2 += e; q->q3 += e; }
    v.sp0 += e; v.sp1 += e; v.sp2 += e; v.hitq += e;
    if (v.pres) v.pres += e;  // per leaf b at b * pres_stride (the whole buffer's stride)
    v.rad += p.rad_off;
    v.ctl += h * WF_CTL_WORDS;
    v.rcnt += h * 3 * kRegions;
    v.capacity = p.capacity;
    v.qcap = p.qcap;
    return v;
}

// what a PathSource's making cannot rule out (pt_kernels.h)
static bool source_ok(const PathSource& src, bool accum, uint32_t stride) {
    if ((src.kind != PathSource::WINDOW || src.m2) && !accum) return false;
    if (src.cam && (src.cam->model < CAM_THIN_LENS || src.cam->model > CAM_EQUIRECT)) return false;
    switch (src.kind) {
        case PathSource::WINDOW: return true;
        case PathSource::RECTS: return src.rects.n != 0 && src.rects.npix != 0;
        case PathSource::RAYS: return stride == 1 && src.rays.n != 0;
        case PathSource::GATHER: return stride == 1 && src.gather.n != 0 && src.gather.mode <= GATHER_SH9;
        case PathSource::VIEWS: return src.views.n != 0 && src.views.npix != 0;
    }
    return false;
}

hipError_t launch_wavefront(const LaunchOpts& lo, const SceneView& sc, const FrameParams& fp, const WfBuffers& wb,
                            const PathSource& src, uint32_t frame0, uint32_t nframes, uint32_t stride, bool accum,
                            bool count, float* out, Counters* cnt, hipStream_t stream, const WfStreams& ws) {
    if (!source_ok(src, accum, stride)) return hipErrorInvalidValue;
    if (!accum) { nframes = 1; stride = 1; }
    const bool lds = lo.lds && scene_fits_lds(sc);
    // the leaf pass (FLV_PRE) when the scene's table of pre-resolved leaves holds its big leaves
    // (pt_capi.hip shape_view: option leaf_pre, default on) and the buffers exist
    const int trav = select_wavefront(lo, sc.fast_rcp != 0, sc.mailbox != 0, sc.big_leaf > 0, sc.npre > 0 && sc.pre && wb.pres);
    // the flavour's trace (or trace + shade) stage, from the unit that owns its kernels; sg.sc: the scene
    // with that unit's per-instance defaults (sc.node_bias <= 0: chosen there)
    WfStage sg;
    if (!(flv_brute_force(trav) ? bf_stage(trav, lds, count, sc, sg) : trace_stage(trav, lds, count, sc, lo, sg)))
        return hipErrorInvalidValue;
    const uint32_t npix = src.paths_per_frame(fp);
    // the fused kernel's first launch makes the camera paths itself (GEN)
    const bool fgen = sg.fused && src.fused_gen(lo);
    const int np = wf_parts(lo.dual, lo.parts, ws.aux[0] != nullptr, nframes, wb.capacity, npix);
    const uint32_t F = wf_batch_frames(np, nframes, wb.capacity, npix);
    int tblocks = occupancy_blocks(sg.kernel, kTraceBlock, sg.lds);
    if (lo.trace_blocks > 0) tblocks = std::min(tblocks, lo.trace_blocks);  // option wf_trace_blocks (tests)
    // option trace_watchdog: tests of the failure report
    const WfCall c{fp, lo, frame0, stride, accum, cnt, tblocks, lo.watchdog > 0 ? lo.watchdog : kTraceWatchdog,
                   wf_trace_sparse(lo.trace_sparse), wf_bf_slots(lo.bf_slots)};
    const int sort_bins = wf_sort_bins(lo.sort);
    // region-partitioned queues (k_wf_step_bf)
    const WfRegions rg = sg.fused ? wf_regions(tblocks, kTraceBlock / 64, lo.region_perm) : WfRegions{0, 1, 1};
    if (fgen)  // the camera batches' table (k_wf_camtab), before every part's GEN launch
        HIP_RETURN_IF(launch_camtab(sg.sc, fp, wb.camtab, stream));
    for (uint32_t fb = 0; fb < nframes; fb += F) {
        const uint32_t Fb = std::min(F, nframes - fb);
        // frames of the batch dealt to the parts in contiguous runs (part h: frames fb + f0 ..)
        const WfBatchPlan bp = wf_deal(Fb, np, npix, wb.capacity, wb.qcap);
        const int nh = bp.n;
        WfPart pv[kMaxParts];
        for (int h = 0; h < nh; ++h) {
            pv[h].w = np > 1 ? wb_part(wb, h, bp.part[h]) : wb;
            pv[h].fbase = fb + bp.part[h].f0;
            pv[h].P = bp.part[h].paths;
            pv[h].st = np > 1 ? ws.aux[h] : stream;
            if (sg.fused) {
                pv[h].w.nreg = rg.R;
                pv[h].w.rstride = wf_region_stride(pv[h].w.qcap, rg.R);
                pv[h].w.rq = rg.q;
                pv[h].w.rqi = rg.qi;
            }
        }
        // the fused kernel's GEN launch appends into count slot 1, zeroed here (k_wf_generate zeroes it
        // otherwise), and a compacting generate kernel into the queue's count or the regions' count slots 0,
        // zeroed here with slot 1 (as k_wf_generate would have set them) — on the caller's stream
        // before the fork: on a part's stream the second part's memset waited ~0.5 ms for a CU slot
        // behind the first part's first launch, and the parts ran that far apart (a kernel trace of
        // the bench, r06m)
        if (fgen)
            for (int h = 0; h < nh; ++h)
                HIP_RETURN_IF(hipMemsetAsync(pv[h].w.rcnt + kRegions, 0, kRegions * sizeof(uint32_t), stream));
        if (src.compacts())
            for (int h = 0; h < nh; ++h) {
                HIP_RETURN_IF(hipMemsetAsync(pv[h].w.ctl + WF_COUNT0, 0, 2 * sizeof(uint32_t), stream));
                if (sg.fused) HIP_RETURN_IF(hipMemsetAsync(pv[h].w.rcnt, 0, 2 * kRegions * sizeof(uint32_t), stream));
            }
        if (np > 1) {
            HIP_RETURN_IF(hipEventRecord(ws.fork, stream));
            for (int h = 0; h < nh; ++h) HIP_RETURN_IF(hipStreamWaitEvent(pv[h].st, ws.fork, 0));
        }
        const WfRegen regen = wf_regen(fgen, lo.regen, bp, rg.R, fp.max_depth);
        for (int h = 0; h < nh && !fgen; ++h) launch_generate(src, c, pv[h], count);
        for (int it = 0; it < regen.iters; ++it) {
            for (int h = 0; h < nh; ++h) {
                HIP_RETURN_IF(sg.launch(sg, c, pv[h], it, wf_step_kind(regen, fgen, it), regen.q));
                if (!sg.fused) launch_shade(sg.sc, c, pv[h], it, count, sort_bins);
            }
            // a launch that cannot run (e.g. a configuration error) fails here, after the first
            // iteration, instead of leaving the later launches to read counts it never wrote
            if (it == 0) HIP_RETURN_IF(hipGetLastError());
        }
        if (np > 1) {
            for (int h = 0; h < nh; ++h) {
                HIP_RETURN_IF(hipEventRecord(ws.join[h], pv[h].st));
                HIP_RETURN_IF(hipStreamWaitEvent(stream, ws.join[h], 0));
            }
        }
        launch_accum(src, fp, wb.rad, npix, frame0 + fb, Fb, accum, out, stream);
    }
    return hipGetLastError();
}

}  // namespace pt
