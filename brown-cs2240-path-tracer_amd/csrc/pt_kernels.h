// pt_kernels.h — launch wrappers between the C-ABI layer (pt_capi.cpp) and the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "pt_device.h"
#include "pt_flavour.h"
#include "pt_query_plan.h"
#include "pt_rect_plan.h"
#include "pt_step_addr.h"

// ids for k_selftest_math (also used by pt_selftest_math in the C-ABI)
enum {
    PT_MATH_SIN = 0, PT_MATH_COS, PT_MATH_TAN, PT_MATH_ACOS, PT_MATH_LOG2, PT_MATH_EXP2, PT_MATH_POW, PT_MATH_SQRT,
    PT_MATH_DIV, PT_MATH_HASH1U, PT_MATH_HASH1, PT_MATH_HASH2X, PT_MATH_HASH2Y, PT_MATH_MIN, PT_MATH_MAX, PT_MATH_RAY_INV, PT_MATH_COUNT_
};

namespace pt {

// Kernel timing (pt_profile_enable / pt_profile_read): while a profiler is attached to the
// calling thread, every launch is bracketed by two HIP events on its stream.
enum KernelId : int {
    KID_MEGA = 0, KID_REGEN, KID_WF_GENERATE, KID_WF_TRACE, KID_WF_SHADE_EXT, KID_WF_SHADE_SHADOW, KID_WF_ACCUM,
    KID_TONEMAP, KID_WF_STEP, KID_WF_LEAF, KID_NOISE_TILES, KID_TILE_MEAN, KID_FEATURES, KID_DENOISE_PREPARE, KID_ATROUS,
    KID_QUERY_HITS, KID_QUERY_OCCLUDED, KID_CAMERA_RAYS, KID_COUNT
};
inline const char* kernel_name(int k) {
    static const char* const n[KID_COUNT] = {"k_mega",         "k_regen",           "k_wf_generate", "k_wf_trace",
                                             "k_wf_shade_ext", "k_wf_shade_shadow", "k_wf_accum",    "k_tonemap",
                                             "k_wf_step",      "k_wf_leafpass",     "k_noise_tiles", "k_tile_mean",
                                             "k_features",     "k_denoise_prepare", "k_atrous",      "k_query_hits",
                                             "k_query_occluded", "k_camera_rays"};
    return (k >= 0 && k < KID_COUNT) ? n[k] : "?";
}
struct KernelProfiler {
    struct Rec { int kid; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    int only = -1;  // record only this kernel id (pt_profile_select); -1 = all
    bool open = false;  // the last start() recorded (stop() closes it)
    hipEvent_t take();
    void start(int kid, hipStream_t s);
    void stop(hipStream_t s);
    void reset();    // records' events go back to the pool
    void destroy();  // frees every event
};
extern thread_local KernelProfiler* t_prof;
#define PT_LAUNCH(KID, STREAM, ...)                                  \
    do {                                                             \
        ::pt::KernelProfiler* p_ = ::pt::t_prof;                     \
        if (p_ && p_->only >= 0 && p_->only != (KID)) p_ = nullptr;  \
        if (p_) p_->start((KID), (STREAM));                          \
        hipLaunchKernelGGL(__VA_ARGS__);                             \
        if (p_) p_->stop(STREAM);                                    \
    } while (0)

constexpr int kMegaBlock = 256;
// dynamic LDS a workgroup may use for traversal stacks + a staged scene copy
constexpr size_t kLdsSceneBudget = 64 * 1024;

// LaunchOpts (the per-call options, with their defaults): pt_flavour.h
bool scene_fits_lds(const SceneView& sc);

// Wavefront path state (HBM), `capacity` entries per queue; see pt_wavefront.hip.  Every
// path's state travels with its ray: queue entry i holds the ray AND the path state, and
// a shade kernel writes the surviving path to its compacted slot of the other queue, so no
// kernel gathers by path index.  Iterations alternate extension / shadow queues.
enum { WF_COUNT0 = 0, WF_COUNT1 = 1, WF_WATCHDOG = 2, WF_SNAP_CLAIM = 3, WF_RING = 4, WF_SNAP = 8, WF_SNAP_WORDS = 16, WF_CTL_WORDS = 64 };
// the control block holds WF_CTL_WORDS words per half of a dual-stream batch (wb_half)
// iterations after which a trace wave gives up: it sets ctl[WF_WATCHDOG], the first such wave
// leaves its scheduling state in ctl[WF_SNAP..], and the host reports an error
constexpr uint32_t kTraceWatchdog = 1u << 24;
constexpr uint64_t kTraceWatchdogTicks = 500000000ull;  // 5 s of wall_clock64 (100 MHz)
struct WfQueue {
    float4* ray;  // [i][2]: (o.xyz, d.x), (d.y, d.z, path index bits, depth | spec << 16)
    float4* q2;   // (L.xyz, seed bits)
    float4* q3;   // (beta.xyz, -)
};
struct WfBuffers {
    WfQueue ext;   // extension rays (queue 0)
    WfQueue shd;   // shadow rays (queue 1) ...
    float4* sp0;   // ... and their shading points: (hp.xyz, material id)
    float4* sp1;   // (hn.xyz, wi.x)
    float2* sp2;   // (wi.y, wi.z)
    int2* hitq;    // per queue entry: (leaf record, t bits)
    float* rad;    // per path: radiance when it ended [capacity][3]
    uint32_t* ctl; // queue counts
    uint32_t capacity;  // paths per batch
    uint32_t qcap;      // entries per queue array (capacity + slack for the region layout)
    // region-partitioned queues of the fused kernel (k_wf_step_bf): region r of a queue holds
    // entries [r * rstride, r * rstride + count_r); rcnt[slot * kRegions + r] = count_r for
    // the three rotating count slots
    uint32_t* rcnt;
    uint32_t rstride;
    uint32_t nreg;
    // camera batch j of the fused kernel's regions goes to region (j mod nreg) * rqi mod nreg, so
    // region r holds the batches j = r * rq mod nreg (+ k nreg) (rq * rqi = 1 mod nreg; option
    // region_perm; 1, 1: j mod nreg, neighbouring regions — one block's waves — take neighbouring
    // batches)
    uint32_t rq, rqi;
    uint64_t rad_cap;   // paths whose radiance `rad` holds (>= capacity)
    // big leaves resolved before the traversal (k_wf_leafpass): per leaf b and queue entry i the
    // key (f32 bits of t << 32 | position; ~0: no hit) at pres[b * pres_stride + i] (pres_stride = the
    // whole buffer's qcap: a part's pres is offset like its queues); nullptr when the scene has none
    uint64_t* pres;
    uint32_t pres_stride;
    // per distinct entry, the camera-origin parts of the triangle test (k_wf_camtab; 2 x 64 float4)
    float4* camtab;
};
constexpr uint32_t kRegions = 512;
// queue slack (entries per part = 64 * this): regions of R <= kRegions hold ceil(batches / R)
// 64-entry batches each
constexpr uint32_t kQueueSlackRegions = 4096;
constexpr size_t kWfBytesPerPath = 64 + 64 + 40 + 8 + 12;

// The wavefront's parts: streams owned by the scene, created back to back so that HIP's
// round-robin stream -> hardware-queue mapping puts them on different queues (a shared queue
// serialises the parts), plus fork/join events with the caller's stream.  Null = one stream.
constexpr int kMaxParts = 4;  // parts of a wavefront batch on their own streams (LaunchOpts::parts)
struct WfStreams {
    hipStream_t aux[kMaxParts] = {};
    hipEvent_t fork = nullptr, join[kMaxParts] = {};
};
// A rectangle list on the device (pt_render_rects; pt_rect_plan.h): the third slot -> pixel map beside
// the window's two (slot_path, pixel_of).  A list render's FrameParams window is the call's frame: a
// pixel (x, y) of a rectangle is stored at out + 3 * ((y - win_y0) * row_pitch + (x - win_x0)).
struct RectList {
    const RectRow* rows;      // n, list order
    const RectBlock* blocks;  // the megakernel's grid, one entry per 16 x 16 block (nullptr: a wavefront render)
    uint32_t n, npix;         // rectangles, pixels per frame
    uint32_t nblocks;
    uint32_t fx0, fy0;        // the frame's origin (FrameParams::win_x0, win_y0)
};
// rl (nullable, accumulating calls): the call renders the rectangles of the list instead of fp's
// window — paths per frame rl->npix, camera paths by k_wf_generate's list instance (whatever
// lo.fuse_gen and lo.regen say), k_wf_accum's list instance
hipError_t launch_wavefront(const LaunchOpts& lo, const SceneView& sc, const FrameParams& fp, const WfBuffers& wb,
                            uint32_t frame0, uint32_t nframes, uint32_t stride, bool accum, bool count, float* out,
                            Counters* cnt, hipStream_t stream, const WfStreams& ws, float* m2 = nullptr,
                            const RectList* rl = nullptr);

// set width (32 / 64 bits) of the stackless replay in the fused kernel launched last in this process
// (0: none yet, or the stack walk) — pt_last_bf_width, for the tests of the narrow instance
int last_bf_width();
// offset width (32 / 64 bits) of the queue addressing in the fused kernel launched last in this process
// (0: none yet) — pt_last_step_addr, for the tests of the 64-bit instance
int last_step_addr();

// Megakernel render (accum=true: frames frame0 + i*stride, i < nframes, added to out) or one
// dispatch (accum=false: raw radiance of salt frame0 written to out).  m2 (accum only, as in
// launch_wavefront): the second moments, m2 += clamp(L)^2 per frame, laid out like out.
// rl (nullable, accum only): the rectangles of the list instead of fp's window, a grid of rl->nblocks blocks.
hipError_t launch_megakernel(const LaunchOpts& lo, const SceneView& sc, const FrameParams& fp, uint32_t frame0,
                             uint32_t nframes, uint32_t stride, bool accum, bool count, float* out, Counters* cnt,
                             hipStream_t stream, float* m2 = nullptr, const RectList* rl = nullptr);

// display transform of program-raymarch.ts:295-316 on device (pt_image.hip)
hipError_t launch_tonemap(const float* acc, size_t npix, uint32_t runs, uint8_t* rgba, hipStream_t stream);
// per-tile noise verdicts from the two accumulators, and the per-tile mean (pt_image.hip; pt_hip.h
// pt_noise_tiles_async, pt_tile_mean_async)
struct TileGrid { uint32_t w, h, row_pitch, tile_w, tile_h, tx, ty; };  // tx, ty: tiles across and down
struct TileNoise { uint32_t noisy, pixels; double max_err; };              // pt_hip.h pt_tile_noise
hipError_t launch_noise_tiles(const float* acc, const float* m2, const TileGrid& g, const uint32_t* frames, double tol,
                              double floor, TileNoise* out, hipStream_t stream);
hipError_t launch_tile_mean(const float* acc, const TileGrid& g, const uint32_t* frames, float* mean, hipStream_t stream);
// guide buffers of the first hit (pt_features.hip; pt_hip.h pt_render_features_async): geo += (n, t),
// alb += (albedo, 1) per frame and hit, four floats per pixel, rows fp.row_pitch pixels apart
hipError_t launch_features(const SceneView& sc, const FrameParams& fp, uint32_t frame0, uint32_t nframes, uint32_t stride,
                           bool count, float* geo, float* alb, Counters* cnt, hipStream_t stream);
// the a-trous denoiser (pt_denoise.hip; pt_hip.h pt_denoise_async).  prepare: the accumulators and the
// guides (g: the tile grid of frames, g.row_pitch the pitch of all four inputs) -> three dense planes
// of g.w * g.h float4: cv (c.rgb, var), nz (N.xyz, Z), ab (A.rgb, 0).  atrous: one pass with step s
// from cv to cv_out (nullable) and, the last pass, to out [h][w][3] and var_out (nullable) [h][w],
// rows row_pitch pixels apart; staged: the block's region through LDS (atrous_can_stage(s)), same bits.
hipError_t launch_denoise_prepare(const float* acc, const float* m2, const float* geo, const float* alb, const TileGrid& g,
                                  const uint32_t* frames, uint32_t feature_frames, float4* cv, float4* nz, float4* ab,
                                  hipStream_t stream);
bool atrous_can_stage(uint32_t s);
hipError_t launch_atrous(const float4* cv, const float4* nz, const float4* ab, uint32_t w, uint32_t h, uint32_t s, float isn,
                         float isa, float isz, float sigma_l, bool staged, float4* cv_out, float* out, float* var_out,
                         uint32_t row_pitch, hipStream_t stream);
// ray queries (pt_query.hip; pt_hip.h pt_query_hits_async, pt_query_occluded_async): n <= 2^30 rays of 32 B
// (pt_ray) traced to hits (n pt_hit records) or, hits == nullptr, to occluded (n bytes); exactly one of the
// two is given.  ctl: the scene's ten query control words (a wave that gave up sets ctl[0] and launches
// skip while it is set); watchdog: iterations before a wave gives up (0: kTraceWatchdog); refill: idle
// lanes take the window's next rays (0: only when the whole wave is idle); blocks: the grid (0: by occupancy)
// The batch goes out in launches of at most kQueryLaunchRays rays, in order on the stream.
constexpr int kQueryCtlWords = 10;
hipError_t launch_query(const SceneView& sc, const void* rays, uint32_t n, void* hits, uint8_t* occluded, bool count,
                        Counters* cnt, uint32_t* ctl, uint32_t watchdog, int refill, int blocks, hipStream_t stream);
// the window's camera rays of salt t, row-major, as pt_ray records (tmax = +inf, reserved = 0)
hipError_t launch_camera_rays(const FrameParams& fp, uint32_t t, void* rays, hipStream_t stream);
// n floats from device memory to pinned host memory (h_dst_dev: its device address; pt_image.hip)
hipError_t launch_readback(const float* d_src, float* h_dst_dev, size_t n, hipStream_t stream);
// dst[i] += src[i] for i < n (f32; both on the stream's device; pt_image.hip)
hipError_t launch_accum_add(float* dst, const float* src, size_t n, hipStream_t stream);

// k_wf_leafpass (pt_leafpass.hip): every big leaf of sc.pre resolved for the entries of queue in_q
// whose rays enter its path's boxes, into wb.pres; blocks: the persistent grid (0: occupancy)
hipError_t launch_leafpass(const SceneView& sc, const WfBuffers& wb, int in_q, bool fast_rcp, int blocks, int pairs,
                           hipStream_t stream);

hipError_t launch_selftest_rcp(int steps, uint32_t lo, uint32_t hi, unsigned long long* bad, hipStream_t stream);
hipError_t launch_selftest_math(int fn, const float* a, const float* b, float* o, int n, hipStream_t stream);
hipError_t launch_selftest_valu(int iters, int blocks, int packed, float* out, hipStream_t stream);
// the leaf pass's resolve_leaf / resolve_leaf_pairs against the sequential loop (pt_leafpass.hip)
hipError_t launch_selftest_leafpass(const SceneView& sc, int b, int mode, uint32_t seed, uint32_t nrays, int32_t* out,
                                    hipStream_t stream);
hipError_t launch_selftest_leaf(const SceneView& sc, int rec0, int n, int mode, uint32_t seed, uint32_t nrays, int32_t* out,
                                hipStream_t stream);
// sample_area_lights for n caller-supplied (seed, point): out n x 4 (direction, bits of the slot k)
hipError_t launch_selftest_lights(const SceneView& sc, const uint32_t* seeds, const float* points, uint32_t n, float* out,
                                  hipStream_t stream);

}  // namespace pt
