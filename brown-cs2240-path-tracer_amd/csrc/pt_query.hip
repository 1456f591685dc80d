// pt_query.hip — ray queries for caller-supplied rays (pt_hip.h pt_query_hits, pt_query_occluded,
// pt_camera_rays).
//
//   k_query<TRAV, OCCL, COUNT>   256 threads, one ray per lane, the scene in global memory, the lanes'
//       stacks in LDS.  Every ray is traced as the reference's intersect() traces it (the traversal of
//       k_features and k_regen: trav_advance with CHUNKS = false, no pre-resolved leaves), with 1/det by
//       IEEE division: the rays are the caller's, not unit vectors, and rcp_rn is proved exact for unit
//       directions only.  OCCL = false writes the closest hit's record (two 16-byte stores),
//       OCCL = true one byte: whether the closest hit lies below the ray's tmax — and stops the ray at
//       the first triangle test that succeeds below tmax, which decides that byte (pt_hip.h).
//       The batch is handed to the waves in windows of 64 rays (pt_query_plan.h): a lane that finishes
//       its ray takes the window's next one at the top of the loop, so lanes do not idle while the
//       wave's slowest ray is traced (refill = 0 keeps them idle until all 64 are done: the A/B).
//   k_camera_rays   one lane per pixel of the window: the ray camera_ray gives that pixel and salt.
//   k_camera_seeds  one lane per pixel of the window: the seed camera_ray hands to radiance() there.
#include "pt_kernels.h"
#include "pt_occupancy.h"
#include "pt_path.h"
#include "pt_query_plan.h"

namespace pt {

namespace {

// Per wave in LDS: the current window's rays, kQueryWin x 32 B.  The results are NOT staged: a lane
// stores its own result when its ray ends, from inside the loop (on gfx9 a store shares the wave's
// in-order vmcnt with the loads, so the next use of a loaded register also waits for it; k_wf_trace
// stages its hit records in an LDS ring for that reason, see the comment above kWinRays in
// pt_wf_trace.hip).  Here a store happens once per ray, not per step, and the ring would cost the
// occupancy the stacks leave; DESIGN.md §5.10 keeps staging as a lead.
constexpr uint32_t kQueryStageBytes = kQueryWin * 32;

}  // namespace

// ctl[0]: a wave of an earlier query launch of the scene gave up (the guard below); launches skip
// while it is set.  ctl[1]: claimed by the first such wave, which leaves its state in ctl[2..9].
template <int TRAV, bool OCCL, bool COUNT>
__global__ __launch_bounds__(kMegaBlock) void k_query(SceneView sc, const float4* __restrict__ rays, uint32_t n,
                                                     float4* __restrict__ hits, uint8_t* __restrict__ occluded,
                                                     Counters* cnt_out, uint32_t* ctl, uint32_t watchdog, int refill) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LStack32 stack = LStack32::make(smem, kMegaBlock);  // [max_stack][256] int32, lane-minor
    const uint32_t lane = threadIdx.x & 63u;
    float4* const wray = reinterpret_cast<float4*>(smem + (uint32_t)sc.max_stack * 4u * kMegaBlock +
                                                   (threadIdx.x / 64u) * kQueryStageBytes);  // [kQueryWin][2]
    // division instances only; no chunk walks, no pooled turns, no pre-resolved leaves (their bounds
    // are derived for unit directions)
    sc.fast_rcp = 0;
    sc.lkeys = nullptr;
    sc.pres = nullptr;
    sc.npre = 0;
    const uint32_t nwaves = gridDim.x * (kMegaBlock / 64);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kMegaBlock / 64) + threadIdx.x / 64);
    if (__builtin_amdgcn_readfirstlane(ctl[0]) != 0u) return;  // an earlier launch gave up: skip
    QueryWave q;
    if (!query_begin(q, w, nwaves, n)) return;  // wave-uniform: nothing for this wave
    // window rays: lane l loads the float4s l and l + 64 of the window's 2 * len (coalesced)
    auto load = [&](uint32_t wid, uint32_t len, float4& a, float4& b) {
        const float4* p = rays + 2 * (size_t)wid * kQueryWin;
        if (lane < 2 * len) a = p[lane];
        if (lane + 64 < 2 * len) b = p[lane + 64];
    };
    auto stage = [&](uint32_t len, const float4& a, const float4& b) {
        if (lane < 2 * len) wray[lane] = a;
        if (lane + 64 < 2 * len) wray[lane + 64] = b;
    };
    float4 na = make_float4(0, 0, 0, 0), nb = na;
    load(q.base / kQueryWin, q.wv, na, nb);
    stage(q.wv, na, nb);
    if (q.wnx != kQueryNone) load(q.wnx, q.nv, na, nb);
    Counters c = {};
    bool has = false;
    uint32_t idx = 0;  // the lane's ray, and its result's slot
    float tmax = 0.0f;
    Ray r;
    r.o = r.d = r.inv = mk(0.0f, 0.0f, 0.0f);
    typename TravSel<TRAV>::type s;
    trav_init(s, false);
    const uint64_t t_start = wall_clock64();
    for (uint32_t guard = 0;; ++guard) {
        // every wave reaches an exit: after `watchdog` iterations or kTraceWatchdogTicks of wall
        // clock it reports instead of hanging, and later launches of the scene skip
        if (guard == watchdog || ((guard & 1023u) == 1023u && wall_clock64() - t_start > kTraceWatchdogTicks)) {
            const uint64_t hm = __ballot(has);
            if (lane == 0) {
                atomicOr(&ctl[0], 1u);
                if (atomicCAS(&ctl[1], 0u, 1u) == 0u) {
                    const uint32_t v[8] = {n, nwaves, w, q.nfetch, q.base, q.wv, q.cur, (uint32_t)__popcll(hm)};
                    for (int i = 0; i < 8; ++i) ctl[2 + i] = v[i];
                }
            }
            break;
        }
        // hand the window's next rays to the idle lanes (wave-uniform control)
        const uint64_t need = __ballot(!has);
        if (query_hands_out(need, refill != 0)) {
            if (query_wants_next(q)) {
                wave_lds_sync();  // the lanes' reads of the old window come first
                stage(q.nv, na, nb);
                query_advance(q, w, nwaves, n);
                if (q.wnx != kQueryNone) load(q.wnx, q.nv, na, nb);
            }
            wave_lds_sync();  // the window's rays were written by other lanes
            const uint32_t k = has ? kQueryNone : query_position(q, rank_below(need));
            if (k != kQueryNone) {
                const float4 a = wray[2 * k], b = wray[2 * k + 1];
                r.o = mk(a.x, a.y, a.z);
                r.d = mk(b.x, b.y, b.z);
                r.inv = rcp3(r.d);
                tmax = a.w;
                idx = q.base + k;
                trav_init(s, true);
                has = true;
                if (COUNT) { if (OCCL) c.shadow_queries++; else c.ext_queries++; }
            }
            query_took(q, (uint32_t)__popcll(need));
        }
        const uint64_t busy = __ballot(has);
        if (busy == 0) {
            if (query_done(q, busy)) break;
            continue;  // (not reached: an idle wave always hands out; the guard bounds it anyway)
        }
        trav_advance<TRAV, COUNT>(sc, r, s, stack, c);  // all 64 lanes: the cooperative turns deal over them
        if (has) {
            bool fin = trav_finished(s);
            if (OCCL && !fin && s.best_t > 0.0f && s.best_t < tmax) {
                trav_stop(s);  // the closest t only decreases: the result is decided (pt_hip.h)
                fin = true;
            }
            if (fin) {
                const bool hit = s.best >= 0 && s.best_t < tmax;  // NaN tmax: a miss
                if (OCCL) {
                    occluded[idx] = hit ? 1 : 0;
                } else {
                    float4 o0 = make_float4(0.0f, 0.0f, 0.0f, -1.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
                    if (hit) {
                        const Hit h = hit_data(sc, r, s.best, s.best_t);
                        o0 = make_float4(h.p.x, h.p.y, h.p.z, s.best_t);
                        o1 = make_float4(h.n.x, h.n.y, h.n.z, __int_as_float(h.mat));
                    }
                    hits[2 * (size_t)idx] = o0;
                    hits[2 * (size_t)idx + 1] = o1;
                }
                has = false;
            }
        }
    }
    if (COUNT) flush_counters(c, cnt_out);
}

// The batch goes out in launches of at most kQueryLaunchRays rays, in order on the stream: a wave lives
// as long as its launch and its wall-clock guard counts from its start, so the guard must bound a
// launch's work, not the caller's batch (as wf_paths bounds a k_wf_trace launch).  Every ray's result
// is its own, so the cut changes no value; a cut is a multiple of the window, so rays and hits stay
// 16-byte aligned.
template <int TRAV, bool OCCL>
static hipError_t launch_query_t(const SceneView& sc, const float4* rays, uint32_t n, float4* hits, uint8_t* occ, bool count,
                                 Counters* cnt, uint32_t* ctl, uint32_t watchdog, int refill, int blocks, hipStream_t stream) {
    const size_t lds = (size_t)sc.max_stack * kMegaBlock * 4 + (kMegaBlock / 64) * kQueryStageBytes;
    const void* const kernel = count ? reinterpret_cast<const void*>(&k_query<TRAV, OCCL, true>)
                                     : reinterpret_cast<const void*>(&k_query<TRAV, OCCL, false>);
    int full = blocks;
    if (full <= 0) {  // auto: what the device holds at once
        const hipError_t e = occupancy_blocks(kernel, kMegaBlock, lds, full);  // a pick of one ray pays no runtime call: cached
        if (e != hipSuccess) return e;
    }
    const int kid = OCCL ? KID_QUERY_OCCLUDED : KID_QUERY_HITS;
    for (uint32_t first = 0; first < n; first += kQueryLaunchRays) {
        const uint32_t m = std::min(n - first, kQueryLaunchRays);
        const uint32_t nwin = query_windows(m), waves_per_block = kMegaBlock / 64;
        // ... and no more blocks than there are windows
        const int grid = (int)std::min<uint32_t>((uint32_t)full, (nwin + waves_per_block - 1) / waves_per_block);
        const float4* const r = rays + 2 * (size_t)first;
        float4* const h = hits ? hits + 2 * (size_t)first : nullptr;
        uint8_t* const o = occ ? occ + first : nullptr;
        if (count)
            PT_LAUNCH(kid, stream, (k_query<TRAV, OCCL, true>), dim3(grid), dim3(kMegaBlock), lds, stream, sc, r, m, h, o, cnt, ctl,
                      watchdog, refill);
        else
            PT_LAUNCH(kid, stream, (k_query<TRAV, OCCL, false>), dim3(grid), dim3(kMegaBlock), lds, stream, sc, r, m, h, o, cnt, ctl,
                      watchdog, refill);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_query(const SceneView& scene, const void* rays, uint32_t n, void* hits, uint8_t* occluded, bool count,
                        Counters* cnt, uint32_t* ctl, uint32_t watchdog, int refill, int blocks, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > kQueryMaxRays || (hits != nullptr) == (occluded != nullptr)) return hipErrorInvalidValue;
    SceneView sc = scene;
    // the megakernel's turn policy (launch_megakernel), as k_features
    if (sc.node_bias <= 0) sc.node_bias = 8;
    if (sc.node_steps <= 0) sc.node_steps = 1;
    const float4* r4 = static_cast<const float4*>(rays);
    float4* h4 = static_cast<float4*>(hits);
    if (watchdog == 0) watchdog = kTraceWatchdog;
    // the flavour is the query's own: select_megakernel pairs the cooperative turns with the fast
    // reciprocal, and the query has division instances only
    constexpr int kPlain = flavour(FLV_PLAIN, TRAV_LEAN4, false), kBig = flavour(FLV_BIG, TRAV_LEAN4, false);
    if (sc.big_leaf > 0)
        return occluded ? launch_query_t<kBig, true>(sc, r4, n, h4, occluded, count, cnt, ctl, watchdog, refill, blocks, stream)
                        : launch_query_t<kBig, false>(sc, r4, n, h4, occluded, count, cnt, ctl, watchdog, refill, blocks, stream);
    return occluded ? launch_query_t<kPlain, true>(sc, r4, n, h4, occluded, count, cnt, ctl, watchdog, refill, blocks, stream)
                    : launch_query_t<kPlain, false>(sc, r4, n, h4, occluded, count, cnt, ctl, watchdog, refill, blocks, stream);
}

// One lane per pixel of the window in the megakernels' 16 x 16 layout: ray (y - win_y0) * win_w +
// (x - win_x0) = camera_ray(fp, x, y, t), tmax = +inf, reserved = 0.
__global__ __launch_bounds__(kMegaBlock) void k_camera_rays(FrameParams fp, uint32_t t, float4* __restrict__ rays) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t i = blockIdx.x * 16 + (wv & 1) * 8 + (lane & 7);
    const uint32_t j = blockIdx.y * 16 + (wv >> 1) * 8 + (lane >> 3);
    if (i >= fp.win_w || j >= fp.win_h) return;
    uint32_t seed;
    const Ray r = camera_ray(fp, fp.win_x0 + i, fp.win_y0 + j, t, seed);
    const size_t o = 2 * ((size_t)j * fp.win_w + i);
    rays[o] = make_float4(r.o.x, r.o.y, r.o.z, __builtin_inff());
    rays[o + 1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
}

// k_camera_rays under a lens camera: camera_ray_model<MODEL>'s ray as computed, whether the render
// would admit its direction or not (no compaction: ray q of the window is record q)
template <uint32_t MODEL>
__global__ __launch_bounds__(kMegaBlock) void k_camera_rays_cam(FrameParams fp, LensCam lc, uint32_t t, float4* __restrict__ rays) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t i = blockIdx.x * 16 + (wv & 1) * 8 + (lane & 7);
    const uint32_t j = blockIdx.y * 16 + (wv >> 1) * 8 + (lane >> 3);
    if (i >= fp.win_w || j >= fp.win_h) return;
    uint32_t seed;
    const Ray r = camera_ray_model<MODEL>(fp, lc, fp.win_x0 + i, fp.win_y0 + j, t, seed);
    const size_t o = 2 * ((size_t)j * fp.win_w + i);
    rays[o] = make_float4(r.o.x, r.o.y, r.o.z, __builtin_inff());
    rays[o + 1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
}

hipError_t launch_camera_rays(const FrameParams& fp, uint32_t t, void* rays, hipStream_t stream, const LensCam* cam) {
    const dim3 grid((fp.win_w + 15) / 16, (fp.win_h + 15) / 16), block(kMegaBlock);
    float4* const r4 = static_cast<float4*>(rays);
    if (!cam) PT_LAUNCH(KID_CAMERA_RAYS, stream, k_camera_rays, grid, block, 0, stream, fp, t, r4);
    else if (cam->model == CAM_THIN_LENS) PT_LAUNCH(KID_CAMERA_RAYS, stream, k_camera_rays_cam<CAM_THIN_LENS>, grid, block, 0, stream, fp, *cam, t, r4);
    else if (cam->model == CAM_ORTHO) PT_LAUNCH(KID_CAMERA_RAYS, stream, k_camera_rays_cam<CAM_ORTHO>, grid, block, 0, stream, fp, *cam, t, r4);
    else if (cam->model == CAM_EQUIRECT) PT_LAUNCH(KID_CAMERA_RAYS, stream, k_camera_rays_cam<CAM_EQUIRECT>, grid, block, 0, stream, fp, *cam, t, r4);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// camera_ray's seed_out, the value pixel_sample hands to radiance(), for the same pixels in the same
// order as k_camera_rays (the ray itself is dead code here)
__global__ __launch_bounds__(kMegaBlock) void k_camera_seeds(FrameParams fp, uint32_t t, uint32_t* __restrict__ seeds) {
    const uint32_t q = blockIdx.x * kMegaBlock + threadIdx.x;
    if (q >= fp.win_w * fp.win_h) return;
    const uint32_t j = q / fp.win_w, i = q - j * fp.win_w;
    uint32_t seed;
    (void)camera_ray(fp, fp.win_x0 + i, fp.win_y0 + j, t, seed);
    seeds[q] = seed;
}

hipError_t launch_camera_seeds(const FrameParams& fp, uint32_t t, uint32_t* seeds, hipStream_t stream) {
    const dim3 grid((fp.win_w * fp.win_h + kMegaBlock - 1) / kMegaBlock), block(kMegaBlock);
    PT_LAUNCH(KID_CAMERA_SEEDS, stream, k_camera_seeds, grid, block, 0, stream, fp, t, seeds);
    return hipGetLastError();
}

}  // namespace pt
