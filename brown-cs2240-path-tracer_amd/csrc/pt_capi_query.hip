// pt_capi_query.hip — C ABI (include/pt_hip.h): ray queries for caller-supplied rays and the camera's
// (pt_query.hip).  Host code only.
#include "pt_capi_internal.h"

using namespace pt;

static_assert(sizeof(pt_ray) == 32 && sizeof(pt_hit) == 32 && offsetof(pt_ray, d) == 16 && offsetof(pt_hit, n) == 16,
              "pt_ray and pt_hit are two 16-byte halves");

// the checks that need no device, in the header's order: true when the call ends here with rc (an
// error, or PT_OK for an empty batch), false to go on
// align_rays, align_out: the _async forms' device pointers (the blocking forms copy host buffers of any
// alignment the types allow into the scene's aligned scratch)
static bool query_args(const void* s, const void* rays, size_t n, const void* out, bool align_rays, bool align_out, int& rc) {
    if (n > kQueryMaxRays) { rc = fail(PT_ERR_INVALID, "query: n exceeds 2^30 rays"); return true; }
    if (n > 0 && (!rays || !out)) { rc = fail(PT_ERR_INVALID, "query: null ray or result pointer"); return true; }
    if (n > 0 && ((align_rays && ((uintptr_t)rays & 15u)) || (align_out && ((uintptr_t)out & 15u)))) {
        rc = fail(PT_ERR_INVALID, "query: rays and hits must be 16-byte aligned");
        return true;
    }
    if (!s) { rc = fail(PT_ERR_INVALID, "null scene"); return true; }
    if (n == 0) { rc = PT_OK; return true; }
    return false;
}

// the kernels' control words, zeroed when made, and their pinned mirror
static int ensure_query_ctl(pt_scene* s) {
    if (!s->d_qctl.p) {
        PT_TRY(s->d_qctl.ensure_idle(kQueryCtlWords, "query control words"));
        HIP_TRY(hipMemset(s->d_qctl.p, 0, kQueryCtlWords * sizeof(uint32_t)));
    }
    return s->h_qctl.ensure(kQueryCtlWords, "query control mirror");
}

// the blocking calls' scratch, counted in device_bytes while held (as the denoiser's planes)
static int ensure_query_scratch(pt_scene* s, size_t bytes) { return s->d_query.ensure(bytes, "query rays and results"); }

// d_hits or d_occ, the other NULL; the arguments are checked (query_args)
static int query_impl(pt_scene* s, const pt_ray* d_rays, size_t n, pt_hit* d_hits, uint8_t* d_occ, Counters* d_cnt,
                      hipStream_t stream) {
    HIP_TRY(hipSetDevice(s->device));
    int rc = ensure_query_ctl(s);
    if (rc != PT_OK) return rc;
    ProfScope prof_scope(s);
    const Opts o = opts_snapshot();
    // the scene as the default megakernel instance sees it (the big-leaf threshold, the leaf
    // remainders), as the guide buffers; of the options only the query's own and trace_watchdog apply
    SceneView view;
    if ((rc = shape_view(s, Opts{}, FrameParams{}, PT_MODE_MEGAKERNEL, n, view)) != PT_OK) return rc;
    if ((rc = take_watchdog(s)) != PT_OK) return rc;  // an earlier asynchronous call failed
    HIP_TRY(launch_query(view, d_rays, (uint32_t)n, d_hits, d_occ, d_cnt != nullptr, d_cnt, s->d_qctl.p,
                         (uint32_t)o.num("trace_watchdog", 0), o.flag("query_refill", 1), (int)o.num("query_blocks", 0), stream));
    HIP_TRY(hipMemcpyAsync(s->h_qctl.p, s->d_qctl.p, kQueryCtlWords * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    return PT_OK;
}

static int query_blocking(pt_scene* s, const pt_ray* rays, size_t n, pt_hit* hits, uint8_t* occ, pt_counters* counters) {
    const size_t ray_bytes = n * sizeof(pt_ray), out_bytes = hits ? n * sizeof(pt_hit) : n;
    Blocking b(s, counters);
    PT_TRY(b.device());
    PT_TRY(ensure_query_scratch(s, ray_bytes + align_up(out_bytes, 16)));
    PT_TRY(b.open());
    pt_ray* const d_rays = reinterpret_cast<pt_ray*>(s->d_query.p);
    char* const d_out = s->d_query.p + ray_bytes;
    PT_TRY(b.in(d_rays, rays, ray_bytes));
    PT_TRY(query_impl(s, d_rays, n, hits ? reinterpret_cast<pt_hit*>(d_out) : nullptr,
                      hits ? nullptr : reinterpret_cast<uint8_t*>(d_out), b.d_cnt(), s->stream));
    PT_TRY(b.out(hits ? static_cast<void*>(hits) : static_cast<void*>(occ), d_out, out_bytes));
    return b.finish(Blocking::kWatchdog, /*add=*/true);  // the batch's counters are added to the caller's
}

extern "C" {

int pt_query_hits_async(pt_scene* s, const pt_ray* d_rays, size_t n, pt_hit* d_hits, pt_counters* d_counters, void* stream) {
    int rc;
    if (query_args(s, d_rays, n, d_hits, true, true, rc)) return rc;
    return query_impl(s, d_rays, n, d_hits, nullptr, reinterpret_cast<Counters*>(d_counters), static_cast<hipStream_t>(stream));
}

int pt_query_occluded_async(pt_scene* s, const pt_ray* d_rays, size_t n, uint8_t* d_occluded, pt_counters* d_counters,
                            void* stream) {
    int rc;
    if (query_args(s, d_rays, n, d_occluded, true, false, rc)) return rc;
    return query_impl(s, d_rays, n, nullptr, d_occluded, reinterpret_cast<Counters*>(d_counters),
                      static_cast<hipStream_t>(stream));
}

int pt_query_hits(pt_scene* s, const pt_ray* rays, size_t n, pt_hit* hits, pt_counters* counters) {
    int rc;
    if (query_args(s, rays, n, hits, false, false, rc)) return rc;
    return query_blocking(s, rays, n, hits, nullptr, counters);
}

int pt_query_occluded(pt_scene* s, const pt_ray* rays, size_t n, uint8_t* occluded, pt_counters* counters) {
    int rc;
    if (query_args(s, rays, n, occluded, false, false, rc)) return rc;
    return query_blocking(s, rays, n, nullptr, occluded, counters);
}

static int camera_rays_args(const pt_scene* s, const float* meta, const pt_window* win, uint32_t frame, const void* rays,
                            bool aligned, FrameParams& fp) {
    PT_TRY(check_frames(frame, 1, 1));
    if (!meta || !rays) return fail(PT_ERR_INVALID, "null argument");
    if (aligned && ((uintptr_t)rays & 15u)) return fail(PT_ERR_INVALID, "rays must be 16-byte aligned");
    if (!s) return fail(PT_ERR_INVALID, "null scene");
    return make_params(meta, 0, fp, win);
}

int pt_camera_rays_async(pt_scene* s, const float meta[48], const pt_window* win, uint32_t frame, pt_ray* d_rays,
                         void* stream) {
    FrameParams fp{};
    const int rc = camera_rays_args(s, meta, win, frame, d_rays, true, fp);
    if (rc != PT_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    ProfScope prof_scope(s);
    LensCam lens;  // pt_scene_set_camera: the model's rays
    HIP_TRY(launch_camera_rays(fp, (uint32_t)(float)frame, d_rays, static_cast<hipStream_t>(stream), scene_camera(s, lens)));
    return PT_OK;
}

int pt_camera_rays(pt_scene* s, const float meta[48], const pt_window* win, uint32_t frame, pt_ray* rays) {
    FrameParams fp{};
    PT_TRY(camera_rays_args(s, meta, win, frame, rays, false, fp));
    const size_t bytes = (size_t)fp.win_w * fp.win_h * sizeof(pt_ray);
    Blocking b(s);
    PT_TRY(b.device());
    PT_TRY(ensure_query_scratch(s, bytes));
    PT_TRY(b.open());
    PT_TRY(pt_camera_rays_async(s, meta, win, frame, reinterpret_cast<pt_ray*>(s->d_query.p), s->stream));
    PT_TRY(b.out(rays, s->d_query.p, bytes));
    return b.finish(Blocking::kNoWatchdog);  // traces nothing: the next call of the scene takes the watchdog
}

}  // extern "C"
