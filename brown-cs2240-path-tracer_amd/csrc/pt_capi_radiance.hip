// pt_capi_radiance.hip — C ABI (include/pt_hip.h): radiance queries for caller-supplied rays and the
// camera's seeds (pt_wf_source.hip k_wf_generate_rays / k_wf_accum_rays, pt_query.hip k_camera_seeds;
// DESIGN.md §5.11).  Host code only.
#include <cmath>

#include "pt_capi_internal.h"

using namespace pt;

static_assert(sizeof(pt_radiance_params) == 16, "pt_radiance_params is four 32-bit words");

constexpr uint64_t kRadianceMaxRays = 1ull << 26;  // one sample of every ray fits a wavefront batch

// the checks that need no device, in the header's order: true when the call ends here with rc (an
// error, or PT_OK for an empty call), false to go on.  aligned: the _async form's device pointers
static bool radiance_args(const void* s, const void* rays, const void* seeds, size_t n, const pt_radiance_params* prm,
                          const void* accum, bool aligned, int& rc) {
    if (!prm) { rc = fail(PT_ERR_INVALID, "radiance query: params is NULL"); return true; }
    if (n > kRadianceMaxRays) { rc = fail(PT_ERR_INVALID, "radiance query: n exceeds 2^26 rays"); return true; }
    if (prm->max_depth < 0 || prm->max_depth > 1024) { rc = fail(PT_ERR_INVALID, "radiance query: max_depth out of range"); return true; }
    if (n > 0 && (!rays || !seeds || !accum)) { rc = fail(PT_ERR_INVALID, "radiance query: null ray, seed or accumulator pointer"); return true; }
    if (n > 0 && aligned && (((uintptr_t)rays & 15u) || ((uintptr_t)seeds & 3u) || ((uintptr_t)accum & 3u))) {
        rc = fail(PT_ERR_INVALID, "radiance query: rays must be 16-byte aligned, seeds and accum 4-byte aligned");
        return true;
    }
    if (!s) { rc = fail(PT_ERR_INVALID, "null scene"); return true; }
    if (n == 0 || prm->nsamples == 0) { rc = PT_OK; return true; }
    return false;
}

// the arguments are checked (radiance_args)
static int radiance_impl(pt_scene* s, const pt_ray* d_rays, const uint32_t* d_seeds, size_t n, const pt_radiance_params& prm,
                         float* d_accum, Counters* d_cnt, hipStream_t stream) {
    const RayList ql{reinterpret_cast<const float4*>(d_rays), d_seeds, (uint32_t)n};
    return query_call(s, PathSource(ql), n, 0, prm.nsamples, prm.rr_prob, prm.direct_only, prm.max_depth, d_accum, d_cnt,
                      stream);
}

extern "C" {

int pt_query_radiance_async(pt_scene* s, const pt_ray* d_rays, const uint32_t* d_seeds, size_t n,
                            const pt_radiance_params* params, float* d_accum, pt_counters* d_counters, void* stream) {
    int rc;
    if (radiance_args(s, d_rays, d_seeds, n, params, d_accum, true, rc)) return rc;
    return radiance_impl(s, d_rays, d_seeds, n, *params, d_accum, reinterpret_cast<Counters*>(d_counters),
                         static_cast<hipStream_t>(stream));
}

int pt_query_radiance(pt_scene* s, const pt_ray* rays, const uint32_t* seeds, size_t n, const pt_radiance_params* params,
                      float* accum, pt_counters* counters) {
    int rc;
    if (radiance_args(s, rays, seeds, n, params, accum, false, rc)) return rc;
    const size_t ray_bytes = n * sizeof(pt_ray), seed_bytes = align_up(n * sizeof(uint32_t), 16), acc_bytes = 3 * n * sizeof(float);
    Blocking b(s, counters);
    PT_TRY(b.device());
    PT_TRY(s->d_radq.ensure(ray_bytes + seed_bytes + acc_bytes, "radiance query rays, seeds and accumulator"));
    PT_TRY(b.open());
    pt_ray* const d_rays = reinterpret_cast<pt_ray*>(s->d_radq.p);
    uint32_t* const d_seeds = reinterpret_cast<uint32_t*>(s->d_radq.p + ray_bytes);
    float* const d_acc = reinterpret_cast<float*>(s->d_radq.p + ray_bytes + seed_bytes);
    PT_TRY(b.in(d_rays, rays, ray_bytes));
    PT_TRY(b.in(d_seeds, seeds, n * sizeof(uint32_t)));
    PT_TRY(b.in(d_acc, accum, acc_bytes));
    PT_TRY(radiance_impl(s, d_rays, d_seeds, n, *params, d_acc, b.d_cnt(), s->stream));
    PT_TRY(b.out(accum, d_acc, acc_bytes));
    return b.finish(Blocking::kWatchdog, /*add=*/true);  // the call's counters are added to the caller's
}

static int camera_seeds_args(const pt_scene* s, const float* meta, const pt_window* win, uint32_t frame, const void* seeds,
                             bool aligned, FrameParams& fp) {
    PT_TRY(check_frames(frame, 1, 1));
    if (!meta || !seeds) return fail(PT_ERR_INVALID, "null argument");
    if (aligned && ((uintptr_t)seeds & 3u)) return fail(PT_ERR_INVALID, "seeds must be 4-byte aligned");
    if (!s) return fail(PT_ERR_INVALID, "null scene");
    return make_params(meta, 0, fp, win);
}

int pt_camera_seeds_async(pt_scene* s, const float meta[48], const pt_window* win, uint32_t frame, uint32_t* d_seeds,
                          void* stream) {
    FrameParams fp{};
    PT_TRY(camera_seeds_args(s, meta, win, frame, d_seeds, true, fp));
    HIP_TRY(hipSetDevice(s->device));
    ProfScope prof_scope(s);
    HIP_TRY(launch_camera_seeds(fp, (uint32_t)(float)frame, d_seeds, static_cast<hipStream_t>(stream)));
    return PT_OK;
}

int pt_camera_seeds(pt_scene* s, const float meta[48], const pt_window* win, uint32_t frame, uint32_t* seeds) {
    FrameParams fp{};
    PT_TRY(camera_seeds_args(s, meta, win, frame, seeds, false, fp));
    const size_t bytes = (size_t)fp.win_w * fp.win_h * sizeof(uint32_t);
    Blocking b(s);
    PT_TRY(b.device());
    PT_TRY(s->d_radq.ensure(bytes, "camera seeds"));
    PT_TRY(b.open());
    PT_TRY(pt_camera_seeds_async(s, meta, win, frame, reinterpret_cast<uint32_t*>(s->d_radq.p), s->stream));
    PT_TRY(b.out(seeds, s->d_radq.p, bytes));
    return b.finish(Blocking::kNoWatchdog);  // traces nothing: the next call of the scene takes the watchdog
}

}  // extern "C"
