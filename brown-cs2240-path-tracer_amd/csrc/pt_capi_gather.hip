// pt_capi_gather.hip — C ABI (include/pt_hip.h): irradiance gathers — lightmap texels and SH probes
// sampled on the device (pt_wf_source.hip k_wf_generate_gather / k_wf_accum_gather / k_gather_rays;
// DESIGN.md §5.13).  Host code only.
#include "pt_capi_internal.h"

using namespace pt;

static_assert(sizeof(pt_gather_point) == 32, "pt_gather_point is two float4");
static_assert(sizeof(pt_gather_params) == 24, "pt_gather_params is six 32-bit words");
static_assert(PT_GATHER_COSINE == 0 && PT_GATHER_SH9 == 1, "the kernels' mode numbers (pt_path.h)");

constexpr uint64_t kGatherMaxPoints = 1ull << 26;  // one sample of every point fits a wavefront batch

static size_t gather_words(uint32_t mode) { return mode == PT_GATHER_SH9 ? 27 : 3; }

// the checks that need no device, in the header's order: true when the call ends here with rc (an
// error, or PT_OK for an empty call), false to go on.  aligned: the _async form's device pointers
static bool gather_args(const void* s, const void* pts, size_t n, const pt_gather_params* prm, const void* accum, bool aligned,
                        int& rc) {
    if (!prm) { rc = fail(PT_ERR_INVALID, "gather: params is NULL"); return true; }
    if (prm->mode > PT_GATHER_SH9) { rc = fail(PT_ERR_INVALID, "gather: unknown mode"); return true; }
    if (n > kGatherMaxPoints) { rc = fail(PT_ERR_INVALID, "gather: n exceeds 2^26 points"); return true; }
    if ((uint64_t)prm->sample0 + prm->nsamples > (1ull << 31)) { rc = fail(PT_ERR_INVALID, "gather: sample0 + nsamples exceeds 2^31"); return true; }
    if (prm->max_depth < 0 || prm->max_depth > 1024) { rc = fail(PT_ERR_INVALID, "gather: max_depth out of range"); return true; }
    if (n > 0 && (!pts || !accum)) { rc = fail(PT_ERR_INVALID, "gather: null point or accumulator pointer"); return true; }
    if (n > 0 && aligned && (((uintptr_t)pts & 15u) || ((uintptr_t)accum & 3u))) {
        rc = fail(PT_ERR_INVALID, "gather: points must be 16-byte aligned, accum 4-byte aligned");
        return true;
    }
    if (!s) { rc = fail(PT_ERR_INVALID, "null scene"); return true; }
    if (n == 0 || prm->nsamples == 0) { rc = PT_OK; return true; }
    return false;
}

// the arguments are checked (gather_args); the options, batching and watchdog of pt_query_radiance
static int gather_impl(pt_scene* s, const pt_gather_point* d_pts, size_t n, const pt_gather_params& prm, float* d_accum,
                       Counters* d_cnt, hipStream_t stream) {
    const GatherList gl{reinterpret_cast<const float4*>(d_pts), (uint32_t)n, prm.mode};
    return query_call(s, PathSource(gl), n, prm.sample0, prm.nsamples, prm.rr_prob, prm.direct_only, prm.max_depth,
                      d_accum, d_cnt, stream);
}

static int gather_rays_args(const void* s, const void* pts, size_t n, uint32_t mode, uint32_t sample, const void* rays,
                            const void* seeds, bool aligned) {
    if (mode > PT_GATHER_SH9) return fail(PT_ERR_INVALID, "gather rays: unknown mode");
    if (n > kGatherMaxPoints) return fail(PT_ERR_INVALID, "gather rays: n exceeds 2^26 points");
    if (sample >= (1u << 31)) return fail(PT_ERR_INVALID, "gather rays: sample exceeds 2^31 - 1");
    if (n > 0 && (!pts || !rays || !seeds)) return fail(PT_ERR_INVALID, "gather rays: null point, ray or seed pointer");
    if (n > 0 && aligned && (((uintptr_t)pts & 15u) || ((uintptr_t)rays & 15u) || ((uintptr_t)seeds & 3u)))
        return fail(PT_ERR_INVALID, "gather rays: points and rays must be 16-byte aligned, seeds 4-byte aligned");
    if (!s) return fail(PT_ERR_INVALID, "null scene");
    return PT_OK;
}

extern "C" {

int pt_gather_async(pt_scene* s, const pt_gather_point* d_pts, size_t n, const pt_gather_params* params, float* d_accum,
                    pt_counters* d_counters, void* stream) {
    int rc;
    if (gather_args(s, d_pts, n, params, d_accum, true, rc)) return rc;
    return gather_impl(s, d_pts, n, *params, d_accum, reinterpret_cast<Counters*>(d_counters), static_cast<hipStream_t>(stream));
}

int pt_gather(pt_scene* s, const pt_gather_point* pts, size_t n, const pt_gather_params* params, float* accum,
              pt_counters* counters) {
    int rc;
    if (gather_args(s, pts, n, params, accum, false, rc)) return rc;
    const size_t pt_bytes = n * sizeof(pt_gather_point), acc_bytes = gather_words(params->mode) * n * sizeof(float);
    Blocking b(s, counters);
    PT_TRY(b.device());
    PT_TRY(s->d_radq.ensure(pt_bytes + acc_bytes, "gather points and accumulator"));
    PT_TRY(b.open());
    pt_gather_point* const d_pts = reinterpret_cast<pt_gather_point*>(s->d_radq.p);
    float* const d_acc = reinterpret_cast<float*>(s->d_radq.p + pt_bytes);
    PT_TRY(b.in(d_pts, pts, pt_bytes));
    PT_TRY(b.in(d_acc, accum, acc_bytes));
    PT_TRY(gather_impl(s, d_pts, n, *params, d_acc, b.d_cnt(), s->stream));
    PT_TRY(b.out(accum, d_acc, acc_bytes));
    return b.finish(Blocking::kWatchdog, /*add=*/true);  // the call's counters are added to the caller's
}

int pt_gather_rays_async(pt_scene* s, const pt_gather_point* d_pts, size_t n, uint32_t mode, uint32_t sample, pt_ray* d_rays,
                         uint32_t* d_seeds, void* stream) {
    PT_TRY(gather_rays_args(s, d_pts, n, mode, sample, d_rays, d_seeds, true));
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(s->device));
    ProfScope prof_scope(s);
    const GatherList gl{reinterpret_cast<const float4*>(d_pts), (uint32_t)n, mode};
    HIP_TRY(launch_gather_rays(gl, sample, d_rays, d_seeds, static_cast<hipStream_t>(stream)));
    return PT_OK;
}

int pt_gather_rays(pt_scene* s, const pt_gather_point* pts, size_t n, uint32_t mode, uint32_t sample, pt_ray* rays,
                   uint32_t* seeds) {
    PT_TRY(gather_rays_args(s, pts, n, mode, sample, rays, seeds, false));
    if (n == 0) return PT_OK;
    const size_t pt_bytes = n * sizeof(pt_gather_point), ray_bytes = n * sizeof(pt_ray), seed_bytes = n * sizeof(uint32_t);
    Blocking b(s);
    PT_TRY(b.device());
    PT_TRY(s->d_radq.ensure(pt_bytes + ray_bytes + seed_bytes, "gather points, rays and seeds"));
    PT_TRY(b.open());
    pt_gather_point* const d_pts = reinterpret_cast<pt_gather_point*>(s->d_radq.p);
    pt_ray* const d_rays = reinterpret_cast<pt_ray*>(s->d_radq.p + pt_bytes);
    uint32_t* const d_seeds = reinterpret_cast<uint32_t*>(s->d_radq.p + pt_bytes + ray_bytes);
    PT_TRY(b.in(d_pts, pts, pt_bytes));
    PT_TRY(pt_gather_rays_async(s, d_pts, n, mode, sample, d_rays, d_seeds, s->stream));
    PT_TRY(b.out(rays, d_rays, ray_bytes));
    PT_TRY(b.out(seeds, d_seeds, seed_bytes));
    return b.finish(Blocking::kNoWatchdog);  // traces nothing: the next call of the scene takes the watchdog
}

}  // extern "C"
