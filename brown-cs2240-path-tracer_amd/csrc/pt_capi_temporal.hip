// pt_capi_temporal.hip — C ABI (include/pt_hip.h): temporal accumulation (pt_temporal.hip):
// the reprojection step, the denoiser on a given mean and variance, and the history object that keeps the
// state on the device between calls.  Host code only.
#include <algorithm>
#include <cmath>

#include "pt_capi_internal.h"

using namespace pt;

// Two sets of the three planes, the previous step's meta and the step's working buffers.  scene == nullptr: the
// scene was destroyed first (orphan_histories).  The buffers are counted in the scene's device_bytes, but by
// `held` and release() below, never through Scratch's own counter pointer: that pointer would address the
// pt_scene, and a history may be destroyed after its scene — ~Scratch would then write into freed memory.
struct pt_history {
    pt_scene* scene;
    uint32_t w, h;
    pt::Scratch<float4> planes;  // [2][3][h][w]: set, then hist, mom, gbuf
    pt::Scratch<float> work;     // accum, m2 (3 each), geo, alb (4 each), mean, filtered (3 each), var, fvar (1 each)
    pt::Scratch<uint8_t> rgba;
    uint64_t held = 0;  // bytes of the three buffers added to scene->info.device_bytes
    float meta_prev[48];
    bool has_prev = false;
    int cur = 0;  // the set the last step wrote
    pt_history(pt_scene* s, uint32_t w_, uint32_t h_) : scene(s), w(w_), h(h_) {}
    // the buffers freed and taken out of the scene's count; the scene, if any, is alive and its device set
    void release() {
        planes.free();
        work.free();
        rgba.free();
        if (scene) scene->info.device_bytes -= held;
        held = 0;
    }
};
constexpr size_t kHistoryWorkFloats = 3 + 3 + 4 + 4 + 3 + 3 + 1 + 1;

static int check_temporal(const pt_temporal_params& p) {
    const float v[4] = {p.alpha, p.normal_min, p.depth_tol, p.max_history};
    static const char* const names[4] = {"alpha", "normal_min", "depth_tol", "max_history"};
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(v[k])) return fail(PT_ERR_INVALID, std::string("pt_temporal_params: ") + names[k] + " must be finite");
    if (!(p.alpha > 0.0f && p.alpha <= 1.0f)) return fail(PT_ERR_INVALID, "pt_temporal_params: alpha must lie in (0, 1]");
    if (!(p.depth_tol > 0.0f)) return fail(PT_ERR_INVALID, "pt_temporal_params: depth_tol must be > 0");
    if (!(p.max_history >= 1.0f)) return fail(PT_ERR_INVALID, "pt_temporal_params: max_history must be at least 1");
    return PT_OK;
}

static int temporal_params(const pt_temporal_params* p, pt_temporal_params& out) {
    pt_temporal_defaults(&out);
    if (p) out = *p;
    return check_temporal(out);
}

// the bytes a plane of 16 * comps / 4 bytes per pixel spans, and whether two such spans overlap
static bool spans_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

// the arguments of a step, checked without a device: the kernel's parameters
static int reproject_args(const float* meta_cur, const float* meta_prev, const float* const prev[3], uint32_t n, uint32_t w,
                          uint32_t h, size_t row_pitch, const pt_temporal_params* p, float* const next[3],
                          ReprojectParams& P) {
    pt_temporal_params prm;
    PT_TRY(temporal_params(p, prm));
    if (n < 1) return fail(PT_ERR_INVALID, "n must be at least 1 (the frames of the step's render)");
    const int given = (meta_prev != nullptr) + (prev[0] != nullptr) + (prev[1] != nullptr) + (prev[2] != nullptr);
    if (given != 0 && given != 4)
        return fail(PT_ERR_INVALID, "history: meta_prev and the three previous planes must be all NULL or all given");
    FrameParams fc{}, fq{};
    PT_TRY(make_params(meta_cur, 0, fc));
    if (fc.width != w || fc.height != h) return fail(PT_ERR_INVALID, "meta_cur: W and H must be the image's w and h");
    PT_TRY(make_params(meta_cur, 0, fc, nullptr, &row_pitch));  // the pitch
    if (given) {
        PT_TRY(make_params(meta_prev, 0, fq));
        if (fq.width != w || fq.height != h) return fail(PT_ERR_INVALID, "meta_prev: W and H must be the image's w and h");
    }
    const size_t span = ((size_t)(h - 1) * row_pitch + w) * sizeof(float4);
    for (int k = 0; k < 3; ++k)
        for (int l = 0; l < 3; ++l) {
            if (given && spans_overlap(prev[k], next[l], span))
                return fail(PT_ERR_INVALID, "history: the previous and the new planes must not alias");
            if (k < l && spans_overlap(next[k], next[l], span))
                return fail(PT_ERR_INVALID, "history: the new planes must not alias each other");
        }
    P = ReprojectParams{};
    P.w = w; P.h = h; P.row_pitch = fc.row_pitch; P.n = n;
    P.W = fc.W; P.H = fc.H; P.inv_w = fc.inv_w; P.inv_h = fc.inv_h;
    P.aspect = fc.aspect; P.focal = fc.focal; P.view_half_h = fc.view_half_h;
    std::copy(fc.cam, fc.cam + 4, P.cam);
    std::copy(fc.M, fc.M + 16, P.M);
    if (given) {
        P.paspect = fq.aspect; P.pfocal = fq.focal; P.pview_half_h = fq.view_half_h;
        std::copy(fq.cam, fq.cam + 3, P.pcam);
        std::copy(meta_prev + 12, meta_prev + 28, P.pV);
    }
    P.alpha = prm.alpha; P.normal_min = prm.normal_min; P.depth_tol = prm.depth_tol; P.max_history = prm.max_history;
    return PT_OK;
}

static int reproject_launch(pt_scene* s, const float* d_accum, const float* d_m2, const float* d_geo, const float* d_alb,
                            const ReprojectParams& P, const float* const prev[3], float* const next[3], float* d_out,
                            float* d_var, hipStream_t stream) {
    HIP_TRY(hipSetDevice(s->device));
    ProfScope prof_scope(s);
    HIP_TRY(launch_reproject(d_accum, d_m2, d_geo, d_alb, P, reinterpret_cast<const float4*>(prev[0]),
                             reinterpret_cast<const float4*>(prev[1]), reinterpret_cast<const float4*>(prev[2]),
                             reinterpret_cast<float4*>(next[0]), reinterpret_cast<float4*>(next[1]),
                             reinterpret_cast<float4*>(next[2]), d_out, d_var, stream));
    return PT_OK;
}

static int denoise_mean_args(const pt_denoise_params* p, uint32_t feature_frames, uint32_t w, uint32_t h, size_t row_pitch,
                             pt_denoise_params& prm) {
    PT_TRY(denoise_params(p, feature_frames, prm));
    TileGrid g{};
    return make_grid(w, h, row_pitch, w ? w : 1, h ? h : 1, g);  // w, h and the pitch, checked as pt_denoise_async's
}

namespace pt {

void orphan_histories(pt_scene* s) {
    for (pt_history* hs : s->histories) {
        hs->release();  // while the scene is there to be counted down
        hs->scene = nullptr;
    }
    s->histories.clear();
}

}  // namespace pt

extern "C" {

void pt_temporal_defaults(pt_temporal_params* p) {
    if (p) *p = pt_temporal_params{0.2f, 0.9f, 0.1f, 64.0f};
}

int pt_reproject_async(pt_scene* s, const float* d_accum, const float* d_m2, uint32_t n, const float* d_geo, const float* d_alb,
                       const float meta_cur[48], const float* meta_prev, const float* d_hist_prev, const float* d_mom_prev,
                       const float* d_gbuf_prev, uint32_t w, uint32_t h, size_t row_pitch, const pt_temporal_params* p,
                       float* d_hist, float* d_mom, float* d_gbuf, float* d_out, float* d_var, void* stream) {
    if (!s || !d_accum || !d_m2 || !d_geo || !d_alb || !meta_cur || !d_hist || !d_mom || !d_gbuf)
        return fail(PT_ERR_INVALID, "null argument");
    const float* const prev[3] = {d_hist_prev, d_mom_prev, d_gbuf_prev};
    float* const next[3] = {d_hist, d_mom, d_gbuf};
    ReprojectParams P;
    PT_TRY(reproject_args(meta_cur, meta_prev, prev, n, w, h, row_pitch, p, next, P));
    uintptr_t bits = (uintptr_t)d_geo | (uintptr_t)d_alb;
    for (int k = 0; k < 3; ++k) bits |= (uintptr_t)prev[k] | (uintptr_t)next[k];
    if (bits & 15u) return fail(PT_ERR_INVALID, "geo, alb and the planes must be 16-byte aligned");
    return reproject_launch(s, d_accum, d_m2, d_geo, d_alb, P, prev, next, d_out, d_var, static_cast<hipStream_t>(stream));
}

int pt_reproject(pt_scene* s, const float* accum, const float* m2, uint32_t n, const float* geo, const float* alb,
                 const float meta_cur[48], const float* meta_prev, const float* hist_prev, const float* mom_prev,
                 const float* gbuf_prev, uint32_t w, uint32_t h, const pt_temporal_params* p, float* hist, float* mom,
                 float* gbuf, float* out, float* var) {
    if (!s || !accum || !m2 || !geo || !alb || !meta_cur || !hist || !mom || !gbuf) return fail(PT_ERR_INVALID, "null argument");
    const float* const hprev[3] = {hist_prev, mom_prev, gbuf_prev};
    float* const hnext[3] = {hist, mom, gbuf};
    ReprojectParams P;
    PT_TRY(reproject_args(meta_cur, meta_prev, hprev, n, w, h, w, p, hnext, P));
    const size_t npix = (size_t)w * h;
    Blocking b(s);
    PT_TRY(b.device());
    PT_TRY(s->d_temporal.ensure(42 * npix, "reprojection buffers"));
    PT_TRY(b.open());
    // the planes first (16-byte aligned whatever npix), then the three-float and one-float buffers
    float* const base = s->d_temporal.p;
    float* const d_geo = base;
    float* const d_alb = base + 4 * npix;
    float* const dprev[3] = {base + 8 * npix, base + 12 * npix, base + 16 * npix};
    float* const dnext[3] = {base + 20 * npix, base + 24 * npix, base + 28 * npix};
    float* const d_acc = base + 32 * npix;
    float* const d_m2 = base + 35 * npix;
    float* const d_out = base + 38 * npix;
    float* const d_var = base + 41 * npix;
    PT_TRY(b.in(d_acc, accum, 3 * npix * sizeof(float)));
    PT_TRY(b.in(d_m2, m2, 3 * npix * sizeof(float)));
    PT_TRY(b.in(d_geo, geo, 4 * npix * sizeof(float)));
    PT_TRY(b.in(d_alb, alb, 4 * npix * sizeof(float)));
    const float* cprev[3] = {nullptr, nullptr, nullptr};
    if (meta_prev)
        for (int k = 0; k < 3; ++k) {
            PT_TRY(b.in(dprev[k], hprev[k], 4 * npix * sizeof(float)));
            cprev[k] = dprev[k];
        }
    PT_TRY(reproject_launch(s, d_acc, d_m2, d_geo, d_alb, P, cprev, dnext, out ? d_out : nullptr, var ? d_var : nullptr,
                            s->stream));
    for (int k = 0; k < 3; ++k) PT_TRY(b.out(hnext[k], dnext[k], 4 * npix * sizeof(float)));
    if (out) PT_TRY(b.out(out, d_out, 3 * npix * sizeof(float)));
    if (var) PT_TRY(b.out(var, d_var, npix * sizeof(float)));
    return b.finish(Blocking::kNoWatchdog);  // no render of this call
}

int pt_denoise_mean_async(pt_scene* s, const float* d_c, const float* d_var, uint32_t w, uint32_t h, size_t row_pitch,
                          const float* d_geo, const float* d_alb, uint32_t feature_frames, const pt_denoise_params* p,
                          float* d_out, float* d_var_out, void* stream) {
    if (!s || !d_c || !d_var || !d_geo || !d_alb || !d_out) return fail(PT_ERR_INVALID, "null argument");
    pt_denoise_params prm;
    PT_TRY(denoise_mean_args(p, feature_frames, w, h, row_pitch, prm));
    if (((uintptr_t)d_geo | (uintptr_t)d_alb) & 15u) return fail(PT_ERR_INVALID, "geo and alb must be 16-byte aligned");
    HIP_TRY(hipSetDevice(s->device));
    float4 *cv[2], *nz, *ab;
    PT_TRY(denoise_planes(s, (size_t)w * h, cv, nz, ab));
    ProfScope prof_scope(s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(launch_denoise_prepare_mean(d_c, d_var, d_geo, d_alb, w, h, (uint32_t)row_pitch, feature_frames, cv[0], nz, ab, st));
    return denoise_passes(prm, w, h, (uint32_t)row_pitch, cv, nz, ab, d_out, d_var_out, st);
}

int pt_denoise_mean(pt_scene* s, const float* c, const float* var, uint32_t w, uint32_t h, const float* geo, const float* alb,
                    uint32_t feature_frames, const pt_denoise_params* p, float* out, float* var_out) {
    if (!s || !c || !var || !geo || !alb || !out) return fail(PT_ERR_INVALID, "null argument");
    pt_denoise_params prm;
    PT_TRY(denoise_mean_args(p, feature_frames, w, h, w, prm));
    const size_t npix = (size_t)w * h, n = 3 * npix;
    Blocking b(s);
    int rc;
    if ((rc = b.device()) != PT_OK || (rc = s->d_accum.ensure(n, "mean")) != PT_OK ||
        (rc = s->d_mean.ensure(n, "filtered image")) != PT_OK || (rc = s->d_feat.ensure(8 * npix, "guide buffers")) != PT_OK ||
        (rc = s->d_var.ensure(2 * npix, "variance")) != PT_OK || (rc = b.open()) != PT_OK)
        return rc;
    float* const d_geo = s->d_feat.p;
    float* const d_alb = s->d_feat.p + 4 * npix;
    float* const d_vin = s->d_var.p + npix;
    PT_TRY(b.in(s->d_accum.p, c, n * sizeof(float)));
    PT_TRY(b.in(d_vin, var, npix * sizeof(float)));
    PT_TRY(b.in(d_geo, geo, 4 * npix * sizeof(float)));
    PT_TRY(b.in(d_alb, alb, 4 * npix * sizeof(float)));
    PT_TRY(pt_denoise_mean_async(s, s->d_accum.p, d_vin, w, h, w, d_geo, d_alb, feature_frames, &prm, s->d_mean.p,
                                 var_out ? s->d_var.p : nullptr, s->stream));
    PT_TRY(b.out(out, s->d_mean.p, n * sizeof(float)));
    if (var_out) PT_TRY(b.out(var_out, s->d_var.p, npix * sizeof(float)));
    return b.finish(Blocking::kNoWatchdog);
}

int pt_history_create(pt_scene* s, uint32_t w, uint32_t h, pt_history** out) {
    if (!s || !out) return fail(PT_ERR_INVALID, "null argument");
    *out = nullptr;
    if (w < 1 || h < 1 || w > 32768 || h > 32768) return fail(PT_ERR_INVALID, "history: w and h must lie in [1, 32768]");
    HIP_TRY(hipSetDevice(s->device));
    const size_t npix = (size_t)w * h;
    pt_history* hs = new pt_history(s, w, h);
    int rc;
    if ((rc = hs->planes.ensure(6 * npix, "history planes")) != PT_OK ||
        (rc = hs->work.ensure(kHistoryWorkFloats * npix, "history step buffers")) != PT_OK ||
        (rc = hs->rgba.ensure(4 * npix, "history image")) != PT_OK) {
        delete hs;
        return rc;
    }
    hs->held = hs->planes.cap * sizeof(float4) + hs->work.cap * sizeof(float) + hs->rgba.cap;
    s->info.device_bytes += hs->held;
    s->histories.push_back(hs);
    *out = hs;
    return PT_OK;
}

int pt_history_reset(pt_history* hs) {
    if (!hs) return fail(PT_ERR_INVALID, "null history");
    if (!hs->scene) return fail(PT_ERR_INVALID, "history: its scene was destroyed");
    hs->has_prev = false;
    return PT_OK;
}

void pt_history_destroy(pt_history* hs) {
    if (!hs) return;
    if (pt_scene* s = hs->scene) {
        hipSetDevice(s->device);
        if (s->stream) hipStreamSynchronize(s->stream);
        s->histories.erase(std::remove(s->histories.begin(), s->histories.end(), hs), s->histories.end());
        hs->release();
    }
    delete hs;  // an orphan's buffers are gone already, and nothing of it points into the scene
}

int pt_history_step(pt_history* hs, const float meta[48], uint32_t frame0, uint32_t nframes, uint32_t stride, int max_depth,
                    int mode, uint32_t feature_frames, const pt_temporal_params* tparams, const pt_denoise_params* dparams,
                    float* mean_out, float* var_out, uint8_t* rgba_out, float* history_len_out, pt_counters* counters) {
    if (!hs || !meta) return fail(PT_ERR_INVALID, "null argument");
    pt_scene* const s = hs->scene;
    if (!s) return fail(PT_ERR_INVALID, "history: its scene was destroyed");
    if (nframes < 1) return fail(PT_ERR_INVALID, "nframes must be at least 1");
    const uint32_t w = hs->w, h = hs->h;
    const size_t npix = (size_t)w * h;
    const int nxt = hs->cur ^ 1;
    float* const pl = reinterpret_cast<float*>(hs->planes.p);
    const float* prev[3] = {nullptr, nullptr, nullptr};
    float* next[3];
    for (int k = 0; k < 3; ++k) {
        next[k] = pl + (size_t)(3 * nxt + k) * 4 * npix;
        if (hs->has_prev) prev[k] = pl + (size_t)(3 * hs->cur + k) * 4 * npix;
    }
    ReprojectParams P;
    PT_TRY(reproject_args(meta, hs->has_prev ? hs->meta_prev : nullptr, prev, nframes, w, h, w, tparams, next, P));
    pt_denoise_params dprm;
    if (dparams) PT_TRY(denoise_mean_args(dparams, feature_frames, w, h, w, dprm));
    else if (feature_frames < 1) return fail(PT_ERR_INVALID, "feature_frames must be at least 1");
    float* const wk = hs->work.p;
    float* const d_geo = wk;
    float* const d_alb = wk + 4 * npix;
    float* const d_acc = wk + 8 * npix;
    float* const d_m2 = wk + 11 * npix;
    float* const d_mean = wk + 14 * npix;
    float* const d_filt = wk + 17 * npix;
    float* const d_var = wk + 20 * npix;
    float* const d_fvar = wk + 21 * npix;
    Blocking b(s, counters);
    PT_TRY(b.device());
    PT_TRY(b.open());
    PT_TRY(b.zero(wk, 14 * npix * sizeof(float)));  // the guides and both accumulators
    PT_TRY(render_impl(s, meta, frame0, nframes, stride, max_depth, mode, true, d_acc, b.d_cnt(), s->stream, nullptr, nullptr, d_m2));
    PT_TRY(features_impl(s, meta, nullptr, nullptr, frame0, feature_frames, 1, d_geo, d_alb, b.d_cnt(), s->stream));
    PT_TRY(reproject_launch(s, d_acc, d_m2, d_geo, d_alb, P, prev, next, d_mean, d_var, s->stream));
    const float* d_res = d_mean;
    const float* d_resvar = d_var;
    if (dparams) {
        PT_TRY(pt_denoise_mean_async(s, d_mean, d_var, w, h, w, d_geo, d_alb, feature_frames, &dprm, d_filt, d_fvar, s->stream));
        d_res = d_filt;
        d_resvar = d_fvar;
    }
    if (rgba_out) {
        PT_TRY(pt_tonemap_async(s, d_res, npix, 1, hs->rgba.p, s->stream));
        PT_TRY(b.out(rgba_out, hs->rgba.p, 4 * npix));
    }
    if (mean_out) PT_TRY(b.out(mean_out, d_res, 3 * npix * sizeof(float)));
    if (var_out) PT_TRY(b.out(var_out, d_resvar, npix * sizeof(float)));
    std::vector<float> plane;  // the new hist plane on the host: its fourth component is the history length
    if (history_len_out) {
        plane.resize(4 * npix);
        PT_TRY(b.out(plane.data(), next[0], 4 * npix * sizeof(float)));
    }
    PT_TRY(b.finish(Blocking::kWatchdog));
    // the step is done and no render of it failed: only now the new set is the state (a step that fails anywhere
    // above leaves the previous set and meta in place, and the set it wrote into is written again by the next)
    std::copy(meta, meta + 48, hs->meta_prev);
    hs->has_prev = true;
    hs->cur = nxt;
    for (size_t i = 0; i < plane.size() / 4; ++i) history_len_out[i] = plane[4 * i + 3];
    return PT_OK;
}

}  // extern "C"
