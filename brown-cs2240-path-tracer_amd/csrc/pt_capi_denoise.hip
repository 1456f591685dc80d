// pt_capi_denoise.hip — C ABI (include/pt_hip.h): the guide buffers and the denoiser (pt_features.hip,
// pt_denoise.hip).  Host code only.
#include <cmath>

#include "pt_capi_internal.h"

using namespace pt;

// option denoise_lds: how many of the denoiser's first passes stage their taps in LDS (0..4).  Measured at
// 1024^2 (profiles/denoise_bench.jsonl): staged, the passes with steps 1 and 2 take 0.06 ms
// against 0.10 and 0.09; the pass with step 4 is 4-13 % slower staged, the one with step 8 two thirds slower
constexpr long kDenoiseLdsDefault = 2;

static int check_denoise(const pt_denoise_params& p, uint32_t feature_frames) {
    if (p.iters < 1 || p.iters > 5) return fail(PT_ERR_INVALID, "pt_denoise_params: iters must lie in [1, 5]");
    const float sg[4] = {p.sigma_n, p.sigma_a, p.sigma_z, p.sigma_l};
    static const char* const names[4] = {"sigma_n", "sigma_a", "sigma_z", "sigma_l"};
    for (int k = 0; k < 4; ++k)
        if (!(std::isfinite(sg[k]) && sg[k] > 0.0f))
            return fail(PT_ERR_INVALID, std::string("pt_denoise_params: ") + names[k] + " must be finite and > 0");
    if (feature_frames < 1) return fail(PT_ERR_INVALID, "feature_frames must be at least 1");
    return PT_OK;
}

namespace pt {

// the call's parameters: the defaults, the caller's over them (p nullable), checked
int denoise_params(const pt_denoise_params* p, uint32_t feature_frames, pt_denoise_params& out) {
    pt_denoise_defaults(&out);
    if (p) out = *p;
    return check_denoise(out, feature_frames);
}

int features_impl(pt_scene* s, const float* meta, const pt_window* win, const size_t* pitch, uint32_t frame0,
                  uint32_t nframes, uint32_t stride, float* d_geo, float* d_alb, Counters* d_cnt, hipStream_t stream) {
    FrameParams fp{};
    int rc = make_params(meta, 0, fp, win, pitch);
    if (rc != PT_OK) return rc;
    PT_TRY(check_frames(frame0, nframes, stride));
    if (((uintptr_t)d_geo | (uintptr_t)d_alb) & 15u) return fail(PT_ERR_INVALID, "geo and alb must be 16-byte aligned");
    HIP_TRY(hipSetDevice(s->device));
    if (nframes == 0) return PT_OK;
    ProfScope prof_scope(s);
    // the scene as the default megakernel instance sees it: no option chooses this kernel's flavour
    SceneView view;
    if ((rc = shape_view(s, Opts{}, fp, PT_MODE_MEGAKERNEL, (uint64_t)fp.win_w * fp.win_h * nframes, view)) != PT_OK) return rc;
    if ((rc = take_watchdog(s)) != PT_OK) return rc;  // an earlier asynchronous render failed
    LensCam lens;  // pt_scene_set_camera: the guides follow the model's rays
    HIP_TRY(launch_features(view, fp, frame0, nframes, stride, d_cnt != nullptr, d_geo, d_alb, d_cnt, stream,
                            scene_camera(s, lens)));
    return PT_OK;
}

// the scene's four planes for a w x h image: two ping-pong (c, var), (N, Z), (A, 0)
int denoise_planes(pt_scene* s, size_t npix, float4* cv[2], float4*& nz, float4*& ab) {
    PT_TRY(s->d_dn.ensure(4 * npix, "denoiser planes"));  // (counted in info.device_bytes)
    cv[0] = s->d_dn.p; cv[1] = s->d_dn.p + npix;
    nz = s->d_dn.p + 2 * npix;
    ab = s->d_dn.p + 3 * npix;
    return PT_OK;
}

// the passes over the prepared planes (cv[0] holds the first pass's input)
int denoise_passes(const pt_denoise_params& prm, uint32_t w, uint32_t h, uint32_t row_pitch, float4* const cv[2],
                   const float4* nz, const float4* ab, float* d_out, float* d_var_out, hipStream_t st) {
    // host constants: double, rounded once
    const float isn = (float)(1.0 / ((double)prm.sigma_n * (double)prm.sigma_n));
    const float isa = (float)(1.0 / ((double)prm.sigma_a * (double)prm.sigma_a));
    const float isz = (float)(1.0 / (double)prm.sigma_z);
    // option denoise_lds = v: the first v passes (steps 1 .. 2^(v-1)) read their taps through LDS
    const uint32_t staged = (uint32_t)opts_snapshot().num("denoise_lds", kDenoiseLdsDefault);
    for (uint32_t i = 0; i < prm.iters; ++i) {
        const uint32_t step = 1u << i;
        const bool last = i + 1 == prm.iters;
        HIP_TRY(launch_atrous(cv[i & 1], nz, ab, w, h, step, isn, isa, isz, prm.sigma_l, i < staged && atrous_can_stage(step),
                              last ? nullptr : cv[(i & 1) ^ 1], last ? d_out : nullptr, last ? d_var_out : nullptr,
                              row_pitch, st));
    }
    return PT_OK;
}

}  // namespace pt

extern "C" {

int pt_render_features_async(pt_scene* s, const float meta[48], const pt_window* win, uint32_t frame0, uint32_t nframes,
                             uint32_t frame_stride, float* d_geo, float* d_alb, size_t row_pitch, pt_counters* d_counters,
                             void* stream) {
    if (!s || !meta || !d_geo || !d_alb) return fail(PT_ERR_INVALID, "null argument");
    return features_impl(s, meta, win, &row_pitch, frame0, nframes, frame_stride, d_geo, d_alb,
                         reinterpret_cast<Counters*>(d_counters), static_cast<hipStream_t>(stream));
}

int pt_render_features(pt_scene* s, const float meta[48], const pt_window* win, uint32_t frame0, uint32_t nframes,
                       uint32_t frame_stride, float* geo, float* alb, pt_counters* counters) {
    if (!s || !meta || !geo || !alb) return fail(PT_ERR_INVALID, "null argument");
    FrameParams fp{};
    PT_TRY(make_params(meta, 0, fp, win));
    const size_t n = (size_t)4 * fp.win_w * fp.win_h;
    Blocking b(s, counters);
    PT_TRY(b.device());
    PT_TRY(s->d_feat.ensure(2 * n, "guide buffers"));
    PT_TRY(b.open());
    float* const d_geo = s->d_feat.p;
    float* const d_alb = s->d_feat.p + n;
    PT_TRY(b.in(d_geo, geo, n * sizeof(float)));
    PT_TRY(b.in(d_alb, alb, n * sizeof(float)));
    PT_TRY(features_impl(s, meta, win, nullptr, frame0, nframes, frame_stride, d_geo, d_alb, b.d_cnt(), s->stream));
    PT_TRY(b.out(geo, d_geo, n * sizeof(float)));
    PT_TRY(b.out(alb, d_alb, n * sizeof(float)));
    return b.finish(Blocking::kWatchdog);
}

void pt_denoise_defaults(pt_denoise_params* p) {
    if (p) *p = pt_denoise_params{4u, 0.5f, 0.3f, 0.1f, 4.0f};
}

int pt_denoise_async(pt_scene* s, const float* d_accum, const float* d_m2, uint32_t w, uint32_t h, size_t row_pitch,
                     uint32_t tile_w, uint32_t tile_h, const uint32_t* d_frames, const float* d_geo, const float* d_alb,
                     uint32_t feature_frames, const pt_denoise_params* p, float* d_out, float* d_var_out, void* stream) {
    if (!s || !d_accum || !d_m2 || !d_frames || !d_geo || !d_alb || !d_out) return fail(PT_ERR_INVALID, "null argument");
    pt_denoise_params prm;
    TileGrid g{};
    PT_TRY(denoise_params(p, feature_frames, prm));
    PT_TRY(make_grid(w, h, row_pitch, tile_w, tile_h, g));
    if (((uintptr_t)d_geo | (uintptr_t)d_alb) & 15u) return fail(PT_ERR_INVALID, "geo and alb must be 16-byte aligned");
    const size_t npix = (size_t)w * h;
    HIP_TRY(hipSetDevice(s->device));
    float4 *cv[2], *nz, *ab;
    PT_TRY(denoise_planes(s, npix, cv, nz, ab));
    ProfScope prof_scope(s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(launch_denoise_prepare(d_accum, d_m2, d_geo, d_alb, g, d_frames, feature_frames, cv[0], nz, ab, st));
    return denoise_passes(prm, w, h, g.row_pitch, cv, nz, ab, d_out, d_var_out, st);
}

int pt_denoise(pt_scene* s, const float* accum, const float* m2, uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h,
               const uint32_t* frames, const float* geo, const float* alb, uint32_t feature_frames,
               const pt_denoise_params* p, float* out, float* var_out) {
    if (!s || !accum || !m2 || !frames || !geo || !alb || !out) return fail(PT_ERR_INVALID, "null argument");
    pt_denoise_params prm;
    TileGrid g{};
    PT_TRY(denoise_params(p, feature_frames, prm));
    PT_TRY(make_grid(w, h, w, tile_w, tile_h, g));
    const size_t npix = (size_t)w * h, n = 3 * npix, T = (size_t)g.tx * g.ty;
    Blocking b(s);
    pt_tile_noise* d_noise = nullptr;
    uint32_t* d_frames = nullptr;
    int rc;
    if ((rc = b.device()) != PT_OK || (rc = s->d_accum.ensure(n, "accumulator")) != PT_OK ||
        (rc = s->d_m2.ensure(n, "second moments")) != PT_OK || (rc = s->d_mean.ensure(n, "filtered image")) != PT_OK ||
        (rc = s->d_feat.ensure(8 * npix, "guide buffers")) != PT_OK || (rc = s->d_var.ensure(npix, "filtered variance")) != PT_OK ||
        (rc = ensure_tiles(s, T, d_noise, d_frames)) != PT_OK || (rc = b.open()) != PT_OK)
        return rc;
    float* const d_geo = s->d_feat.p;
    float* const d_alb = s->d_feat.p + 4 * npix;
    PT_TRY(b.in(s->d_accum.p, accum, n * sizeof(float)));
    PT_TRY(b.in(s->d_m2.p, m2, n * sizeof(float)));
    PT_TRY(b.in(d_geo, geo, 4 * npix * sizeof(float)));
    PT_TRY(b.in(d_alb, alb, 4 * npix * sizeof(float)));
    PT_TRY(b.in(d_frames, frames, T * sizeof(uint32_t)));
    PT_TRY(pt_denoise_async(s, s->d_accum.p, s->d_m2.p, w, h, w, tile_w, tile_h, d_frames, d_geo, d_alb, feature_frames, &prm,
                            s->d_mean.p, var_out ? s->d_var.p : nullptr, s->stream));
    PT_TRY(b.out(out, s->d_mean.p, n * sizeof(float)));
    if (var_out) PT_TRY(b.out(var_out, s->d_var.p, npix * sizeof(float)));
    return b.finish(Blocking::kNoWatchdog);  // no render of this call: the next call of the scene takes the watchdog
}

int pt_render_denoised_image(pt_scene* s, const float meta[48], uint32_t frame0, uint32_t nframes, uint32_t frame_stride,
                             int max_depth, int mode, uint32_t feature_frames, const pt_denoise_params* params,
                             uint8_t* rgba, pt_counters* counters) {
    if (!s || !meta || !rgba) return fail(PT_ERR_INVALID, "null argument");
    if (nframes < 2) return fail(PT_ERR_INVALID, "nframes must be at least 2 (the variance needs two samples)");
    pt_denoise_params prm;
    PT_TRY(denoise_params(params, feature_frames, prm));
    FrameParams fp{};
    PT_TRY(make_params(meta, max_depth, fp));
    const uint32_t W = fp.width, H = fp.height;
    const size_t npix = (size_t)W * H, n = 3 * npix;
    Blocking b(s, counters);
    pt_tile_noise* d_noise = nullptr;
    uint32_t* d_frames = nullptr;
    int rc;
    if ((rc = b.device()) != PT_OK || (rc = s->d_accum.ensure(n, "accumulator")) != PT_OK ||
        (rc = s->d_m2.ensure(n, "second moments")) != PT_OK || (rc = s->d_mean.ensure(n, "filtered image")) != PT_OK ||
        (rc = s->d_feat.ensure(8 * npix, "guide buffers")) != PT_OK || (rc = s->d_rgba.ensure(4 * npix, "image")) != PT_OK ||
        (rc = ensure_tiles(s, 1, d_noise, d_frames)) != PT_OK || (rc = b.open()) != PT_OK)
        return rc;
    float* const d_geo = s->d_feat.p;
    float* const d_alb = s->d_feat.p + 4 * npix;
    PT_TRY(b.zero(s->d_accum.p, n * sizeof(float)));
    PT_TRY(b.zero(s->d_m2.p, n * sizeof(float)));
    PT_TRY(b.zero(s->d_feat.p, 8 * npix * sizeof(float)));
    PT_TRY(b.in(d_frames, &nframes, sizeof(uint32_t)));
    PT_TRY(render_impl(s, meta, frame0, nframes, frame_stride, max_depth, mode, true, s->d_accum.p, b.d_cnt(), s->stream, nullptr,
                       nullptr, s->d_m2.p));
    PT_TRY(features_impl(s, meta, nullptr, nullptr, frame0, feature_frames, 1, d_geo, d_alb, b.d_cnt(), s->stream));
    PT_TRY(pt_denoise_async(s, s->d_accum.p, s->d_m2.p, W, H, W, W, H, d_frames, d_geo, d_alb, feature_frames, &prm, s->d_mean.p,
                            nullptr, s->stream));
    PT_TRY(pt_tonemap_async(s, s->d_mean.p, npix, 1, s->d_rgba.p, s->stream));
    PT_TRY(b.out(rgba, s->d_rgba.p, 4 * npix));
    return b.finish(Blocking::kWatchdog);
}

}  // extern "C"
