// pt_features.hip — guide buffers of the first hit (pt_hip.h pt_render_features_async).
//
//   k_features<TRAV, COUNT>   one lane per pixel (8x8 pixels per wave, 16x16 per workgroup, the
//       megakernels' layout), frames looped in-lane.  For every frame the lane traces the camera ray
//       the render traces for that (pixel, frame) — camera_ray is a pure function of both — to its
//       closest hit with the traversal of the default megakernel instance on a scene in global memory,
//       and adds (n.xyz, t) into geo and (a.rgb, 1) into alb, four floats per pixel each, in frame
//       order from the values already there.  A miss adds nothing, so alb.w counts the hits.
//       Every traversal flavour returns the same (record, t), so one flavour per scene kind suffices.
#include "pt_kernels.h"
#include "pt_path.h"

namespace pt {

template <int TRAV, bool COUNT>
__global__ __launch_bounds__(kMegaBlock) void k_features(SceneView sc, FrameParams fp, uint32_t frame0, uint32_t nframes,
                                                        uint32_t stride, float4* __restrict__ geo,
                                                        float4* __restrict__ alb, Counters* cnt_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LStack32 stack = LStack32::make(smem, kMegaBlock);  // [max_stack][256] int32, lane-minor
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t i = blockIdx.x * 16 + (wv & 1) * 8 + (lane & 7);
    const uint32_t j = blockIdx.y * 16 + (wv >> 1) * 8 + (lane >> 3);
    const bool valid = i < fp.win_w && j < fp.win_h;
    const uint32_t x = valid ? fp.win_x0 + i : 0, y = valid ? fp.win_y0 + j : 0;
    const size_t o = valid ? (size_t)j * fp.row_pitch + i : 0;
    Counters c = {};
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a = g;
    if (valid) { g = geo[o]; a = alb[o]; }
    for (uint32_t k = 0; k < nframes; ++k) {
        if (!valid) break;
        const uint32_t t = (uint32_t)(float)(frame0 + k * stride);
        uint32_t seed;
        const Ray r = camera_ray(fp, x, y, t, seed);
        if (COUNT) { c.samples++; c.ext_queries++; }
        float th;
        const int rec = trace_any<TRAV, COUNT>(sc, r, th, stack, c);
        if (rec < 0) continue;
        const Hit h = hit_data(sc, r, rec, th);
        const Mat m = load_mat(sc, h.mat);
        const f3 col = sum3(m.Ke) > 0.0f ? m.Ke : m.Kd + m.Ks;
        g.x += h.n.x; g.y += h.n.y; g.z += h.n.z; g.w += th;
        a.x += col.x; a.y += col.y; a.z += col.z; a.w += 1.0f;
    }
    if (valid) { geo[o] = g; alb[o] = a; }
    if (COUNT) flush_counters(c, cnt_out);
}

// k_features under a lens camera: the same lanes, frames and sums, tracing
// camera_ray_model<MODEL>'s ray.  A sample whose direction is not admitted (ray_admitted) is no sample:
// it adds nothing and counts nothing, as in the render.
template <int TRAV, bool COUNT, uint32_t MODEL>
__global__ __launch_bounds__(kMegaBlock) void k_features_cam(SceneView sc, FrameParams fp, LensCam lc, uint32_t frame0,
                                                            uint32_t nframes, uint32_t stride, float4* __restrict__ geo,
                                                            float4* __restrict__ alb, Counters* cnt_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LStack32 stack = LStack32::make(smem, kMegaBlock);  // [max_stack][256] int32, lane-minor
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t i = blockIdx.x * 16 + (wv & 1) * 8 + (lane & 7);
    const uint32_t j = blockIdx.y * 16 + (wv >> 1) * 8 + (lane >> 3);
    const bool valid = i < fp.win_w && j < fp.win_h;
    const uint32_t x = valid ? fp.win_x0 + i : 0, y = valid ? fp.win_y0 + j : 0;
    const size_t o = valid ? (size_t)j * fp.row_pitch + i : 0;
    Counters c = {};
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a = g;
    if (valid) { g = geo[o]; a = alb[o]; }
    for (uint32_t k = 0; k < nframes; ++k) {
        if (!valid) break;
        const uint32_t t = (uint32_t)(float)(frame0 + k * stride);
        uint32_t seed;
        const Ray r = camera_ray_model<MODEL>(fp, lc, x, y, t, seed);
        if (!ray_admitted(r.d.x, r.d.y, r.d.z)) continue;
        if (COUNT) { c.samples++; c.ext_queries++; }
        float th;
        const int rec = trace_any<TRAV, COUNT>(sc, r, th, stack, c);
        if (rec < 0) continue;
        const Hit h = hit_data(sc, r, rec, th);
        const Mat m = load_mat(sc, h.mat);
        const f3 col = sum3(m.Ke) > 0.0f ? m.Ke : m.Kd + m.Ks;
        g.x += h.n.x; g.y += h.n.y; g.z += h.n.z; g.w += th;
        a.x += col.x; a.y += col.y; a.z += col.z; a.w += 1.0f;
    }
    if (valid) { geo[o] = g; alb[o] = a; }
    if (COUNT) flush_counters(c, cnt_out);
}

template <int TRAV>
static void launch_features_t(const SceneView& sc, const FrameParams& fp, uint32_t frame0, uint32_t nframes, uint32_t stride,
                              bool count, float4* geo, float4* alb, Counters* cnt, hipStream_t stream, const LensCam* cam) {
    const dim3 grid((fp.win_w + 15) / 16, (fp.win_h + 15) / 16), block(kMegaBlock);
    const size_t lds = (size_t)sc.max_stack * kMegaBlock * 4;
    if (cam) {
#define PT_FEAT_CAM(C, M)                                                                                                  \
    PT_LAUNCH(KID_FEATURES, stream, (k_features_cam<TRAV, C, M>), grid, block, lds, stream, sc, fp, *cam, frame0, nframes, \
              stride, geo, alb, cnt)
        if (cam->model == CAM_THIN_LENS) { if (count) PT_FEAT_CAM(true, CAM_THIN_LENS); else PT_FEAT_CAM(false, CAM_THIN_LENS); }
        else if (cam->model == CAM_ORTHO) { if (count) PT_FEAT_CAM(true, CAM_ORTHO); else PT_FEAT_CAM(false, CAM_ORTHO); }
        else { if (count) PT_FEAT_CAM(true, CAM_EQUIRECT); else PT_FEAT_CAM(false, CAM_EQUIRECT); }
#undef PT_FEAT_CAM
        return;
    }
    if (count)
        PT_LAUNCH(KID_FEATURES, stream, (k_features<TRAV, true>), grid, block, lds, stream, sc, fp, frame0, nframes, stride, geo,
                  alb, cnt);
    else
        PT_LAUNCH(KID_FEATURES, stream, (k_features<TRAV, false>), grid, block, lds, stream, sc, fp, frame0, nframes, stride, geo,
                  alb, cnt);
}

hipError_t launch_features(const SceneView& scene, const FrameParams& fp, uint32_t frame0, uint32_t nframes, uint32_t stride,
                           bool count, float* geo, float* alb, Counters* cnt, hipStream_t stream, const LensCam* cam) {
    if (cam && (cam->model < CAM_THIN_LENS || cam->model > CAM_EQUIRECT)) return hipErrorInvalidValue;
    SceneView sc = scene;
    // the megakernel's turn policy (launch_megakernel)
    if (sc.node_bias <= 0) sc.node_bias = 8;
    if (sc.node_steps <= 0) sc.node_steps = 1;
    float4* const g4 = reinterpret_cast<float4*>(geo);
    float4* const a4 = reinterpret_cast<float4*>(alb);
    // the default megakernel instance of the scene: lean4, the fast reciprocal where the scene allows
    // it, cooperative turns where it has big leaves
    switch (select_megakernel(LaunchOpts{}, sc.fast_rcp != 0, sc.mailbox != 0, sc.big_leaf > 0, false)) {
        case flavour(FLV_PLAIN, TRAV_LEAN4, false):
            launch_features_t<flavour(FLV_PLAIN, TRAV_LEAN4, false)>(sc, fp, frame0, nframes, stride, count, g4, a4, cnt, stream, cam);
            break;
        case flavour(FLV_PLAIN, TRAV_LEAN4, true):
            launch_features_t<flavour(FLV_PLAIN, TRAV_LEAN4, true)>(sc, fp, frame0, nframes, stride, count, g4, a4, cnt, stream, cam);
            break;
        case flavour(FLV_BIG, TRAV_LEAN4, true):
            launch_features_t<flavour(FLV_BIG, TRAV_LEAN4, true)>(sc, fp, frame0, nframes, stride, count, g4, a4, cnt, stream, cam);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace pt
