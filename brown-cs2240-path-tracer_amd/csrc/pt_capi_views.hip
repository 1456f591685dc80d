// pt_capi_views.hip — C ABI (include/pt_hip.h): view-list renders (pt_render_views, pt_render_views_async,
// pt_selftest_view_plan).  The list is checked and planned by pt_view_plan.cpp; here every
// view's meta goes through make_params — the one place that turns a meta into camera fields — into its row
// of the device table, and the call takes the wavefront route of a lens camera.  Host code only.
#include "pt_capi_internal.h"
#include "pt_view_plan.h"

using namespace pt;

static_assert(sizeof(pt_view) == 240, "pt_view: meta, window, camera, four words");

namespace pt {

// the list as a call of nframes frames checks it, before anything is launched or copied
static int plan_call(const pt_view* views, size_t n, uint32_t atlas_w, uint32_t atlas_h, uint32_t nframes, uint32_t stride,
                     int max_depth, int mode, const size_t* pitch, ViewPlan& plan) {
    std::string err;
    if (const int rc = plan_views(views, n, atlas_w, atlas_h, nframes, stride, plan, err); rc != PT_OK) return fail(rc, err);
    if (pitch && *pitch < atlas_w) return fail(PT_ERR_INVALID, "views: row_pitch is smaller than the atlas's width");
    if (pitch && *pitch > 0xffffffffull) return fail(PT_ERR_INVALID, "views: row_pitch out of range");
    if (max_depth < -1 || max_depth > 1024) return fail(PT_ERR_INVALID, "max_depth out of range");
    if (mode != PT_MODE_AUTO && mode != PT_MODE_MEGAKERNEL && mode != PT_MODE_WAVEFRONT)
        return fail(PT_ERR_INVALID, "unknown mode");
    return PT_OK;
}

// The rows of the device table: each view's FrameParams from make_params (view_half_h as every render
// computes it), its window, destination, first frame and camera.  fp0: view 0's parameters.
static int make_rows(const pt_view* views, const ViewPlan& plan, int max_depth, std::vector<ViewRow>& rows, FrameParams& fp0) {
    rows.resize(plan.first.size());
    for (size_t k = 0; k < rows.size(); ++k) {
        const pt_view& v = views[k];
        FrameParams fp{};
        PT_TRY(make_params(v.meta, max_depth, fp, &v.win));
        if (k == 0) fp0 = fp;
        ViewRow& r = rows[k];
        r = ViewRow{};
        r.first = plan.first[k];
        r.x0 = v.win.x0; r.y0 = v.win.y0; r.w = v.win.w; r.h = v.win.h;
        r.dst_x = v.dst_x; r.dst_y = v.dst_y;
        r.frame0 = v.frame0;
        r.W = fp.W; r.H = fp.H; r.inv_w = fp.inv_w; r.inv_h = fp.inv_h;
        r.aspect = fp.aspect; r.focal = fp.focal; r.view_half_h = fp.view_half_h;
        r.model = v.cam.model;
        for (int i = 0; i < 4; ++i) r.cam[i] = fp.cam[i];
        for (int i = 0; i < 16; ++i) r.M[i] = fp.M[i];
        r.width = fp.width; r.height = fp.height;
        r.lens_radius = v.cam.lens_radius;
        r.focus_distance = v.cam.focus_distance;
    }
    return PT_OK;
}

static int render_views_impl(pt_scene* s, const pt_view* views, const ViewPlan& plan, uint32_t nframes, uint32_t stride,
                             int max_depth, float* d_out, size_t row_pitch, Counters* d_cnt, hipStream_t stream) {
    std::vector<ViewRow> rows;
    FrameParams fp0{};
    PT_TRY(make_rows(views, plan, max_depth, rows, fp0));
    HIP_TRY(hipSetDevice(s->device));
    if (nframes == 0) return PT_OK;
    ProfScope prof_scope(s);
    const Opts o = opts_snapshot();
    // the wavefront pipeline with camera paths from the generate kernel, whatever the mode and the options
    // kernel, fuse_gen and regen say — a lens camera's route.  The leaf pass is chosen through view 0's
    // camera, once (the choice changes kernels, never bits; a probe per view would hold the scene's mutex
    // n times)
    WfCall c;
    PT_TRY(c.open(s, o, fp0, PT_MODE_WAVEFRONT, plan.npix, nframes));
    c.lo.wavefront = true;
    c.lo.literal = false;
    // the table, on the call's stream before its first launch; the host rows are pageable, so the runtime
    // has read them when hipMemcpyAsync returns (as for a rectangle list)
    PT_TRY(s->d_views.ensure(rows.size() * sizeof(ViewRow), "view table"));
    HIP_TRY(hipMemcpyAsync(s->d_views.p, rows.data(), rows.size() * sizeof(ViewRow), hipMemcpyHostToDevice, stream));
    ViewList vl{};
    vl.rows = reinterpret_cast<const ViewRow*>(s->d_views.p);
    vl.n = (uint32_t)rows.size();
    vl.npix = (uint32_t)plan.npix;
    // what the kernels after the generate kernel read of FrameParams, and the atlas's pitch; no view's image
    // or camera travels here
    FrameParams fp{};
    fp.rr_prob = fp0.rr_prob;
    fp.direct_only = fp0.direct_only;
    fp.max_depth = fp0.max_depth;
    fp.row_pitch = (uint32_t)row_pitch;
    return c.run(s, o, fp, PathSource(vl), 0, stride, true, d_out, d_cnt, stream);
}

}  // namespace pt

extern "C" {

int pt_render_views_async(pt_scene* s, const pt_view* views, size_t n, uint32_t atlas_w, uint32_t atlas_h, uint32_t nframes,
                          uint32_t frame_stride, int max_depth, int mode, float* d_accum, size_t row_pitch,
                          pt_counters* d_counters, void* stream) {
    if (!s || !d_accum) return fail(PT_ERR_INVALID, "null argument");
    ViewPlan plan;
    PT_TRY(plan_call(views, n, atlas_w, atlas_h, nframes, frame_stride, max_depth, mode, &row_pitch, plan));
    return render_views_impl(s, views, plan, nframes, frame_stride, max_depth, d_accum, row_pitch,
                             reinterpret_cast<Counters*>(d_counters), static_cast<hipStream_t>(stream));
}

int pt_render_views(pt_scene* s, const pt_view* views, size_t n, uint32_t atlas_w, uint32_t atlas_h, uint32_t nframes,
                    uint32_t frame_stride, int max_depth, int mode, float* accum, pt_counters* counters) {
    if (!s || !accum) return fail(PT_ERR_INVALID, "null argument");
    ViewPlan plan;  // planned and checked here, before anything is copied
    PT_TRY(plan_call(views, n, atlas_w, atlas_h, nframes, frame_stride, max_depth, mode, nullptr, plan));
    const size_t floats = 3 * (size_t)atlas_w * atlas_h, bytes = floats * sizeof(float);
    Blocking b(s, counters);
    PT_TRY(b.device());
    PT_TRY(s->d_accum.ensure(floats, "accumulator"));
    PT_TRY(b.open());
    PT_TRY(b.in(s->d_accum.p, accum, bytes));
    PT_TRY(render_views_impl(s, views, plan, nframes, frame_stride, max_depth, s->d_accum.p, atlas_w, b.d_cnt(), s->stream));
    PT_TRY(b.out(accum, s->d_accum.p, bytes));
    return b.finish(Blocking::kWatchdog);
}

int pt_selftest_view_plan(const pt_view* views, size_t n, uint32_t atlas_w, uint32_t atlas_h, uint64_t* first_out,
                          uint64_t* npix_out) {
    ViewPlan plan;
    std::string err;
    if (const int rc = plan_views(views, n, atlas_w, atlas_h, 1, 1, plan, err); rc != PT_OK) return fail(rc, err);
    for (size_t k = 0; first_out && k < n; ++k) first_out[k] = plan.first[k];
    if (npix_out) *npix_out = plan.npix;
    return PT_OK;
}

}  // extern "C"
