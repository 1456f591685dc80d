// pt_view_plan.cpp — pt_view_plan.h: a view list checked and planned on the host.
#include "pt_view_plan.h"

#include <cmath>
#include <cstring>

#include "pt_rect_plan.h"

namespace pt {

namespace {

std::string show(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    return "(" + std::to_string(x0) + ", " + std::to_string(y0) + ", " + std::to_string(w) + ", " + std::to_string(h) + ")";
}
std::string name(size_t k) { return "views[" + std::to_string(k) + "]"; }

int invalid(std::string& err, const std::string& msg) {
    err = msg;
    return PT_ERR_INVALID;
}

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, sizeof u);
    return u;
}

}  // namespace

const char* camera_refusal(const pt_camera& cam) {
    const bool focus_ok = std::isfinite(cam.focus_distance) && cam.focus_distance > 0.0f;
    switch (cam.model) {
        case PT_CAMERA_PINHOLE: return nullptr;
        case PT_CAMERA_THIN_LENS:
            if (!std::isfinite(cam.lens_radius) || cam.lens_radius < 0.0f) return "camera: thin lens needs a finite lens_radius >= 0";
            if (!focus_ok) return "camera: thin lens needs a finite focus_distance > 0";
            return nullptr;
        case PT_CAMERA_ORTHO: return focus_ok ? nullptr : "camera: ortho needs a finite focus_distance > 0";
        case PT_CAMERA_EQUIRECT: return nullptr;
        default: return "camera: unknown model";
    }
}

int plan_views(const pt_view* views, size_t n, uint32_t atlas_w, uint32_t atlas_h, uint32_t nframes, uint32_t stride,
               ViewPlan& plan, std::string& err) {
    plan = ViewPlan{};
    if (atlas_w < 1 || atlas_h < 1 || atlas_w > 32768 || atlas_h > 32768)
        return invalid(err, "views: the atlas's width and height must lie in [1, 32768]");
    if (n == 0) return invalid(err, "views: the list is empty (n must be at least 1)");
    if (n > kMaxViews) return invalid(err, "views: " + std::to_string(n) + " views, at most " + std::to_string(kMaxViews));
    if (!views) return invalid(err, "views is NULL");
    plan.first.resize(n);
    std::vector<pt_window> dst(n);
    for (size_t k = 0; k < n; ++k) {
        const pt_view& v = views[k];
        if (v.reserved != 0) return invalid(err, name(k) + ": reserved must be 0");
        const float W = v.meta[0], H = v.meta[1];
        if (!(W >= 1.0f && H >= 1.0f && W <= 32768.0f && H <= 32768.0f) || W != std::floor(W) || H != std::floor(H))
            return invalid(err, name(k) + ": meta[0..1] must be integral resolutions in [1, 32768]");
        const pt_window& w = v.win;
        if (w.w < 1 || w.h < 1) return invalid(err, name(k) + ": window " + show(w.x0, w.y0, w.w, w.h) + ": w and h must be at least 1");
        if ((uint64_t)w.x0 + w.w > (uint32_t)W || (uint64_t)w.y0 + w.h > (uint32_t)H)
            return invalid(err, name(k) + ": window " + show(w.x0, w.y0, w.w, w.h) + " must lie within its image (" +
                                    std::to_string((uint32_t)W) + " x " + std::to_string((uint32_t)H) + ")");
        if ((uint64_t)v.dst_x + w.w > atlas_w || (uint64_t)v.dst_y + w.h > atlas_h)
            return invalid(err, name(k) + ": destination " + show(v.dst_x, v.dst_y, w.w, w.h) + " lies outside the atlas (" +
                                    std::to_string(atlas_w) + " x " + std::to_string(atlas_h) + ")");
        if (const char* why = camera_refusal(v.cam)) return invalid(err, name(k) + ": " + why);
        if ((uint64_t)v.frame0 + (uint64_t)(nframes ? nframes - 1 : 0) * stride >= (1ull << 24))
            return invalid(err, name(k) + ": frame index >= 2^24 (t_k = u32(f32(k)) would round)");
        if (bits(v.meta[45]) != bits(views[0].meta[45]))
            return invalid(err, name(k) + ": meta[45] (the continuation probability) differs from views[0]'s: it is shared by the call");
        if ((v.meta[46] > 0.0f) != (views[0].meta[46] > 0.0f))
            return invalid(err, name(k) + ": meta[46] > 0 (direct lighting only) differs from views[0]'s: it is shared by the call");
        plan.first[k] = (uint32_t)plan.npix;  // below 2^31 + 2^30 here: checked next
        plan.npix += (uint64_t)w.w * w.h;
        if (plan.npix >= (1ull << 31))
            return invalid(err, "views: " + name(0) + " .. " + name(k) + " hold 2^31 or more paths per frame");
        dst[k] = pt_window{v.dst_x, v.dst_y, w.w, w.h};
    }
    // two destinations on one pixel: the rectangle lists' sweep, over the destinations inside the atlas
    // (everything else it checks holds by now, so its one possible complaint is the overlap)
    RectPlan rects;
    std::string rerr;
    if (plan_rects(nullptr, atlas_w, atlas_h, dst.data(), n, rects, rerr) != PT_OK) {
        for (size_t at = 0; (at = rerr.find("rects[", at)) != std::string::npos; at += 6) rerr.replace(at, 6, "views[");
        return invalid(err, "destination rectangles " + rerr);
    }
    return PT_OK;
}

}  // namespace pt
