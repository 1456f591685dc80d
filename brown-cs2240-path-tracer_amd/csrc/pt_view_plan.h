// pt_view_plan.h — the plan of a view-list render (pt_render_views): the list checked and
// every view's first slot.  Standard C++ only, no HIP: a stand-alone program links pt_view_plan.cpp and
// pt_rect_plan.cpp (scripts/view_plan_harness.cpp, tests/test_views_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pt_hip.h"

namespace pt {

constexpr size_t kMaxViews = 65536;

struct ViewPlan {
    std::vector<uint32_t> first;  // list order: the slot of the view's first pixel
    uint64_t npix = 0;            // paths per frame: the sum of the window areas
};

// Why pt_scene_set_camera refuses cam (nullptr: it does not): the one statement of what a pt_camera must
// hold, for the scene's setting and for a view's.
const char* camera_refusal(const pt_camera& cam);

// Everything pt_render_views refuses about its list (pt_hip.h), in this order per view: reserved, the
// image's size, the window, the destination, the camera, the frames (frame0 + (nframes - 1) * stride below
// 2^24), the fields shared with view 0; then npix < 2^31 and the destinations' disjointness (plan_rects'
// sort and sweep over the destination rectangles, pt_rect_plan.h).  PT_OK, or PT_ERR_INVALID with err
// naming the offending view(s).
int plan_views(const pt_view* views, size_t n, uint32_t atlas_w, uint32_t atlas_h, uint32_t nframes, uint32_t stride,
               ViewPlan& plan, std::string& err);

}  // namespace pt
