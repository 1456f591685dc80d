// pt_capi_camera.hip — C ABI (include/pt_hip.h): the scene's camera model (pt_scene_set_camera,
// pt_scene_get_camera).  The models themselves are camera_ray_model (pt_device.h); the
// calls that make camera paths read the setting through scene_camera.  Host code only.
#include <cmath>

#include "pt_capi_internal.h"
#include "pt_view_plan.h"

using namespace pt;

static_assert(sizeof(pt_camera) == 16, "pt_camera is four 32-bit words");
static_assert((uint32_t)PT_CAMERA_THIN_LENS == CAM_THIN_LENS && (uint32_t)PT_CAMERA_ORTHO == CAM_ORTHO &&
                  (uint32_t)PT_CAMERA_EQUIRECT == CAM_EQUIRECT && (uint32_t)PT_CAMERA_PINHOLE == CAM_PINHOLE,
              "pt_camera_model and the kernels' CAM_* agree");

namespace pt {

const LensCam* scene_camera(const pt_scene* s, LensCam& lc) {
    const pt_camera c = s->cam;
    if (c.model == PT_CAMERA_PINHOLE) return nullptr;
    lc.model = c.model;
    lc.lens_radius = c.lens_radius;
    lc.focus_distance = c.focus_distance;
    return &lc;
}

}  // namespace pt

extern "C" {

int pt_scene_set_camera(pt_scene* s, const pt_camera* cam) {
    if (!s) return fail(PT_ERR_INVALID, "null scene");
    if (!cam || cam->model == PT_CAMERA_PINHOLE) {
        s->cam = pt_camera{};
        return PT_OK;
    }
    if (const char* why = camera_refusal(*cam)) return fail(PT_ERR_INVALID, why);  // pt_view_plan.h: a view's camera too
    s->cam = *cam;
    return PT_OK;
}

int pt_scene_get_camera(const pt_scene* s, pt_camera* out) {
    if (!s || !out) return fail(PT_ERR_INVALID, "null argument");
    *out = s->cam;
    return PT_OK;
}

}  // extern "C"
