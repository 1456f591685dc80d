"""pt_amd — Python host binding of the MI355X path-tracing core (libpt_hip.so).

Mirrors the reference's render-path interface (src/program-raymarch.ts:50-54,
`programEntry(screenDimension, ctx, primitive_data, camera_data, scene_description)`)
for Python callers: `Scene` wraps one uploaded `SceneObjectPacked`
(triangle_data + bvh_data, src/ts-util/data-structs.ts:46-50), `Scene.render`
is the render_loop of program-raymarch.ts:226-335 without per-frame readback,
`tonemap` is its display transform (:295-316).

The product path never falls back to CPU code: if libpt_hip.so is missing or
no GPU is visible, calls raise `PtError`.
"""
from ._lib import (  # noqa: F401
    ABI_VERSION,
    Adaptive,
    CAMERA_MODELS,
    Camera,
    MODE_AUTO,
    MODE_MEGAKERNEL,
    MODE_WAVEFRONT,
    Counters,
    DenoiseParams,
    HIT_DTYPE,
    History,
    Hit,
    PtError,
    RAY_DTYPE,
    RadianceParams,
    Ray,
    Scene,
    SceneInfo,
    TILE_NOISE_DTYPE,
    TemporalParams,
    TileNoise,
    View,
    Window,
    abi_version,
    build_id,
    bvh_build,
    denoise_defaults,
    device_count,
    get_option,
    lib_path,
    load_library,
    options,
    rect_plan,
    release_communicators,
    render_multi,
    render_tiled,
    reset_options,
    selftest_math,
    selftest_rcp,
    selftest_valu,
    selftest_view_half_h,
    set_hw_queues,
    set_option,
    source_hash,
    temporal_defaults,
    tile_rects,
    tonemap,
    view_atlas,
    view_plan,
    unit_rays,
    gather_points,
    sh9_basis,
    sh9_irradiance,
    GATHER_MODES,
)
from .host import PackedScene, load_scene, program_entry  # noqa: F401
