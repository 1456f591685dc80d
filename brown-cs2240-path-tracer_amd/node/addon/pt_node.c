/*
 * pt_node.c — N-API addon (N-API v8, Node >= 12.22) binding include/pt_hip.h for the Node
 * host.  This is the thin layer between the reference-shaped JS API (node/lib/program-entry.js,
 * replacing src/program-raymarch.ts:50-357) and libpt_hip.so.  Typed arrays are passed
 * through without copies; render() runs as napi_async_work off the event loop and resolves a
 * Promise (the reference's mapAsync().then chain, program-raymarch.ts:273).  Errors become JS
 * Error objects carrying pt_last_error().
 */
#include <node_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/pt_hip.h"

#define CHECK_NAPI(env, call)                                                  \
    do {                                                                       \
        if ((call) != napi_ok) {                                               \
            napi_throw_error((env), NULL, "N-API call failed: " #call);        \
            return NULL;                                                       \
        }                                                                      \
    } while (0)

static napi_value throw_pt(napi_env env, int rc) {
    char buf[512];
    snprintf(buf, sizeof buf, "pt_hip error %d: %s", rc, pt_last_error());
    napi_throw_error(env, NULL, buf);
    return NULL;
}

static int get_f32(napi_env env, napi_value v, float** data, size_t* len) {
    bool is_ta = false;
    if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return 0;
    napi_typedarray_type t;
    void* p;
    napi_value ab;
    size_t off;
    if (napi_get_typedarray_info(env, v, &t, len, &p, &ab, &off) != napi_ok || t != napi_float32_array) return 0;
    *data = (float*)p;
    return 1;
}

static int get_u8(napi_env env, napi_value v, uint8_t** data, size_t* len) {
    bool is_ta = false;
    if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return 0;
    napi_typedarray_type t;
    void* p;
    napi_value ab;
    size_t off;
    if (napi_get_typedarray_info(env, v, &t, len, &p, &ab, &off) != napi_ok ||
        (t != napi_uint8_array && t != napi_uint8_clamped_array))
        return 0;
    *data = (uint8_t*)p;
    return 1;
}

static int get_i32(napi_env env, napi_value v, int32_t* out) { return napi_get_value_int32(env, v, out) == napi_ok; }
static int get_u32(napi_env env, napi_value v, uint32_t* out) { return napi_get_value_uint32(env, v, out) == napi_ok; }

/* A JS scene handle: the library's scene plus the addon's job guard.  Calls on one pt_scene are
 * not re-entrant (include/pt_hip.h), and render()/renderImage() run on libuv worker threads, so
 * a second job on a scene whose job is still running is rejected (busy), and so are
 * renderSync()/frame()/sceneDestroy() while one runs.  All of these checks run on the JS thread,
 * which also clears `busy` when the job completes: no locking needed. */
typedef struct {
    pt_scene* s;
    int busy;
} scene_box;

static void scene_finalize(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    scene_box* b = (scene_box*)data;
    if (b->s) pt_scene_destroy(b->s);
    free(b);
}

static scene_box* get_box(napi_env env, napi_value v) {
    void* p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok) return NULL;
    return (scene_box*)p;
}

/* the live scene of a handle: NULL (and a pending JS error) if destroyed or busy */
static pt_scene* get_scene(napi_env env, napi_value v) {
    scene_box* b = get_box(env, v);
    if (!b) return NULL;
    if (!b->s) { napi_throw_error(env, NULL, "scene was destroyed (sceneDestroy)"); return NULL; }
    if (b->busy) { napi_throw_error(env, NULL, "scene is busy: a render job on it has not completed"); return NULL; }
    return b->s;
}

static int pending_exception(napi_env env) {
    bool p = false;
    return napi_is_exception_pending(env, &p) == napi_ok && p;
}

static napi_value counters_obj(napi_env env, const pt_counters* c) {
    napi_value o, v;
    napi_create_object(env, &o);
    const char* names[6] = {"samples", "ext_queries", "shadow_queries", "nodes", "tri_tests", "box_tests"};
    const uint64_t vals[6] = {c->samples, c->ext_queries, c->shadow_queries, c->nodes, c->tri_tests, c->box_tests};
    for (int i = 0; i < 6; ++i) {
        napi_create_double(env, (double)vals[i], &v);
        napi_set_named_property(env, o, names[i], v);
    }
    return o;
}

/* abiVersion() -> number */
static napi_value js_abi_version(napi_env env, napi_callback_info info) {
    (void)info;
    napi_value r;
    CHECK_NAPI(env, napi_create_int32(env, pt_abi_version(), &r));
    return r;
}

/* setOption(name, value | null) — pt_set_option (kernel-selection switches; null = default) */
static napi_value js_set_option(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    char name[64], value[64];
    size_t n = 0;
    if (argc < 1 || napi_get_value_string_utf8(env, argv[0], name, sizeof name, &n) != napi_ok) {
        napi_throw_type_error(env, NULL, "setOption(name: string, value: string | number | null)");
        return NULL;
    }
    const char* v = NULL;
    napi_valuetype t = napi_undefined;
    if (argc >= 2) CHECK_NAPI(env, napi_typeof(env, argv[1], &t));
    if (t == napi_string) {
        if (napi_get_value_string_utf8(env, argv[1], value, sizeof value, &n) != napi_ok) return NULL;
        v = value;
    } else if (t == napi_number) {
        int64_t x = 0;
        CHECK_NAPI(env, napi_get_value_int64(env, argv[1], &x));
        snprintf(value, sizeof value, "%lld", (long long)x);
        v = value;
    } else if (t != napi_null && t != napi_undefined) {
        napi_throw_type_error(env, NULL, "setOption: value must be a string, a number or null");
        return NULL;
    }
    int rc = pt_set_option(name, v);
    if (rc) return throw_pt(env, rc);
    return NULL;
}

/* deviceCount() -> number */
static napi_value js_device_count(napi_env env, napi_callback_info info) {
    (void)info;
    int n = 0;
    int rc = pt_device_count(&n);
    if (rc) return throw_pt(env, rc);
    napi_value r;
    CHECK_NAPI(env, napi_create_int32(env, n, &r));
    return r;
}

/* a new scene as the external the other calls take; the scene is destroyed if that fails */
static napi_value wrap_scene(napi_env env, pt_scene* s) {
    scene_box* b = (scene_box*)calloc(1, sizeof(scene_box));
    if (!b) { pt_scene_destroy(s); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    b->s = s;
    napi_value ext;
    if (napi_create_external(env, b, scene_finalize, NULL, &ext) != napi_ok) {
        pt_scene_destroy(s);
        free(b);
        napi_throw_error(env, NULL, "napi_create_external failed");
        return NULL;
    }
    /* V8 cannot see device memory: tell it, so that dropped scenes are collected */
    pt_scene_info si;
    if (pt_scene_get_info(s, &si) == PT_OK) {
        int64_t adj = 0;
        napi_adjust_external_memory(env, (int64_t)si.device_bytes, &adj);
    }
    return ext;
}

/* sceneCreate(triangle_data: Float32Array, bvh_data: Float32Array, device: number) -> external */
static napi_value js_scene_create(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float *tri, *bvh;
    size_t tl, bl;
    int32_t dev = 0;
    if (argc < 2 || !get_f32(env, argv[0], &tri, &tl) || !get_f32(env, argv[1], &bvh, &bl) ||
        (argc > 2 && !get_i32(env, argv[2], &dev))) {
        napi_throw_type_error(env, NULL, "sceneCreate(Float32Array triangle_data, Float32Array bvh_data, device?)");
        return NULL;
    }
    pt_scene* s = NULL;
    int rc = pt_scene_create(tri, tl, bvh, bl, dev, &s);
    if (rc) return throw_pt(env, rc);
    return wrap_scene(env, s);
}

/* the optional {maxLeaf, isolateEmitters} of the LBVH calls over pt_build_defaults; false: a type error is pending */
static bool get_build_params(napi_env env, napi_value v, pt_build_params* prm) {
    pt_build_defaults(prm);
    napi_valuetype t = napi_undefined;
    if (v && napi_typeof(env, v, &t) != napi_ok) return false;
    if (t == napi_undefined || t == napi_null) return true;
    bool has = false;
    napi_value f;
    if (t != napi_object) goto bad;
    if (napi_has_named_property(env, v, "maxLeaf", &has) == napi_ok && has) {
        int32_t m = 0;
        if (napi_get_named_property(env, v, "maxLeaf", &f) != napi_ok || !get_i32(env, f, &m) || m < 0) goto bad;
        prm->max_leaf = (uint32_t)m;
    }
    if (napi_has_named_property(env, v, "isolateEmitters", &has) == napi_ok && has) {
        bool iso = true;
        if (napi_get_named_property(env, v, "isolateEmitters", &f) != napi_ok || napi_get_value_bool(env, f, &iso) != napi_ok) goto bad;
        prm->isolate_emitters = iso ? 1 : 0;
    }
    return true;
bad:
    napi_throw_type_error(env, NULL, "build options: { maxLeaf?: number, isolateEmitters?: boolean }");
    return false;
}

/* sceneCreateMesh(triangle_data: Float32Array[, {maxLeaf, isolateEmitters}[, device]]) -> external: the
 * scene's tree (the LBVH of pt_hip.h) and records built on the device, pt_scene_create_mesh */
static napi_value js_scene_create_mesh(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float* tri;
    size_t tl;
    int32_t dev = 0;
    if (argc < 1 || !get_f32(env, argv[0], &tri, &tl) || (argc > 2 && !get_i32(env, argv[2], &dev))) {
        napi_throw_type_error(env, NULL, "sceneCreateMesh(Float32Array triangle_data, options?, device?)");
        return NULL;
    }
    pt_build_params prm;
    if (!get_build_params(env, argc > 1 ? argv[1] : NULL, &prm)) return NULL;
    pt_scene* s = NULL;
    int rc = pt_scene_create_mesh(tri, tl, &prm, dev, &s);
    if (rc) return throw_pt(env, rc);
    return wrap_scene(env, s);
}

/* sceneExportBvh(scene) -> Float32Array: the packed tree of a scene made by sceneCreateMesh */
static napi_value js_scene_export_bvh(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    pt_scene* s = argc ? get_scene(env, argv[0]) : NULL;
    if (!s) {
        if (!pending_exception(env)) napi_throw_type_error(env, NULL, "sceneExportBvh(scene)");
        return NULL;
    }
    size_t len = 0;
    int rc = pt_scene_export_bvh(s, NULL, 0, &len);
    if (rc) return throw_pt(env, rc);
    napi_value buf, arr;
    void* data = NULL;
    CHECK_NAPI(env, napi_create_arraybuffer(env, len * sizeof(float), &data, &buf));
    rc = pt_scene_export_bvh(s, (float*)data, len, &len);
    if (rc) return throw_pt(env, rc);
    CHECK_NAPI(env, napi_create_typedarray(env, napi_float32_array, len, buf, 0, &arr));
    return arr;
}

/* bvhBuildLbvh(triangle_data: Float32Array[, {maxLeaf, isolateEmitters}]) -> Float32Array bvh_data: the same
 * tree built on the host, pt_bvh_build_lbvh */
static napi_value js_bvh_build_lbvh(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float* tri;
    size_t tl;
    if (argc < 1 || !get_f32(env, argv[0], &tri, &tl)) {
        napi_throw_type_error(env, NULL, "bvhBuildLbvh(Float32Array triangle_data, options?)");
        return NULL;
    }
    pt_build_params prm;
    if (!get_build_params(env, argc > 1 ? argv[1] : NULL, &prm)) return NULL;
    size_t len = 0;
    int rc = pt_bvh_build_lbvh(tri, tl, &prm, NULL, 0, &len);
    if (rc) return throw_pt(env, rc);
    napi_value buf, arr;
    void* data = NULL;
    CHECK_NAPI(env, napi_create_arraybuffer(env, len * sizeof(float), &data, &buf));
    rc = pt_bvh_build_lbvh(tri, tl, &prm, (float*)data, len, &len);
    if (rc) return throw_pt(env, rc);
    CHECK_NAPI(env, napi_create_typedarray(env, napi_float32_array, len, buf, 0, &arr));
    return arr;
}

/* sceneDestroy(scene): free the scene's device memory now (the handle becomes unusable); throws
 * while a render job on it runs */
static napi_value js_scene_destroy(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    scene_box* b = argc ? get_box(env, argv[0]) : NULL;
    if (!b) { napi_throw_type_error(env, NULL, "sceneDestroy(scene)"); return NULL; }
    if (b->busy) { napi_throw_error(env, NULL, "scene is busy: a render job on it has not completed"); return NULL; }
    if (b->s) {
        pt_scene_info si;
        int have = pt_scene_get_info(b->s, &si) == PT_OK;
        pt_scene_destroy(b->s);
        b->s = NULL;
        if (have) {
            int64_t adj = 0;
            napi_adjust_external_memory(env, -(int64_t)si.device_bytes, &adj);
        }
    }
    return NULL;
}

/* sceneInfo(scene) -> object */
static napi_value js_scene_info(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    pt_scene* s = argc ? get_scene(env, argv[0]) : NULL;
    if (!s) { if (!pending_exception(env)) napi_throw_type_error(env, NULL, "sceneInfo(scene)"); return NULL; }
    pt_scene_info si;
    int rc = pt_scene_get_info(s, &si);
    if (rc) return throw_pt(env, rc);
    napi_value o, v;
    napi_create_object(env, &o);
#define SET(name) napi_create_double(env, (double)si.name, &v); napi_set_named_property(env, o, #name, v);
    SET(nodes) SET(leaves) SET(leaf_refs) SET(max_leaf) SET(max_stack) SET(materials) SET(emissive_tris) SET(vertices)
    SET(device_bytes)
#undef SET
    return o;
}

typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref refs[3]; /* scene, meta, accum kept alive while the worker runs */
    scene_box* box;   /* busy while the job runs */
    pt_scene* scene;
    float meta[48];
    uint32_t frame0, nframes, stride;
    int32_t max_depth, mode;
    float* accum;
    uint8_t* rgba; /* renderImage: the displayed image instead of the accumulator */
    pt_window win; /* renderWindow: the rectangle of the image to render (has_win) */
    int has_win;
    pt_window* rects; /* renderRects: the list (malloc'd; win is then its frame), nrects > 0 */
    size_t nrects;
    pt_counters counters;
    int want_counters; /* optional last argument (default true): counting builds of the kernels */
    int rc;
    char err[512];
} render_job;

static void render_execute(napi_env env, void* data) {
    (void)env;
    render_job* j = (render_job*)data;
    pt_counters* c = j->want_counters ? &j->counters : NULL;
    j->rc = j->rgba ? pt_render_image(j->scene, j->meta, j->frame0, j->nframes, j->stride, j->max_depth, j->mode, j->rgba, c)
            : j->rects ? pt_render_rects(j->scene, j->meta, j->has_win ? &j->win : NULL, j->rects, j->nrects, j->frame0,
                                         j->nframes, j->stride, j->max_depth, j->mode, j->accum, NULL, c)
                    : pt_render_window(j->scene, j->meta, j->has_win ? &j->win : NULL, j->frame0, j->nframes, j->stride,
                                       j->max_depth, j->mode, j->accum, c);
    if (j->rc) snprintf(j->err, sizeof j->err, "pt_hip error %d: %s", j->rc, pt_last_error());
}

static void render_complete(napi_env env, napi_status status, void* data) {
    render_job* j = (render_job*)data;
    if (j->box) j->box->busy = 0;
    if (status == napi_ok && j->rc == 0) {
        napi_value none;
        napi_get_null(env, &none);
        napi_resolve_deferred(env, j->deferred, j->want_counters ? counters_obj(env, &j->counters) : none);
    } else {
        napi_value msg, e;
        napi_create_string_utf8(env, j->rc ? j->err : "render cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, NULL, msg, &e);
        napi_reject_deferred(env, j->deferred, e);
    }
    for (int i = 0; i < 3; ++i) napi_delete_reference(env, j->refs[i]);
    napi_delete_async_work(env, j->work);
    free(j->rects);
    free(j);
}

/* optional boolean argv[8]: work counters wanted (default true) */
static int parse_want_counters(napi_env env, size_t argc, napi_value* argv, render_job* j) {
    bool want = true;
    if (argc > 8) {
        napi_valuetype t;
        if (napi_typeof(env, argv[8], &t) != napi_ok) return 0;
        if (t != napi_undefined && napi_get_value_bool(env, argv[8], &want) != napi_ok) return 0;
    }
    j->want_counters = want ? 1 : 0;
    return 1;
}

/* [x0, y0, w, h]: four non-negative integers below 2^32 (the library checks them against the image) */
static int parse_window(napi_env env, napi_value v, pt_window* win) {
    bool is_arr = false;
    uint32_t n = 0;
    if (napi_is_array(env, v, &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, v, &n) != napi_ok || n != 4)
        return 0;
    uint32_t* out[4] = {&win->x0, &win->y0, &win->w, &win->h};
    for (uint32_t i = 0; i < 4; ++i) {
        napi_value e;
        double d;
        if (napi_get_element(env, v, i, &e) != napi_ok || napi_get_value_double(env, e, &d) != napi_ok) return 0;
        if (!(d >= 0.0 && d <= 4294967295.0) || d != (double)(uint32_t)d) return 0;
        *out[i] = (uint32_t)d;
    }
    return 1;
}

/* parse (scene, meta, frame0, nframes, stride, maxDepth, mode, accum[, counters]); with has_win set
 * the accumulator is the window's, w*h*3 */
static int parse_render_argv(napi_env env, size_t argc, napi_value argv[9], render_job* j) {
    if (argc < 8) return 0;
    if (!parse_want_counters(env, argc, argv, j)) return 0;
    float* meta;
    size_t ml, al;
    j->box = get_box(env, argv[0]);
    j->scene = get_scene(env, argv[0]);
    if (!j->scene || !get_f32(env, argv[1], &meta, &ml) || ml < 48) return 0;
    memcpy(j->meta, meta, sizeof j->meta);
    if (!get_u32(env, argv[2], &j->frame0) || !get_u32(env, argv[3], &j->nframes) || !get_u32(env, argv[4], &j->stride) ||
        !get_i32(env, argv[5], &j->max_depth) || !get_i32(env, argv[6], &j->mode) || !get_f32(env, argv[7], &j->accum, &al))
        return 0;
    if (al != (j->has_win ? (size_t)j->win.w * j->win.h : (size_t)j->meta[0] * (size_t)j->meta[1]) * 3) return 0;
    return 1;
}

static int parse_render_args(napi_env env, napi_callback_info info, render_job* j, napi_value argv[9]) {
    size_t argc = 9;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok) return 0;
    if (argc > 9) argc = 9; /* the call's own count: only argv[0..8] were filled */
    return parse_render_argv(env, argc, argv, j);
}

/* the same with the window after meta: (scene, meta, [x0, y0, w, h], frame0, ...); argv comes back
 * without it, in render()'s order */
static int parse_render_window_args(napi_env env, napi_callback_info info, render_job* j, napi_value argv[9]) {
    napi_value a[10];
    size_t argc = 10;
    if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 9) return 0;
    if (argc > 10) return 0; /* argc comes back as the call's own count, whatever a[] holds: too many is a TypeError */
    if (!parse_window(env, a[2], &j->win)) return 0;
    j->has_win = 1;
    argv[0] = a[0];
    argv[1] = a[1];
    for (size_t i = 3; i < argc; ++i) argv[i - 1] = a[i];
    return parse_render_argv(env, argc - 1, argv, j);
}

/* renderRects' (scene, meta, frame | null, [[x0, y0, w, h], ...], frame0, ...): the frame (null or
 * undefined: the whole image; the accumulator is the frame's, w*h*3) and a non-empty list of at most
 * 65536 rectangles; argv comes back without the two, in render()'s order.  The library checks the
 * list against the frame and for overlaps. */
#define PT_NODE_MAX_RECTS 65536u
static int parse_render_rects_args(napi_env env, napi_callback_info info, render_job* j, napi_value argv[9]) {
    napi_value a[11];
    size_t argc = 11;
    if (napi_get_cb_info(env, info, &argc, a, NULL, NULL) != napi_ok || argc < 10 || argc > 11) return 0;
    napi_valuetype t;
    if (napi_typeof(env, a[2], &t) != napi_ok) return 0;
    if (t != napi_null && t != napi_undefined) {
        if (!parse_window(env, a[2], &j->win)) return 0;
        j->has_win = 1;
    }
    bool is_arr = false;
    uint32_t n = 0;
    if (napi_is_array(env, a[3], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, a[3], &n) != napi_ok ||
        n < 1 || n > PT_NODE_MAX_RECTS)
        return 0;
    j->rects = (pt_window*)malloc((size_t)n * sizeof(pt_window));
    if (!j->rects) return 0;
    j->nrects = n;
    for (uint32_t k = 0; k < n; ++k) {
        napi_value e;
        if (napi_get_element(env, a[3], k, &e) != napi_ok || !parse_window(env, e, &j->rects[k])) return 0;
    }
    argv[0] = a[0];
    argv[1] = a[1];
    for (size_t i = 4; i < argc; ++i) argv[i - 2] = a[i];
    return parse_render_argv(env, argc - 2, argv, j);
}

/* render(scene, meta, frame0, nframes, stride, maxDepth, mode, accum[, counters=true]) -> Promise<counters|null>
 * renderWindow(scene, meta, [x0, y0, w, h], frame0, nframes, stride, maxDepth, mode, accum[w*h*3][, counters=true]):
 * the same for a rectangle of the image (pt_render_window)
 * renderRects(scene, meta, [x0, y0, w, h] | null, [[x0, y0, w, h], ...], frame0, nframes, stride, maxDepth, mode,
 * accum[frame w*h*3][, counters=true]): the rectangles of the list in one pass, in place inside the
 * frame's accumulator (pt_render_rects); window: 0 render, 1 renderWindow, 2 renderRects */
static napi_value render_start(napi_env env, napi_callback_info info, int window) {
    napi_value argv[9];
    render_job* j = (render_job*)calloc(1, sizeof(render_job));
    if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    if (!(window == 2   ? parse_render_rects_args(env, info, j, argv)
          : window == 1 ? parse_render_window_args(env, info, j, argv)
                        : parse_render_args(env, info, j, argv))) {
        free(j->rects);
        free(j);
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL,
                                  window == 2 ? "renderRects(scene, Float32Array meta[48], [x0, y0, w, h] | null, [[x0, y0, w, h], ...], "
                                                "frame0, nframes, stride, maxDepth, mode, Float32Array accum[frame w*h*3], counters?)"
                                  : window ? "renderWindow(scene, Float32Array meta[48], [x0, y0, w, h], frame0, nframes, stride, "
                                           "maxDepth, mode, Float32Array accum[w*h*3], counters?)"
                                         : "render(scene, Float32Array meta[48], frame0, nframes, stride, maxDepth, mode, "
                                           "Float32Array accum[W*H*3], counters?)");
        return NULL;
    }
    j->box->busy = 1;
    napi_value promise, name;
    CHECK_NAPI(env, napi_create_promise(env, &j->deferred, &promise));
    napi_create_reference(env, argv[0], 1, &j->refs[0]);
    napi_create_reference(env, argv[1], 1, &j->refs[1]);
    napi_create_reference(env, argv[7], 1, &j->refs[2]);
    napi_create_string_utf8(env, "pt_render", NAPI_AUTO_LENGTH, &name);
    CHECK_NAPI(env, napi_create_async_work(env, NULL, name, render_execute, render_complete, j, &j->work));
    CHECK_NAPI(env, napi_queue_async_work(env, j->work));
    return promise;
}

static napi_value js_render(napi_env env, napi_callback_info info) { return render_start(env, info, 0); }
static napi_value js_render_window(napi_env env, napi_callback_info info) { return render_start(env, info, 1); }
static napi_value js_render_rects(napi_env env, napi_callback_info info) { return render_start(env, info, 2); }

/* renderMulti([scene, ...], meta, frame0, nframes, stride, maxDepth, mode, accum[, counters=true])
 * -> Promise<counters|null>: one image over one scene per device (pt_render_multi: frames dealt
 * round-robin, partial accumulators reduced onto the first scene's device) */
#define PT_NODE_MAX_DEVICES 64
typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref refs[3]; /* scene array, meta, accum */
    scene_box* boxes[PT_NODE_MAX_DEVICES];
    pt_scene* scenes[PT_NODE_MAX_DEVICES];
    int n;
    float meta[48];
    uint32_t frame0, nframes, stride;
    int32_t max_depth, mode;
    float* accum;
    pt_counters counters;
    int want_counters;
    int rc;
    char err[512];
} multi_job;

static void multi_execute(napi_env env, void* data) {
    (void)env;
    multi_job* j = (multi_job*)data;
    j->rc = pt_render_multi(j->scenes, j->n, j->meta, j->frame0, j->nframes, j->stride, j->max_depth, j->mode, j->accum,
                            j->want_counters ? &j->counters : NULL);
    if (j->rc) snprintf(j->err, sizeof j->err, "pt_hip error %d: %s", j->rc, pt_last_error());
}

static void multi_complete(napi_env env, napi_status status, void* data) {
    multi_job* j = (multi_job*)data;
    for (int i = 0; i < j->n; ++i) j->boxes[i]->busy = 0;
    if (status == napi_ok && j->rc == 0) {
        napi_value none;
        napi_get_null(env, &none);
        napi_resolve_deferred(env, j->deferred, j->want_counters ? counters_obj(env, &j->counters) : none);
    } else {
        napi_value msg, e;
        napi_create_string_utf8(env, j->rc ? j->err : "render cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, NULL, msg, &e);
        napi_reject_deferred(env, j->deferred, e);
    }
    for (int i = 0; i < 3; ++i) napi_delete_reference(env, j->refs[i]);
    napi_delete_async_work(env, j->work);
    free(j);
}

static napi_value js_render_multi(napi_env env, napi_callback_info info) {
    size_t argc = 9;
    napi_value argv[9];
    multi_job* j = (multi_job*)calloc(1, sizeof(multi_job));
    if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    int ok = napi_get_cb_info(env, info, &argc, argv, NULL, NULL) == napi_ok && argc >= 8;
    bool is_arr = false;
    uint32_t n = 0;
    if (ok) ok = napi_is_array(env, argv[0], &is_arr) == napi_ok && is_arr &&
                 napi_get_array_length(env, argv[0], &n) == napi_ok && n >= 1 && n <= PT_NODE_MAX_DEVICES;
    for (uint32_t i = 0; ok && i < n; ++i) {
        napi_value e;
        ok = napi_get_element(env, argv[0], i, &e) == napi_ok && (j->boxes[i] = get_box(env, e)) != NULL &&
             (j->scenes[i] = get_scene(env, e)) != NULL;
        for (uint32_t k = 0; ok && k < i; ++k) ok = j->boxes[k] != j->boxes[i];
    }
    j->n = (int)n;
    float* meta = NULL;
    size_t ml = 0, al = 0;
    if (ok) {
        bool want = true;
        if (argc > 8) {
            napi_valuetype t;
            ok = napi_typeof(env, argv[8], &t) == napi_ok && (t == napi_undefined || napi_get_value_bool(env, argv[8], &want) == napi_ok);
        }
        j->want_counters = want ? 1 : 0;
    }
    if (ok) ok = get_f32(env, argv[1], &meta, &ml) && ml >= 48;
    if (ok) {
        memcpy(j->meta, meta, sizeof j->meta);
        ok = get_u32(env, argv[2], &j->frame0) && get_u32(env, argv[3], &j->nframes) && get_u32(env, argv[4], &j->stride) &&
             get_i32(env, argv[5], &j->max_depth) && get_i32(env, argv[6], &j->mode) && get_f32(env, argv[7], &j->accum, &al) &&
             al == (size_t)j->meta[0] * (size_t)j->meta[1] * 3;
    }
    if (!ok) {
        free(j);
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL,
                                  "renderMulti([scene, ...] (distinct handles, <= 64), Float32Array meta[48], frame0, "
                                  "nframes, stride, maxDepth, mode, Float32Array accum[W*H*3], counters?)");
        return NULL;
    }
    for (int i = 0; i < j->n; ++i) j->boxes[i]->busy = 1;
    napi_value promise, name;
    CHECK_NAPI(env, napi_create_promise(env, &j->deferred, &promise));
    napi_create_reference(env, argv[0], 1, &j->refs[0]);
    napi_create_reference(env, argv[1], 1, &j->refs[1]);
    napi_create_reference(env, argv[7], 1, &j->refs[2]);
    napi_create_string_utf8(env, "pt_render_multi", NAPI_AUTO_LENGTH, &name);
    CHECK_NAPI(env, napi_create_async_work(env, NULL, name, multi_execute, multi_complete, j, &j->work));
    CHECK_NAPI(env, napi_queue_async_work(env, j->work));
    return promise;
}

/* renderImage(scene, meta, frame0, nframes, stride, maxDepth, mode, Uint8Array rgba[W*H*4][, counters=true])
 * -> Promise<counters|null>:
 * programEntry's displayed image, tone-mapped on the device (pt_render_image) */
static napi_value js_render_image(napi_env env, napi_callback_info info) {
    size_t argc = 9;
    napi_value argv[9];
    render_job* j = (render_job*)calloc(1, sizeof(render_job));
    if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    float* meta;
    size_t ml = 0, il = 0;
    int ok = napi_get_cb_info(env, info, &argc, argv, NULL, NULL) == napi_ok && argc >= 8 &&
             parse_want_counters(env, argc, argv, j);
    if (ok) {
        j->box = get_box(env, argv[0]);
        j->scene = get_scene(env, argv[0]);
        ok = j->scene && get_f32(env, argv[1], &meta, &ml) && ml >= 48;
    }
    if (ok) {
        memcpy(j->meta, meta, sizeof j->meta);
        ok = get_u32(env, argv[2], &j->frame0) && get_u32(env, argv[3], &j->nframes) && get_u32(env, argv[4], &j->stride) &&
             get_i32(env, argv[5], &j->max_depth) && get_i32(env, argv[6], &j->mode) && get_u8(env, argv[7], &j->rgba, &il) &&
             il == (size_t)j->meta[0] * (size_t)j->meta[1] * 4;
    }
    if (!ok) {
        free(j);
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL,
                                  "renderImage(scene, Float32Array meta[48], frame0, nframes, stride, maxDepth, mode, "
                                  "Uint8Array rgba[W*H*4])");
        return NULL;
    }
    j->box->busy = 1;
    napi_value promise, name;
    CHECK_NAPI(env, napi_create_promise(env, &j->deferred, &promise));
    napi_create_reference(env, argv[0], 1, &j->refs[0]);
    napi_create_reference(env, argv[1], 1, &j->refs[1]);
    napi_create_reference(env, argv[7], 1, &j->refs[2]);
    napi_create_string_utf8(env, "pt_render_image", NAPI_AUTO_LENGTH, &name);
    CHECK_NAPI(env, napi_create_async_work(env, NULL, name, render_execute, render_complete, j, &j->work));
    CHECK_NAPI(env, napi_queue_async_work(env, j->work));
    return promise;
}

/* renderSync(...same...) -> counters */
static napi_value js_render_sync(napi_env env, napi_callback_info info) {
    napi_value argv[9];
    render_job j;
    memset(&j, 0, sizeof j);
    if (!parse_render_args(env, info, &j, argv)) {
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL, "renderSync(scene, meta, frame0, nframes, stride, maxDepth, mode, accum)");
        return NULL;
    }
    int rc = pt_render(j.scene, j.meta, j.frame0, j.nframes, j.stride, j.max_depth, j.mode, j.accum,
                       j.want_counters ? &j.counters : NULL);
    if (rc) return throw_pt(env, rc);
    napi_value none;
    napi_get_null(env, &none);
    return j.want_counters ? counters_obj(env, &j.counters) : none;
}

/* frame(scene, meta, t, maxDepth, out Float32Array[W*H*3]) */
static napi_value js_frame(napi_env env, napi_callback_info info) {
    size_t argc = 5;
    napi_value argv[5];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float *meta, *out;
    size_t ml, ol;
    uint32_t t;
    int32_t md;
    pt_scene* s = argc >= 5 ? get_scene(env, argv[0]) : NULL;
    if (!s || !get_f32(env, argv[1], &meta, &ml) || ml < 48 || !get_u32(env, argv[2], &t) || !get_i32(env, argv[3], &md) ||
        !get_f32(env, argv[4], &out, &ol) || ol != (size_t)meta[0] * (size_t)meta[1] * 3) {
        if (!pending_exception(env)) napi_throw_type_error(env, NULL, "frame(scene, meta, t, maxDepth, Float32Array out[W*H*3])");
        return NULL;
    }
    int rc = pt_frame(s, meta, t, md, out);
    if (rc) return throw_pt(env, rc);
    return NULL;
}

/* renderDenoised(scene, meta, frame0, nframes, stride, maxDepth, mode, featureFrames, iters, Uint8Array rgba[W*H*4]):
 * pt_render_denoised_image — a moments render, the guide buffers, the a-trous filter and the device tone
 * map in one blocking call; iters 0 = pt_denoise_defaults, else the defaults with that many passes */
static napi_value js_render_denoised(napi_env env, napi_callback_info info) {
    size_t argc = 10;
    napi_value argv[10];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float* meta;
    uint8_t* out;
    size_t ml, ol;
    uint32_t frame0, nframes, stride, ff, iters;
    int32_t md, mode;
    pt_scene* s = argc >= 10 ? get_scene(env, argv[0]) : NULL;
    if (!s || !get_f32(env, argv[1], &meta, &ml) || ml < 48 || !get_u32(env, argv[2], &frame0) ||
        !get_u32(env, argv[3], &nframes) || !get_u32(env, argv[4], &stride) || !get_i32(env, argv[5], &md) ||
        !get_i32(env, argv[6], &mode) || !get_u32(env, argv[7], &ff) || !get_u32(env, argv[8], &iters) ||
        !get_u8(env, argv[9], &out, &ol) || ol != (size_t)meta[0] * (size_t)meta[1] * 4) {
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL,
                                  "renderDenoised(scene, Float32Array meta[48], frame0, nframes, stride, maxDepth, mode, "
                                  "featureFrames, iters, Uint8Array rgba[W*H*4])");
        return NULL;
    }
    pt_denoise_params p;
    pt_denoise_defaults(&p);
    if (iters) p.iters = iters;
    int rc = pt_render_denoised_image(s, meta, frame0, nframes, stride, md, mode, ff, &p, out, NULL);
    if (rc) return throw_pt(env, rc);
    return NULL;
}

/* a new typed array of n elements (Float32Array, Uint32Array or Uint8Array) and its storage */
static napi_value new_typedarray(napi_env env, napi_typedarray_type type, size_t n, void** data) {
    napi_value ab, ta;
    const size_t bytes = n * (type == napi_uint8_array ? 1 : 4);
    if (napi_create_arraybuffer(env, bytes, data, &ab) != napi_ok || napi_create_typedarray(env, type, n, ab, 0, &ta) != napi_ok) {
        if (!pending_exception(env)) napi_throw_error(env, NULL, "could not allocate the result array");
        return NULL;
    }
    return ta;
}

/* Temporal accumulation (include/pt_hip.h pt_reproject, pt_denoise_mean, pt_history_*): blocking calls, as
 * renderDenoised.  params: null (pt_temporal_defaults) or a Float32Array [alpha, normal_min, depth_tol, max_history] */
static int get_temporal(napi_env env, napi_value v, pt_temporal_params* p, const pt_temporal_params** out) {
    napi_valuetype t = napi_undefined;
    *out = NULL;
    if (napi_typeof(env, v, &t) != napi_ok) return 0;
    if (t == napi_null || t == napi_undefined) return 1;
    float* f;
    size_t n;
    if (!get_f32(env, v, &f, &n) || n != 4) return 0;
    p->alpha = f[0]; p->normal_min = f[1]; p->depth_tol = f[2]; p->max_history = f[3];
    *out = p;
    return 1;
}

static int is_nullish(napi_env env, napi_value v) {
    napi_valuetype t = napi_undefined;
    return napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined);
}

/* reproject(scene, accum[W*H*3], m2[W*H*3], n, geo[W*H*4], alb[W*H*4], meta[48], prevMeta | null, prevHist | null,
 *           prevMom | null, prevGbuf | null, params | null) -> {hist, mom, gbuf, out, var}: pt_reproject */
static napi_value js_reproject(napi_env env, napi_callback_info info) {
    size_t argc = 12;
    napi_value argv[12];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float *acc, *m2, *geo, *alb, *meta, *prev[4] = {NULL, NULL, NULL, NULL};
    size_t al, sl, gl, bl, ml, pl;
    uint32_t n;
    pt_temporal_params prm;
    const pt_temporal_params* pp = NULL;
    pt_scene* s = argc >= 12 ? get_scene(env, argv[0]) : NULL;
    int ok = s && get_f32(env, argv[1], &acc, &al) && get_f32(env, argv[2], &m2, &sl) && get_u32(env, argv[3], &n) &&
             get_f32(env, argv[4], &geo, &gl) && get_f32(env, argv[5], &alb, &bl) && get_f32(env, argv[6], &meta, &ml) &&
             ml >= 48 && get_temporal(env, argv[11], &prm, &pp);
    size_t npix = 0;
    if (ok) {
        npix = (size_t)meta[0] * (size_t)meta[1];
        ok = npix > 0 && al == 3 * npix && sl == 3 * npix && gl == 4 * npix && bl == 4 * npix;
    }
    for (int k = 0; ok && k < 4; ++k)
        if (!is_nullish(env, argv[7 + k])) ok = get_f32(env, argv[7 + k], &prev[k], &pl) && pl == (k ? 4 * npix : 48);
    if (!ok) {
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL,
                                  "reproject(scene, Float32Array accum[W*H*3], m2[W*H*3], n, geo[W*H*4], alb[W*H*4], meta[48], "
                                  "prevMeta[48] | null, prevHist[W*H*4] | null, prevMom | null, prevGbuf | null, "
                                  "Float32Array params[4] | null)");
        return NULL;
    }
    float *hist, *mom, *gbuf, *out, *var;
    napi_value o, vh = new_typedarray(env, napi_float32_array, 4 * npix, (void**)&hist),
                  vm = new_typedarray(env, napi_float32_array, 4 * npix, (void**)&mom),
                  vg = new_typedarray(env, napi_float32_array, 4 * npix, (void**)&gbuf),
                  vo = new_typedarray(env, napi_float32_array, 3 * npix, (void**)&out),
                  vv = new_typedarray(env, napi_float32_array, npix, (void**)&var);
    if (!vh || !vm || !vg || !vo || !vv) return NULL;
    int rc = pt_reproject(s, acc, m2, n, geo, alb, meta, prev[0], prev[1], prev[2], prev[3], (uint32_t)meta[0], (uint32_t)meta[1],
                          pp, hist, mom, gbuf, out, var);
    if (rc) return throw_pt(env, rc);
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_set_named_property(env, o, "hist", vh);
    napi_set_named_property(env, o, "mom", vm);
    napi_set_named_property(env, o, "gbuf", vg);
    napi_set_named_property(env, o, "out", vo);
    napi_set_named_property(env, o, "var", vv);
    return o;
}

/* denoiseMean(scene, c[w*h*3], var[w*h], w, h, geo[w*h*4], alb[w*h*4], featureFrames, iters) -> {out, var}:
 * pt_denoise_mean; iters 0 = pt_denoise_defaults, else the defaults with that many passes */
static napi_value js_denoise_mean(napi_env env, napi_callback_info info) {
    size_t argc = 9;
    napi_value argv[9];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float *c, *var, *geo, *alb;
    size_t cl, vl, gl, bl;
    uint32_t w, h, ff, iters;
    pt_scene* s = argc >= 9 ? get_scene(env, argv[0]) : NULL;
    if (!s || !get_f32(env, argv[1], &c, &cl) || !get_f32(env, argv[2], &var, &vl) || !get_u32(env, argv[3], &w) ||
        !get_u32(env, argv[4], &h) || !get_f32(env, argv[5], &geo, &gl) || !get_f32(env, argv[6], &alb, &bl) ||
        !get_u32(env, argv[7], &ff) || !get_u32(env, argv[8], &iters) || !w || !h || vl != (size_t)w * h || cl != 3 * vl ||
        gl != 4 * vl || bl != 4 * vl) {
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL,
                                  "denoiseMean(scene, Float32Array c[w*h*3], var[w*h], w, h, geo[w*h*4], alb[w*h*4], featureFrames, "
                                  "iters)");
        return NULL;
    }
    pt_denoise_params p;
    pt_denoise_defaults(&p);
    if (iters) p.iters = iters;
    float *out, *vout;
    napi_value o, vo = new_typedarray(env, napi_float32_array, cl, (void**)&out),
                  vv = new_typedarray(env, napi_float32_array, vl, (void**)&vout);
    if (!vo || !vv) return NULL;
    int rc = pt_denoise_mean(s, c, var, w, h, geo, alb, ff, &p, out, vout);
    if (rc) return throw_pt(env, rc);
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_set_named_property(env, o, "out", vo);
    napi_set_named_property(env, o, "var", vv);
    return o;
}

/* A JS history handle: the library's history, its size, and a reference that keeps its scene's handle alive (the
 * scene's job guard covers the history's calls: they run on the scene's stream) */
typedef struct {
    pt_history* h;
    uint32_t w, ht;
    napi_ref scene;
} history_box;

static void history_release(napi_env env, history_box* b) {
    if (b->h) {
        pt_history_destroy(b->h);
        b->h = NULL;
        int64_t adj = 0;
        napi_adjust_external_memory(env, -(int64_t)((size_t)b->w * b->ht * 188), &adj);
    }
    if (b->scene) { napi_delete_reference(env, b->scene); b->scene = NULL; }
}

static void history_finalize(napi_env env, void* data, void* hint) {
    (void)hint;
    history_release(env, (history_box*)data);
    free(data);
}

/* the live history of a handle whose scene is neither destroyed nor busy: NULL (and a pending JS error) otherwise */
static history_box* get_history(napi_env env, napi_value v) {
    void* p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) return NULL;
    history_box* b = (history_box*)p;
    if (!b->h) { napi_throw_error(env, NULL, "history was destroyed (historyDestroy)"); return NULL; }
    napi_value sv;
    if (napi_get_reference_value(env, b->scene, &sv) != napi_ok || !sv) return NULL;
    scene_box* sb = get_box(env, sv);
    if (sb && !sb->s) { napi_throw_error(env, NULL, "scene was destroyed (sceneDestroy): the history is unusable"); return NULL; }
    if (sb && sb->busy) { napi_throw_error(env, NULL, "scene is busy: a render job on it has not completed"); return NULL; }
    return b;
}

/* historyCreate(scene, w, h) -> external */
static napi_value js_history_create(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    uint32_t w, h;
    pt_scene* s = argc >= 3 ? get_scene(env, argv[0]) : NULL;
    if (!s || !get_u32(env, argv[1], &w) || !get_u32(env, argv[2], &h)) {
        if (!pending_exception(env)) napi_throw_type_error(env, NULL, "historyCreate(scene, w, h)");
        return NULL;
    }
    history_box* b = (history_box*)calloc(1, sizeof(history_box));
    if (!b) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    int rc = pt_history_create(s, w, h, &b->h);
    if (rc) { free(b); return throw_pt(env, rc); }
    b->w = w; b->ht = h;
    napi_value ext;
    if (napi_create_reference(env, argv[0], 1, &b->scene) != napi_ok ||
        napi_create_external(env, b, history_finalize, NULL, &ext) != napi_ok) {
        history_release(env, b);
        free(b);
        napi_throw_error(env, NULL, "napi_create_external failed");
        return NULL;
    }
    int64_t adj = 0;
    napi_adjust_external_memory(env, (int64_t)((size_t)w * h * 188), &adj);  /* 6 planes, 22 floats, 4 bytes per pixel */
    return ext;
}

/* historyReset(history): the next step is a first step */
static napi_value js_history_reset(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    history_box* b = argc ? get_history(env, argv[0]) : NULL;
    if (!b) {
        if (!pending_exception(env)) napi_throw_type_error(env, NULL, "historyReset(history)");
        return NULL;
    }
    int rc = pt_history_reset(b->h);
    if (rc) return throw_pt(env, rc);
    return NULL;
}

/* historyDestroy(history): free its device memory now (the handle becomes unusable) */
static napi_value js_history_destroy(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    void* p = NULL;
    if (!argc || napi_get_value_external(env, argv[0], &p) != napi_ok || !p) {
        napi_throw_type_error(env, NULL, "historyDestroy(history)");
        return NULL;
    }
    history_box* b = (history_box*)p;
    /* a history whose scene is gone has lost its buffers already: only the handle is released */
    if (b->h) {
        napi_value sv;
        scene_box* sb = napi_get_reference_value(env, b->scene, &sv) == napi_ok && sv ? get_box(env, sv) : NULL;
        if (sb && sb->busy) { napi_throw_error(env, NULL, "scene is busy: a render job on it has not completed"); return NULL; }
    }
    history_release(env, b);
    return NULL;
}

/* historyStep(history, meta[48], frame0, nframes, stride, maxDepth, mode, featureFrames, params | null, denoiseIters)
 * -> {mean[w*h*3], var[w*h], rgba[w*h*4], historyLen[w*h]}: pt_history_step; denoiseIters -1 = unfiltered,
 * 0 = pt_denoise_defaults, else the defaults with that many passes */
static napi_value js_history_step(napi_env env, napi_callback_info info) {
    size_t argc = 10;
    napi_value argv[10];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float* meta;
    size_t ml;
    uint32_t frame0, nframes, stride, ff;
    int32_t md, mode, iters;
    pt_temporal_params prm;
    const pt_temporal_params* pp = NULL;
    history_box* b = argc >= 10 ? get_history(env, argv[0]) : NULL;
    if (!b || !get_f32(env, argv[1], &meta, &ml) || ml < 48 || !get_u32(env, argv[2], &frame0) ||
        !get_u32(env, argv[3], &nframes) || !get_u32(env, argv[4], &stride) || !get_i32(env, argv[5], &md) ||
        !get_i32(env, argv[6], &mode) || !get_u32(env, argv[7], &ff) || !get_temporal(env, argv[8], &prm, &pp) ||
        !get_i32(env, argv[9], &iters) || iters < -1) {
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL,
                                  "historyStep(history, Float32Array meta[48], frame0, nframes, stride, maxDepth, mode, "
                                  "featureFrames, Float32Array params[4] | null, denoiseIters)");
        return NULL;
    }
    pt_denoise_params dp;
    pt_denoise_defaults(&dp);
    if (iters > 0) dp.iters = (uint32_t)iters;
    const size_t npix = (size_t)b->w * b->ht;
    float *mean, *var, *len;
    uint8_t* rgba;
    napi_value o, vm = new_typedarray(env, napi_float32_array, 3 * npix, (void**)&mean),
                  vv = new_typedarray(env, napi_float32_array, npix, (void**)&var),
                  vr = new_typedarray(env, napi_uint8_array, 4 * npix, (void**)&rgba),
                  vl = new_typedarray(env, napi_float32_array, npix, (void**)&len);
    if (!vm || !vv || !vr || !vl) return NULL;
    int rc = pt_history_step(b->h, meta, frame0, nframes, stride, md, mode, ff, pp, iters >= 0 ? &dp : NULL, mean, var, rgba, len,
                             NULL);
    if (rc) return throw_pt(env, rc);
    CHECK_NAPI(env, napi_create_object(env, &o));
    napi_set_named_property(env, o, "mean", vm);
    napi_set_named_property(env, o, "var", vv);
    napi_set_named_property(env, o, "rgba", vr);
    napi_set_named_property(env, o, "historyLen", vl);
    return o;
}

/* queryHits(scene, Float32Array rays[8n]) -> Float32Array[8n]: pt_query_hits — per ray (o.xyz, tmax, d.xyz,
 * reserved) the closest hit's (p.xyz, t, n.xyz, material as int32 bits; a miss: t = -1, material = -1).
 * queryOccluded(scene, rays) -> Uint8Array[n]: pt_query_occluded.  Blocking. */
static napi_value query_call(napi_env env, napi_callback_info info, int occluded) {
    size_t argc = 2;
    napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float* rays;
    size_t rl;
    pt_scene* s = argc >= 2 ? get_scene(env, argv[0]) : NULL;
    if (!s || !get_f32(env, argv[1], &rays, &rl) || rl % 8 != 0) {
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL, occluded ? "queryOccluded(scene, Float32Array rays[8n])"
                                                      : "queryHits(scene, Float32Array rays[8n])");
        return NULL;
    }
    const size_t n = rl / 8;
    void* out = NULL;
    napi_value res = new_typedarray(env, occluded ? napi_uint8_array : napi_float32_array, occluded ? n : 8 * n, &out);
    if (!res) return NULL;
    const int rc = occluded ? pt_query_occluded(s, (const pt_ray*)rays, n, (uint8_t*)out, NULL)
                            : pt_query_hits(s, (const pt_ray*)rays, n, (pt_hit*)out, NULL);
    if (rc) return throw_pt(env, rc);
    return res;
}
static napi_value js_query_hits(napi_env env, napi_callback_info info) { return query_call(env, info, 0); }
static napi_value js_query_occluded(napi_env env, napi_callback_info info) { return query_call(env, info, 1); }

/* queryRadiance(scene, Float32Array rays[8n], Uint32Array seeds[n], nsamples, maxDepth, rr, directOnly[,
 * Float32Array accum[3n]]) -> Float32Array[3n]: pt_query_radiance — per ray the clamped radiance of nsamples
 * full paths, summed (into a copy of accum when given).  Blocking. */
static napi_value js_query_radiance(napi_env env, napi_callback_info info) {
    size_t argc = 8;
    napi_value argv[8];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float *rays, *acc = NULL;
    size_t rl, sl = 0, al = 0;
    uint32_t* seeds = NULL;
    pt_radiance_params prm;
    double rr = 0.0;
    bool direct = false;
    pt_scene* s = argc >= 7 ? get_scene(env, argv[0]) : NULL;
    int ok = s && get_f32(env, argv[1], &rays, &rl) && rl % 8 == 0;
    if (ok) {
        bool is_ta = false;
        napi_typedarray_type t;
        void* p;
        napi_value ab;
        size_t off;
        ok = napi_is_typedarray(env, argv[2], &is_ta) == napi_ok && is_ta &&
             napi_get_typedarray_info(env, argv[2], &t, &sl, &p, &ab, &off) == napi_ok && t == napi_uint32_array && sl == rl / 8;
        seeds = (uint32_t*)p;
    }
    ok = ok && get_u32(env, argv[3], &prm.nsamples) && get_i32(env, argv[4], &prm.max_depth) &&
         napi_get_value_double(env, argv[5], &rr) == napi_ok && napi_get_value_bool(env, argv[6], &direct) == napi_ok;
    if (ok && argc >= 8) {
        napi_valuetype vt;
        if (napi_typeof(env, argv[7], &vt) != napi_ok) ok = 0;
        else if (vt != napi_undefined && vt != napi_null) ok = get_f32(env, argv[7], &acc, &al) && al == rl / 8 * 3;
    }
    if (!ok) {
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL, "queryRadiance(scene, Float32Array rays[8n], Uint32Array seeds[n], nsamples, maxDepth, "
                                             "rr, directOnly[, Float32Array accum[3n]])");
        return NULL;
    }
    prm.rr_prob = (float)rr;
    prm.direct_only = direct ? 1 : 0;
    const size_t n = rl / 8;
    void* out = NULL;
    napi_value res = new_typedarray(env, napi_float32_array, 3 * n, &out);
    if (!res) return NULL;
    if (acc) memcpy(out, acc, 3 * n * sizeof(float));  /* a new ArrayBuffer is zeroed */
    const int rc = pt_query_radiance(s, (const pt_ray*)rays, seeds, n, &prm, (float*)out, NULL);
    if (rc) return throw_pt(env, rc);
    return res;
}

/* gather(scene, Float32Array points[8n], nsamples, sample0, mode, maxDepth, rr, directOnly[, Float32Array
 * accum[3n | 27n]]) -> Float32Array[3n | 27n]: pt_gather — points are pt_gather_point records (p.xyz, seed as
 * uint32 bits, n.xyz, 0); mode 0 = cosine (3 sums per point), 1 = SH9 (27).  Blocking.
 * gatherRays(scene, points, sample, mode) -> { rays: Float32Array[8n], seeds: Uint32Array[n] }: pt_gather_rays. */
static napi_value js_gather(napi_env env, napi_callback_info info) {
    size_t argc = 9;
    napi_value argv[9];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float *pts, *acc = NULL;
    size_t pl, al = 0;
    pt_gather_params prm;
    double rr = 0.0;
    bool direct = false;
    pt_scene* s = argc >= 8 ? get_scene(env, argv[0]) : NULL;
    int ok = s && get_f32(env, argv[1], &pts, &pl) && pl % 8 == 0;
    ok = ok && get_u32(env, argv[2], &prm.nsamples) && get_u32(env, argv[3], &prm.sample0) && get_u32(env, argv[4], &prm.mode) &&
         prm.mode <= PT_GATHER_SH9 && get_i32(env, argv[5], &prm.max_depth) && napi_get_value_double(env, argv[6], &rr) == napi_ok &&
         napi_get_value_bool(env, argv[7], &direct) == napi_ok;
    const size_t n = ok ? pl / 8 : 0, w = ok && prm.mode == PT_GATHER_SH9 ? 27 : 3;
    if (ok && argc >= 9) {
        napi_valuetype vt;
        if (napi_typeof(env, argv[8], &vt) != napi_ok) ok = 0;
        else if (vt != napi_undefined && vt != napi_null) ok = get_f32(env, argv[8], &acc, &al) && al == w * n;
    }
    if (!ok) {
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL, "gather(scene, Float32Array points[8n], nsamples, sample0, mode (0 | 1), maxDepth, rr, "
                                             "directOnly[, Float32Array accum[3n | 27n]])");
        return NULL;
    }
    prm.rr_prob = (float)rr;
    prm.direct_only = direct ? 1 : 0;
    void* out = NULL;
    napi_value res = new_typedarray(env, napi_float32_array, w * n, &out);
    if (!res) return NULL;
    if (acc) memcpy(out, acc, w * n * sizeof(float));  /* a new ArrayBuffer is zeroed */
    const int rc = pt_gather(s, (const pt_gather_point*)pts, n, &prm, (float*)out, NULL);
    if (rc) return throw_pt(env, rc);
    return res;
}

static napi_value js_gather_rays(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float* pts;
    size_t pl;
    uint32_t sample, mode;
    pt_scene* s = argc >= 4 ? get_scene(env, argv[0]) : NULL;
    if (!s || !get_f32(env, argv[1], &pts, &pl) || pl % 8 != 0 || !get_u32(env, argv[2], &sample) || !get_u32(env, argv[3], &mode)) {
        if (!pending_exception(env)) napi_throw_type_error(env, NULL, "gatherRays(scene, Float32Array points[8n], sample, mode (0 | 1))");
        return NULL;
    }
    const size_t n = pl / 8;
    void *rays = NULL, *seeds = NULL;
    napi_value jr = new_typedarray(env, napi_float32_array, 8 * n, &rays);
    if (!jr) return NULL;
    napi_value js = new_typedarray(env, napi_uint32_array, n, &seeds);
    if (!js) return NULL;
    const int rc = pt_gather_rays(s, (const pt_gather_point*)pts, n, mode, sample, (pt_ray*)rays, (uint32_t*)seeds);
    if (rc) return throw_pt(env, rc);
    napi_value res;
    CHECK_NAPI(env, napi_create_object(env, &res));
    CHECK_NAPI(env, napi_set_named_property(env, res, "rays", jr));
    CHECK_NAPI(env, napi_set_named_property(env, res, "seeds", js));
    return res;
}

/* cameraRays(scene, meta, frame[, [x0, y0, w, h]]) -> Float32Array[8 w h]: pt_camera_rays, the rays the render
 * traces for the window's pixels in that frame, row-major, tmax = +inf.
 * cameraSeeds(same arguments) -> Uint32Array[w h]: pt_camera_seeds, the seeds it hands to radiance() there. */
static napi_value camera_call(napi_env env, napi_callback_info info, int seeds) {
    size_t argc = 4;
    napi_value argv[4];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float* meta;
    size_t ml;
    uint32_t frame;
    pt_window win;
    int has_win = 0;
    pt_scene* s = argc >= 3 ? get_scene(env, argv[0]) : NULL;
    int ok = s && get_f32(env, argv[1], &meta, &ml) && ml >= 48 && get_u32(env, argv[2], &frame);
    if (ok && argc >= 4) {
        napi_valuetype vt;
        if (napi_typeof(env, argv[3], &vt) != napi_ok) ok = 0;
        else if (vt != napi_undefined && vt != napi_null) ok = has_win = parse_window(env, argv[3], &win);
    }
    if (!ok) {
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL, seeds ? "cameraSeeds(scene, Float32Array meta[48], frame[, [x0, y0, w, h]])"
                                                   : "cameraRays(scene, Float32Array meta[48], frame[, [x0, y0, w, h]])");
        return NULL;
    }
    /* the result's size is the window's, so the window is checked against the image (the library's own
     * rule, pt_window) before anything is allocated for it */
    const double W = (double)meta[0], H = (double)meta[1];
    if (!(W >= 1.0 && H >= 1.0 && W <= 32768.0 && H <= 32768.0)) {
        napi_throw_range_error(env, NULL, "cameraRays: meta[0..1] must be resolutions in [1, 32768]");
        return NULL;
    }
    if (has_win && (win.w < 1 || win.h < 1 || (double)win.x0 + (double)win.w > W || (double)win.y0 + (double)win.h > H)) {
        napi_throw_range_error(env, NULL, "cameraRays: the window must have w, h >= 1 and lie within the image (meta[0..1])");
        return NULL;
    }
    const double npix = has_win ? (double)win.w * (double)win.h : W * H;
    void* out = NULL;
    napi_value res = seeds ? new_typedarray(env, napi_uint32_array, (size_t)npix, &out)
                           : new_typedarray(env, napi_float32_array, 8 * (size_t)npix, &out);
    if (!res) return NULL;
    const int rc = seeds ? pt_camera_seeds(s, meta, has_win ? &win : NULL, frame, (uint32_t*)out)
                         : pt_camera_rays(s, meta, has_win ? &win : NULL, frame, (pt_ray*)out);
    if (rc) return throw_pt(env, rc);
    return res;
}
static napi_value js_camera_rays(napi_env env, napi_callback_info info) { return camera_call(env, info, 0); }
static napi_value js_camera_seeds(napi_env env, napi_callback_info info) { return camera_call(env, info, 1); }

/* tonemap(accum Float32Array, sampleRuns, out Uint8Array[npix*4]) */
static napi_value js_tonemap(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    float* acc;
    uint8_t* out;
    size_t al, ol;
    uint32_t runs;
    if (argc < 3 || !get_f32(env, argv[0], &acc, &al) || !get_u32(env, argv[1], &runs) || !get_u8(env, argv[2], &out, &ol) ||
        ol != al / 3 * 4) {
        napi_throw_type_error(env, NULL, "tonemap(Float32Array accum, sampleRuns, Uint8Array out)");
        return NULL;
    }
    int rc = pt_tonemap(acc, al / 3, runs, out);
    if (rc) return throw_pt(env, rc);
    return NULL;
}

/* bvhBuild(Float64Array vertices, Int32Array tris (i0,i1,i2,mat)[, sah=false[, Uint8Array isolate]])
 * -> Float32Array bvh_data (native twin of node/lib/bvh.js + packer.js:pack_bvh, byte-identical; sah:
 * the fast binned-SAH mode, pt_bvh_build_sah, same layout, not the reference's tree; isolate: per
 * material a flag — the emitters — whose triangles go under the root's left child,
 * pt_bvh_build_sah2) */
static napi_value js_bvh_build(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    bool sah = false;
    if (argc > 2) {
        napi_valuetype t;
        if (napi_typeof(env, argv[2], &t) != napi_ok || (t != napi_undefined && napi_get_value_bool(env, argv[2], &sah) != napi_ok)) {
            napi_throw_type_error(env, NULL, "bvhBuild(Float64Array vertices, Int32Array tris, sah?, isolate?)");
            return NULL;
        }
    }
    const uint8_t* iso = NULL;
    size_t niso = 0;
    if (argc > 3) {
        napi_valuetype t;
        napi_typedarray_type ti;
        void* di = NULL;
        size_t oi;
        napi_value abi;
        if (napi_typeof(env, argv[3], &t) != napi_ok ||
            (t != napi_undefined && (napi_get_typedarray_info(env, argv[3], &ti, &niso, &di, &abi, &oi) != napi_ok ||
                                     ti != napi_uint8_array))) {
            napi_throw_type_error(env, NULL, "bvhBuild(..., isolate: Uint8Array of material flags)");
            return NULL;
        }
        iso = (const uint8_t*)di;
    }
    napi_typedarray_type t0, t1;
    size_t n0 = 0, n1 = 0, off;
    void *d0 = NULL, *d1 = NULL;
    napi_value ab;
    if (argc < 2 || napi_get_typedarray_info(env, argv[0], &t0, &n0, &d0, &ab, &off) != napi_ok ||
        napi_get_typedarray_info(env, argv[1], &t1, &n1, &d1, &ab, &off) != napi_ok || t0 != napi_float64_array ||
        t1 != napi_int32_array || n0 % 3 || n1 % 4) {
        napi_throw_type_error(env, NULL, "bvhBuild(Float64Array vertices, Int32Array tris)");
        return NULL;
    }
    size_t len = 0;
    int rc = !sah ? pt_bvh_build((const double*)d0, n0 / 3, (const int32_t*)d1, n1 / 4, NULL, 0, &len)
                  : pt_bvh_build_sah2((const double*)d0, n0 / 3, (const int32_t*)d1, n1 / 4, iso, iso ? niso : 0, NULL, 0, &len);
    if (rc) return throw_pt(env, rc);
    napi_value buf, arr;
    void* data = NULL;
    CHECK_NAPI(env, napi_create_arraybuffer(env, len * sizeof(float), &data, &buf));
    rc = !sah ? pt_bvh_build((const double*)d0, n0 / 3, (const int32_t*)d1, n1 / 4, (float*)data, len, &len)
              : pt_bvh_build_sah2((const double*)d0, n0 / 3, (const int32_t*)d1, n1 / 4, iso, iso ? niso : 0, (float*)data,
                                  len, &len);
    if (rc) return throw_pt(env, rc);
    CHECK_NAPI(env, napi_create_typedarray(env, napi_float32_array, len, buf, 0, &arr));
    return arr;
}

/* profileEnable(scene, bool): bracket every kernel launch of the scene with HIP events */
static napi_value js_profile_enable(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    pt_scene* s = argc ? get_scene(env, argv[0]) : NULL;
    bool on = true;
    if (!s || (argc > 1 && napi_get_value_bool(env, argv[1], &on) != napi_ok)) {
        if (!pending_exception(env)) napi_throw_type_error(env, NULL, "profileEnable(scene, enable)");
        return NULL;
    }
    int rc = pt_profile_enable(s, on ? 1 : 0);
    if (rc) return throw_pt(env, rc);
    return NULL;
}

/* sceneSetVertexNormals(scene, enable): vertex-normal shading (pt_scene_set_vertex_normals) */
static napi_value js_scene_set_vertex_normals(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    pt_scene* s = argc ? get_scene(env, argv[0]) : NULL;
    bool on = true;
    if (!s || (argc > 1 && napi_get_value_bool(env, argv[1], &on) != napi_ok)) {
        if (!pending_exception(env)) napi_throw_type_error(env, NULL, "sceneSetVertexNormals(scene, enable)");
        return NULL;
    }
    int rc = pt_scene_set_vertex_normals(s, on ? 1 : 0);
    if (rc) return throw_pt(env, rc);
    return NULL;
}

/* {model, lensRadius = 0, focusDistance = 1} -> pt_camera.  model: 'pinhole' | 'thin_lens' (or 'thinlens') | 'ortho' |
 * 'equirect', or its number; null or undefined instead of the object: the pinhole. */
static bool parse_camera(napi_env env, napi_value obj, pt_camera* out) {
    pt_camera cam = {PT_CAMERA_PINHOLE, 0.0f, 1.0f, 0};
    bool ok = true;
    napi_valuetype t = napi_undefined;
    if (napi_typeof(env, obj, &t) != napi_ok) return false;
    if (t == napi_object) {
        napi_value v;
        napi_valuetype vt = napi_undefined;
        ok = napi_get_named_property(env, obj, "model", &v) == napi_ok && napi_typeof(env, v, &vt) == napi_ok;
        if (ok && vt == napi_string) {
            char name[16] = "";
            size_t len = 0;
            ok = napi_get_value_string_utf8(env, v, name, sizeof name, &len) == napi_ok;
            if (!strcmp(name, "pinhole")) cam.model = PT_CAMERA_PINHOLE;
            else if (!strcmp(name, "thin_lens") || !strcmp(name, "thinlens")) cam.model = PT_CAMERA_THIN_LENS;
            else if (!strcmp(name, "ortho")) cam.model = PT_CAMERA_ORTHO;
            else if (!strcmp(name, "equirect")) cam.model = PT_CAMERA_EQUIRECT;
            else ok = false;
        } else if (ok && vt == napi_number) {
            ok = napi_get_value_uint32(env, v, &cam.model) == napi_ok;
        } else {
            ok = false;
        }
        const char* keys[2] = {"lensRadius", "focusDistance"};
        float* dst[2] = {&cam.lens_radius, &cam.focus_distance};
        for (int k = 0; k < 2 && ok; ++k) {
            double d;
            if (napi_get_named_property(env, obj, keys[k], &v) != napi_ok || napi_typeof(env, v, &vt) != napi_ok) ok = false;
            else if (vt == napi_number) { ok = napi_get_value_double(env, v, &d) == napi_ok; *dst[k] = (float)d; }
            else if (vt != napi_undefined) ok = false;
        }
    } else if (t != napi_undefined && t != napi_null) {
        ok = false;
    }
    if (ok) *out = cam;
    return ok;
}

/* sceneSetCamera(scene, {model, lensRadius = 0, focusDistance = 1}): the camera model of later calls on the
 * scene (pt_scene_set_camera); the object as parse_camera takes it. */
static napi_value js_scene_set_camera(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    pt_scene* s = argc ? get_scene(env, argv[0]) : NULL;
    pt_camera cam = {PT_CAMERA_PINHOLE, 0.0f, 1.0f, 0};
    bool ok = s != NULL;
    if (ok && argc > 1) ok = parse_camera(env, argv[1], &cam);
    if (!ok) {
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL, "sceneSetCamera(scene, {model: 'pinhole'|'thin_lens'|'ortho'|'equirect', lensRadius, focusDistance})");
        return NULL;
    }
    int rc = pt_scene_set_camera(s, &cam);
    if (rc) return throw_pt(env, rc);
    return NULL;
}

/* renderViews(scene, [{meta: Float32Array[48], window: [x0, y0, w, h] | undefined, camera: {model, lensRadius,
 * focusDistance} | undefined, dst: [x, y], frame0 = 0}, ...], atlasW, atlasH, nframes, stride, maxDepth, mode,
 * accum[atlasH*atlasW*3][, counters=true]) -> Promise<counters|null>: the views of the list in one pass, each at
 * its place of the atlas accumulator (pt_render_views).  The library checks the list. */
#define PT_NODE_MAX_VIEWS 65536u
typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref refs[2]; /* scene, accum kept alive while the worker runs */
    scene_box* box;
    pt_scene* scene;
    pt_view* views; /* malloc'd */
    size_t n;
    uint32_t atlas_w, atlas_h, nframes, stride;
    int32_t max_depth, mode;
    float* accum;
    pt_counters counters;
    int want_counters;
    int rc;
    char err[512];
} views_job;

static void views_execute(napi_env env, void* data) {
    (void)env;
    views_job* j = (views_job*)data;
    j->rc = pt_render_views(j->scene, j->views, j->n, j->atlas_w, j->atlas_h, j->nframes, j->stride, j->max_depth, j->mode,
                            j->accum, j->want_counters ? &j->counters : NULL);
    if (j->rc) snprintf(j->err, sizeof j->err, "pt_hip error %d: %s", j->rc, pt_last_error());
}

static void views_complete(napi_env env, napi_status status, void* data) {
    views_job* j = (views_job*)data;
    if (j->box) j->box->busy = 0;
    if (status == napi_ok && j->rc == 0) {
        napi_value none;
        napi_get_null(env, &none);
        napi_resolve_deferred(env, j->deferred, j->want_counters ? counters_obj(env, &j->counters) : none);
    } else {
        napi_value msg, e;
        napi_create_string_utf8(env, j->rc ? j->err : "render cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, NULL, msg, &e);
        napi_reject_deferred(env, j->deferred, e);
    }
    for (int i = 0; i < 2; ++i) napi_delete_reference(env, j->refs[i]);
    napi_delete_async_work(env, j->work);
    free(j->views);
    free(j);
}

/* one view object into *v; the window defaults to the whole image of meta[0..1] */
static int parse_view(napi_env env, napi_value obj, pt_view* v) {
    napi_valuetype t;
    napi_value e;
    float* meta;
    size_t ml;
    memset(v, 0, sizeof *v);
    if (napi_typeof(env, obj, &t) != napi_ok || t != napi_object) return 0;
    if (napi_get_named_property(env, obj, "meta", &e) != napi_ok || !get_f32(env, e, &meta, &ml) || ml < 48) return 0;
    memcpy(v->meta, meta, sizeof v->meta);
    if (napi_get_named_property(env, obj, "window", &e) != napi_ok || napi_typeof(env, e, &t) != napi_ok) return 0;
    if (t == napi_undefined || t == napi_null) {
        if (!(v->meta[0] >= 1.0f && v->meta[0] <= 32768.0f && v->meta[1] >= 1.0f && v->meta[1] <= 32768.0f)) return 0;
        v->win.w = (uint32_t)v->meta[0];
        v->win.h = (uint32_t)v->meta[1];
    } else if (!parse_window(env, e, &v->win)) {
        return 0;
    }
    if (napi_get_named_property(env, obj, "camera", &e) != napi_ok || !parse_camera(env, e, &v->cam)) return 0;
    if (v->cam.model == PT_CAMERA_PINHOLE) v->cam.lens_radius = v->cam.focus_distance = 0.0f;
    bool is_arr = false;
    uint32_t n = 0;
    napi_value c;
    if (napi_get_named_property(env, obj, "dst", &e) != napi_ok || napi_is_array(env, e, &is_arr) != napi_ok || !is_arr ||
        napi_get_array_length(env, e, &n) != napi_ok || n != 2)
        return 0;
    uint32_t* out[2] = {&v->dst_x, &v->dst_y};
    for (uint32_t i = 0; i < 2; ++i) {
        double d;
        if (napi_get_element(env, e, i, &c) != napi_ok || napi_get_value_double(env, c, &d) != napi_ok) return 0;
        if (!(d >= 0.0 && d <= 4294967295.0) || d != (double)(uint32_t)d) return 0;
        *out[i] = (uint32_t)d;
    }
    if (napi_get_named_property(env, obj, "frame0", &e) != napi_ok || napi_typeof(env, e, &t) != napi_ok) return 0;
    if (t != napi_undefined) {
        double d;
        if (napi_get_value_double(env, e, &d) != napi_ok || !(d >= 0.0 && d <= 4294967295.0) || d != (double)(uint32_t)d) return 0;
        v->frame0 = (uint32_t)d;
    }
    return 1;
}

static int parse_views_args(napi_env env, napi_callback_info info, views_job* j, napi_value argv[10]) {
    size_t argc = 10;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < 9 || argc > 10) return 0;
    bool want = true;
    napi_valuetype t;
    if (argc > 9) {
        if (napi_typeof(env, argv[9], &t) != napi_ok) return 0;
        if (t != napi_undefined && napi_get_value_bool(env, argv[9], &want) != napi_ok) return 0;
    }
    j->want_counters = want ? 1 : 0;
    j->box = get_box(env, argv[0]);
    j->scene = get_scene(env, argv[0]);
    if (!j->scene) return 0;
    bool is_arr = false;
    uint32_t n = 0;
    if (napi_is_array(env, argv[1], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, argv[1], &n) != napi_ok ||
        n < 1 || n > PT_NODE_MAX_VIEWS)
        return 0;
    j->views = (pt_view*)malloc((size_t)n * sizeof(pt_view));
    if (!j->views) return 0;
    j->n = n;
    for (uint32_t k = 0; k < n; ++k) {
        napi_value e;
        if (napi_get_element(env, argv[1], k, &e) != napi_ok || !parse_view(env, e, &j->views[k])) return 0;
    }
    size_t al;
    if (!get_u32(env, argv[2], &j->atlas_w) || !get_u32(env, argv[3], &j->atlas_h) || !get_u32(env, argv[4], &j->nframes) ||
        !get_u32(env, argv[5], &j->stride) || !get_i32(env, argv[6], &j->max_depth) || !get_i32(env, argv[7], &j->mode) ||
        !get_f32(env, argv[8], &j->accum, &al))
        return 0;
    return al == (size_t)j->atlas_w * j->atlas_h * 3;
}

static napi_value js_render_views(napi_env env, napi_callback_info info) {
    napi_value argv[10];
    views_job* j = (views_job*)calloc(1, sizeof(views_job));
    if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    if (!parse_views_args(env, info, j, argv)) {
        free(j->views);
        free(j);
        if (!pending_exception(env))
            napi_throw_type_error(env, NULL,
                                  "renderViews(scene, [{meta: Float32Array[48], window: [x0, y0, w, h]?, camera: {model, lensRadius, "
                                  "focusDistance}?, dst: [x, y], frame0?}, ...], atlasW, atlasH, nframes, stride, maxDepth, mode, "
                                  "Float32Array accum[atlasH*atlasW*3], counters?)");
        return NULL;
    }
    j->box->busy = 1;
    napi_value promise, name;
    CHECK_NAPI(env, napi_create_promise(env, &j->deferred, &promise));
    napi_create_reference(env, argv[0], 1, &j->refs[0]);
    napi_create_reference(env, argv[8], 1, &j->refs[1]);
    napi_create_string_utf8(env, "pt_render_views", NAPI_AUTO_LENGTH, &name);
    CHECK_NAPI(env, napi_create_async_work(env, NULL, name, views_execute, views_complete, j, &j->work));
    CHECK_NAPI(env, napi_queue_async_work(env, j->work));
    return promise;
}

/* profileRead(scene) -> {kernel: {launches, totalMs, minMs, maxMs, busyMs}} */
static napi_value js_profile_read(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    CHECK_NAPI(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    pt_scene* s = argc ? get_scene(env, argv[0]) : NULL;
    if (!s) { if (!pending_exception(env)) napi_throw_type_error(env, NULL, "profileRead(scene)"); return NULL; }
    pt_kernel_time kt[16];
    int n = 0;
    int rc = pt_profile_read(s, kt, 16, &n);
    if (rc) return throw_pt(env, rc);
    napi_value o, k, v;
    napi_create_object(env, &o);
    for (int i = 0; i < n; ++i) {
        napi_create_object(env, &k);
        napi_create_double(env, (double)kt[i].launches, &v); napi_set_named_property(env, k, "launches", v);
        napi_create_double(env, kt[i].total_ms, &v); napi_set_named_property(env, k, "totalMs", v);
        napi_create_double(env, kt[i].min_ms, &v); napi_set_named_property(env, k, "minMs", v);
        napi_create_double(env, kt[i].max_ms, &v); napi_set_named_property(env, k, "maxMs", v);
        napi_create_double(env, kt[i].busy_ms, &v); napi_set_named_property(env, k, "busyMs", v);
        napi_set_named_property(env, o, kt[i].name, k);
    }
    return o;
}

static napi_value init(napi_env env, napi_value exports) {
    napi_property_descriptor props[] = {
        {"abiVersion", NULL, js_abi_version, NULL, NULL, NULL, napi_enumerable, NULL},
        {"deviceCount", NULL, js_device_count, NULL, NULL, NULL, napi_enumerable, NULL},
        {"setOption", NULL, js_set_option, NULL, NULL, NULL, napi_enumerable, NULL},
        {"sceneCreate", NULL, js_scene_create, NULL, NULL, NULL, napi_enumerable, NULL},
        {"sceneInfo", NULL, js_scene_info, NULL, NULL, NULL, napi_enumerable, NULL},
        {"sceneDestroy", NULL, js_scene_destroy, NULL, NULL, NULL, napi_enumerable, NULL},
        {"render", NULL, js_render, NULL, NULL, NULL, napi_enumerable, NULL},
        /* added after the ABI 3 surface: callable by name but not enumerable, so Object.keys(addon) —
         * which tests/test_host_node.py pins — still lists exactly the original set */
        {"renderWindow", NULL, js_render_window, NULL, NULL, NULL, napi_default, NULL},
        {"renderRects", NULL, js_render_rects, NULL, NULL, NULL, napi_default, NULL},
        {"renderViews", NULL, js_render_views, NULL, NULL, NULL, napi_default, NULL},
        {"renderSync", NULL, js_render_sync, NULL, NULL, NULL, napi_enumerable, NULL},
        {"renderMulti", NULL, js_render_multi, NULL, NULL, NULL, napi_enumerable, NULL},
        {"renderImage", NULL, js_render_image, NULL, NULL, NULL, napi_enumerable, NULL},
        {"renderDenoised", NULL, js_render_denoised, NULL, NULL, NULL, napi_default, NULL},
        {"queryHits", NULL, js_query_hits, NULL, NULL, NULL, napi_default, NULL},
        {"queryOccluded", NULL, js_query_occluded, NULL, NULL, NULL, napi_default, NULL},
        {"cameraRays", NULL, js_camera_rays, NULL, NULL, NULL, napi_default, NULL},
        {"cameraSeeds", NULL, js_camera_seeds, NULL, NULL, NULL, napi_default, NULL},
        {"queryRadiance", NULL, js_query_radiance, NULL, NULL, NULL, napi_default, NULL},
        {"gather", NULL, js_gather, NULL, NULL, NULL, napi_default, NULL},
        {"gatherRays", NULL, js_gather_rays, NULL, NULL, NULL, napi_default, NULL},
        {"frame", NULL, js_frame, NULL, NULL, NULL, napi_enumerable, NULL},
        {"tonemap", NULL, js_tonemap, NULL, NULL, NULL, napi_enumerable, NULL},
        {"profileEnable", NULL, js_profile_enable, NULL, NULL, NULL, napi_enumerable, NULL},
        {"profileRead", NULL, js_profile_read, NULL, NULL, NULL, napi_enumerable, NULL},
        {"bvhBuild", NULL, js_bvh_build, NULL, NULL, NULL, napi_enumerable, NULL},
        {"bvhBuildLbvh", NULL, js_bvh_build_lbvh, NULL, NULL, NULL, napi_default, NULL},
        {"sceneCreateMesh", NULL, js_scene_create_mesh, NULL, NULL, NULL, napi_default, NULL},
        {"sceneExportBvh", NULL, js_scene_export_bvh, NULL, NULL, NULL, napi_default, NULL},
        {"sceneSetVertexNormals", NULL, js_scene_set_vertex_normals, NULL, NULL, NULL, napi_enumerable, NULL},
        {"sceneSetCamera", NULL, js_scene_set_camera, NULL, NULL, NULL, napi_default, NULL},
        {"reproject", NULL, js_reproject, NULL, NULL, NULL, napi_default, NULL},
        {"denoiseMean", NULL, js_denoise_mean, NULL, NULL, NULL, napi_default, NULL},
        {"historyCreate", NULL, js_history_create, NULL, NULL, NULL, napi_default, NULL},
        {"historyStep", NULL, js_history_step, NULL, NULL, NULL, napi_default, NULL},
        {"historyReset", NULL, js_history_reset, NULL, NULL, NULL, napi_default, NULL},
        {"historyDestroy", NULL, js_history_destroy, NULL, NULL, NULL, napi_default, NULL},
    };
    napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
