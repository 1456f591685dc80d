/*
 * pt_hip.h — C ABI of the MI355X (gfx950) path-tracing core.
 *
 * Drop-in boundary for the reference's render path (Kauhentus/brown-cs2240-path-tracer):
 * everything behind `programEntry(screenDimension, ctx, primitive_data, camera_data,
 * scene_description)` (src/program-raymarch.ts:50-54) — the WebGPU device/buffer setup
 * (:71-213), the per-frame dispatch + readback + host accumulation loop (:226-335) and the
 * WGSL megakernel it dispatches (src/program-raymarch.wgsl:35-303 with
 * the src/wgsl-util WGSL files) — is replaced by the calls below.  Inputs are the reference's own
 * packed buffers, bit for bit: `SceneObjectPacked.triangle_data` / `.bvh_data`
 * (src/ts-util/data-structs.ts:46-50, produced by src/packer.ts:4-137) and the 48-float
 * meta block (src/program-raymarch.ts:79-92; layout SURVEY.md §8a A2).
 *
 * Conventions: plain pointers and sizes, no torch/HIP types in signatures (streams are
 * `void*` = hipStream_t).  Every function returns PT_OK (0) or a negative pt_status; the
 * message is available from pt_last_error() (thread-local).  Calls on one scene are not
 * re-entrant; distinct scenes may be used from distinct threads.  Ownership: the library
 * owns all device memory of a scene; the caller owns every buffer it passes in.
 *
 * RNG salts: the reference salts each dispatch with the wall-clock `time_elapsed` in ms
 * (program-raymarch.ts:227,246 -> meta[11]); here frame k of a render is salted with
 * t_k = u32(f32(k)) so results are reproducible.  meta[11] is ignored.
 */
#ifndef PT_HIP_H
#define PT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 3

typedef enum {
    PT_OK = 0,
    PT_ERR_INVALID = -1,  /* bad argument (null pointer, zero size, bad meta) */
    PT_ERR_SCENE = -2,    /* malformed packed buffers (see pt_last_error) */
    PT_ERR_NOMEM = -3,    /* device or host allocation failed */
    PT_ERR_HIP = -4,      /* HIP runtime error */
    PT_ERR_NODEVICE = -5  /* no gfx950 device / bad device ordinal */
} pt_status;

typedef enum {
    PT_MODE_AUTO = 0,       /* wavefront at every size on <= 64-entry (mailbox) and big-leaf scenes, else from 2^19 paths (W*H*nframes); megakernel below */
    PT_MODE_MEGAKERNEL = 1, /* one lane per pixel, frames looped in-lane */
    PT_MODE_WAVEFRONT = 2   /* SoA path/ray queues, per-bounce kernels, wave64 compaction */
} pt_mode;

/* Work counters (optional). A "sample" is one camera path with all its bounces
 * and shadow rays; queries count closest-hit traversals. */
typedef struct {
    uint64_t samples;
    uint64_t ext_queries;
    uint64_t shadow_queries;
    uint64_t nodes;      /* BVH nodes popped (each tests 2 child boxes) */
    uint64_t tri_tests;
    uint64_t box_tests;
} pt_counters;

typedef struct {
    uint32_t nodes;        /* internal nodes (root included) */
    uint32_t leaves;
    uint32_t leaf_refs;    /* triangle references in leaves (duplicates included) */
    uint32_t max_leaf;
    uint32_t max_stack;    /* deepest traversal stack the tree can produce */
    uint32_t materials;
    uint32_t emissive_tris;/* Ntri of sample_area_lights */
    uint32_t vertices;
    uint64_t device_bytes; /* HBM held by the scene */
} pt_scene_info;

typedef struct pt_scene pt_scene;

/* Per-kernel launch timing (pt_profile_read). */
typedef struct {
    char name[32];     /* "k_regen", "k_wf_trace", "k_wf_shade_ext", ... */
    uint64_t launches;
    double total_ms;   /* sum over launches of the HIP-event time around each launch */
    double min_ms;
    double max_ms;
    double busy_ms;    /* GPU time during which at least one launch of the kernel ran: the union of the
                          launches' event intervals (launches on several streams overlap, so this is
                          <= total_ms; bytes / busy_ms is the kernel's achieved rate) */
} pt_kernel_time;

/* ABI version of the loaded library (== PT_ABI_VERSION when headers match). */
int pt_abi_version(void);

/* Last error message of the calling thread ("" if none). */
const char* pt_last_error(void);

/* Number of visible HIP devices. */
int pt_device_count(int* count_out);

/* Upload a scene.  Replaces the storage-buffer creation of program-raymarch.ts:109-131
 * (bindings 3 and 10).  Validates the packed layouts and re-encodes them for the device
 * (brown-cs2240-path-tracer_amd/csrc/pt_layout.h).  device: HIP ordinal. */
int pt_scene_create(const float* triangle_data, size_t triangle_len, const float* bvh_data, size_t bvh_len,
                    int device, pt_scene** scene_out);
void pt_scene_destroy(pt_scene* scene);
int pt_scene_get_info(const pt_scene* scene, pt_scene_info* info_out);

/* Vertex-normal shading (off by default = the reference's behaviour): the
 * hit normal of a triangle whose third index i2 = (idx2 - 1) * 3 < vn_range (triangle_data[6])
 * becomes normalize(w*n0 + u*n1 + v*n2) with the test's barycentrics and the normals at
 * vn_start + (idx - 1) * 3 (triangle_data[5]) — ray_triangle_intersection_vertex_normals
 * (src/wgsl-util/ray-triangle-intersection.wgsl:44-87), which the reference calls only from
 * commented-out code (src/wgsl-util/intersection-logic.wgsl:81-108).  Changes results on scenes
 * with vertex normals.  Applies to later renders of the scene. */
int pt_scene_set_vertex_normals(pt_scene* scene, int enable);

/* Lens cameras, evaluated on the device where a render makes its camera paths.  A
 * scene-level setting like pt_scene_set_vertex_normals: it applies to later calls on the scene and
 * reaches every entry point that makes camera paths — pt_render*, pt_render_window*, pt_render_moments*,
 * pt_render_rects*, pt_render_adaptive, pt_render_features*, pt_render_denoised_image, pt_render_image,
 * pt_frame*, pt_camera_rays* — while pt_camera_seeds is independent of it.  cam NULL or model
 * PT_CAMERA_PINHOLE: the reference's jittered pinhole, and every call launches what it always launched.
 *
 * Every model keeps the pinhole's prologue (program-raymarch.wgsl:50-76): the pixel's seed chain, its
 * jitter, norm_x / norm_y, vx / vy and the radiance seed — so the anti-aliasing jitter and the seed of a
 * (pixel, frame) do not depend on the model.  With M = cam_to_world (meta[28..43], column-major),
 * X(c)_k = fma(M[12+k], 1, fma(M[8+k], c.z, fma(M[4+k], c.y, M[k] * c.x))) and N3(v) = v / sqrt(fma(v.z,
 * v.z, fma(v.y, v.y, v.x * v.x))), every operation f32 and rounded once, sincos the pinned one, PI 3.14159f:
 *   THIN_LENS  hl = hash1u(ts + 0x9e3779b9) (ts: the chain after its third hash), (u1, u2) = hash2(hl),
 *              r = lens_radius * sqrt(u1), phi = (2 PI) * u2, l = (r cos phi, r sin phi, 0),
 *              k = focus_distance / focal, c = (vx * k, vy * k, -focus_distance),
 *              o = X(l), d = N3(X(c) - o).
 *              The origin comes from M's translation column, not from meta[4..6]; every meta the hosts
 *              make has the two equal.  lens_radius = 0 is a pinhole that differs from the reference's
 *              in rounding only.
 *   ORTHO      k = focus_distance / focal, o = X((vx * k, vy * k, 0)), d = N3((-M[8], -M[9], -M[10])):
 *              what the pinhole sees at the plane of focus, in parallel projection.
 *   EQUIRECT   phi = norm_x * (2 PI), th = norm_y * PI, c = (cos th sin phi, sin th, -(cos th cos phi)),
 *              o = meta[4..6], d = N3(M's rotation applied to c); aspect, focal and vfov play no part.
 * Contract: a pixel's sample of frame k is the reference's radiance(ray, seed) for that ray (inv = 1 / d)
 * and the pinhole's seed, clamped and added in frame order — per frame, pt_query_radiance(nsamples = 1)
 * on pt_camera_rays and pt_camera_seeds.  A direction that pt_query_radiance would not admit (a lens
 * point that coincides with its target gives NaN) contributes nothing to that sample — the accumulator
 * keeps its bits — and adds to no counter; pt_camera_rays reports it as computed.  (pt_frame* writes -0
 * for such a sample, and pt_render_moments turns a second moment of -0 into +0.)
 * With a model set a call always runs the wavefront pipeline with camera paths from the generate kernel:
 * options kernel=mega|literal, fuse_gen and regen do not apply, as for pt_query_radiance.
 * Errors (PT_ERR_INVALID): unknown model; THIN_LENS with lens_radius not finite or < 0, or
 * focus_distance not finite or <= 0; ORTHO with focus_distance not finite or <= 0.  Fields a model does
 * not use are ignored (lens_radius by ORTHO and EQUIRECT, focus_distance by EQUIRECT).
 * pt_render_multi needs the same pt_camera (bytewise) on all its scenes. */
typedef enum { PT_CAMERA_PINHOLE = 0, PT_CAMERA_THIN_LENS = 1, PT_CAMERA_ORTHO = 2, PT_CAMERA_EQUIRECT = 3 } pt_camera_model;
typedef struct { uint32_t model; float lens_radius; float focus_distance; uint32_t reserved; } pt_camera; /* 16 B */
int pt_scene_set_camera(pt_scene* scene, const pt_camera* cam);
int pt_scene_get_camera(const pt_scene* scene, pt_camera* cam_out);

/* Render frames k = frame0 + i*frame_stride, i < nframes, each 1 spp per pixel, and add
 * clamp(L) (v >= 0 ? v : 0, NaN -> 0) into accum in frame order — the render_loop of
 * program-raymarch.ts:226-335 without the per-frame readback.  accum: host f32
 * [H][W][3], in/out.  max_depth: the literal 16 of `while(depth <= 16)`
 * (program-raymarch.wgsl:118); pass -1 for 16.  counters: nullable.  Blocking. */
int pt_render(pt_scene* scene, const float meta[48], uint32_t frame0, uint32_t nframes, uint32_t frame_stride,
              int max_depth, int mode, float* accum, pt_counters* counters);

/* Same on device memory, asynchronous on `stream` (hipStream_t; NULL = default stream).
 * d_accum: device f32 [H][W][3] in/out.  d_counters: device pt_counters or NULL (added to).
 * A device-side failure of an earlier asynchronous render of this scene (a traversal wave that
 * gave up, see pt_scene_check) is reported by the next call once that render has completed:
 * this call then fails with PT_ERR_HIP and renders nothing. */
int pt_render_async(pt_scene* scene, const float meta[48], uint32_t frame0, uint32_t nframes, uint32_t frame_stride,
                    int max_depth, int mode, float* d_accum, pt_counters* d_counters, void* stream);

/* A window of the image: pixels [x0, x0 + w) x [y0, y0 + h) of the W x H image of meta[0..1]
 * (y0 = the image's top row, as in every [H][W][3] buffer here); w, h >= 1, x0 + w <= W,
 * y0 + h <= H, else PT_ERR_INVALID.  NULL where a window is accepted = the whole image. */
typedef struct { uint32_t x0, y0, w, h; } pt_window;

/* pt_render for the pixels of a window only: accum is host f32 [h][w][3], in/out, the window's
 * pixels row-major.  Frame salts, seeds, rays and results are those of the full image's pixels:
 * the window's accumulator holds the same bits as that rectangle of a pt_render of the whole
 * image started from the same values, whatever the window, pipeline or batch shape (a pixel
 * depends on its image coordinates only).  AUTO chooses the pipeline by the window's paths
 * (w * h * nframes).  counters: nullable, the window's paths only.  pt_render is this with
 * win = NULL.  Blocking. */
int pt_render_window(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t frame0, uint32_t nframes,
                     uint32_t frame_stride, int max_depth, int mode, float* accum, pt_counters* counters);

/* pt_render_async for a window: d_accum points at the window's FIRST pixel in device memory and
 * row_pitch is the distance between its rows in pixels (>= w, else PT_ERR_INVALID).  row_pitch = w
 * is a dense [h][w][3] buffer; row_pitch = W with d_accum = image + 3 * (y0 * W + x0) renders the
 * window in place inside a full [H][W][3] image, of which nothing outside the window is read or
 * written — tiles of one image may be rendered by separate calls, on separate scenes or devices.
 * Same bits as pt_render_window.  d_counters: device pt_counters or NULL (added to). */
int pt_render_window_async(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t frame0,
                           uint32_t nframes, uint32_t frame_stride, int max_depth, int mode, float* d_accum,
                           size_t row_pitch, pt_counters* d_counters, void* stream);

/* pt_render_window / pt_render_window_async that also accumulate the second moments: for every pixel
 * and channel, beside accum += c with c = (L >= 0 ? L : 0), m2 = m2 + c * c (the product rounded to
 * f32, then the sum), frame after frame from the value already in the buffer.  m2 / d_m2: f32, the
 * accumulator's shape and pitch, in/out, not NULL.  The accumulator's bits and the counters are those
 * of the call without moments.  win NULL = the whole image. */
int pt_render_moments(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t frame0, uint32_t nframes,
                      uint32_t frame_stride, int max_depth, int mode, float* accum, float* m2, pt_counters* counters);
int pt_render_moments_async(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t frame0,
                            uint32_t nframes, uint32_t frame_stride, int max_depth, int mode, float* d_accum,
                            float* d_m2, size_t row_pitch, pt_counters* d_counters, void* stream);

/* Render frames frame0 + i*stride (i < nframes) of the pixels of n rectangles of the image, in ONE
 * pass through the pipeline: the paths of all rectangles share the call's batches and launches.
 * rects: image coordinates, each inside `frame` (NULL = the whole image), pairwise disjoint, w,h >= 1,
 * 1 <= n <= 65536, in any order.  Destination: d_accum points at frame's first pixel, rows row_pitch
 * pixels apart (>= frame->w); pixel (x, y) of a rectangle lives at
 * d_accum + 3*((y - frame.y0)*row_pitch + (x - frame.x0)); in/out; nothing outside the rectangles is
 * read or written.  d_m2: nullable, second moments at the same places (pt_render_moments' rule).
 * Every pixel gets the bits of pt_render_window[_moments] of any window that holds it.
 * A path's id is f * npix + q: npix the sum of the rectangles' areas ("paths per frame" for AUTO's
 * choice of pipeline, the batches and the counters), q the pixel's position in the concatenation of
 * the rectangles in list order, row-major inside each.  An empty list, n > 65536, a rectangle of no
 * area or outside frame or the image, and any two rectangles that share a pixel (two slots on one
 * pixel would race in the accumulation) fail with PT_ERR_INVALID before anything is launched or
 * copied; pt_last_error() names the offending rectangle(s).  The rectangle table lives in device
 * memory of the scene and is written on `stream` before the first launch. */
int pt_render_rects_async(pt_scene* scene, const float meta[48], const pt_window* frame, const pt_window* rects,
                          size_t n, uint32_t frame0, uint32_t nframes, uint32_t frame_stride, int max_depth, int mode,
                          float* d_accum, float* d_m2, size_t row_pitch, pt_counters* d_counters, void* stream);
/* Blocking, host buffers: accum (and nullable m2) dense [frame.h][frame.w][3], in/out. */
int pt_render_rects(pt_scene* scene, const float meta[48], const pt_window* frame, const pt_window* rects, size_t n,
                    uint32_t frame0, uint32_t nframes, uint32_t frame_stride, int max_depth, int mode, float* accum,
                    float* m2, pt_counters* counters);
/* Host only, for tests: validates a list and writes each rectangle's first slot (prefix sum of w*h in
 * list order) and *npix_out = the pixels per frame.  W, H: the image's size; first_out, npix_out: nullable. */
int pt_selftest_rect_plan(const pt_window* frame, uint32_t W, uint32_t H, const pt_window* rects, size_t n,
                          uint64_t* first_out, uint64_t* npix_out);

/* A list of views: n images of one scene, each with its own meta, window, camera model,
 * first frame and place in a shared atlas, rendered in ONE pass through the pipeline — the paths of all
 * views share the call's batches and launches, as the rectangles of pt_render_rects do. */
typedef struct {
    float     meta[48];     /* the view's own image and camera, as pt_render takes it */
    pt_window win;          /* the window of THAT image to render (w, h >= 1, inside meta[0..1]) */
    pt_camera cam;          /* model of this view; PT_CAMERA_PINHOLE = the reference's camera */
    uint32_t  dst_x, dst_y; /* where window pixel (0, 0) lands in the atlas */
    uint32_t  frame0;       /* this view's first frame: frames frame0 + i * frame_stride */
    uint32_t  reserved;     /* 0 */
} pt_view; /* 240 B */
/* Render frames frame0_v + i*frame_stride (i < nframes) of every view v of the list.  Destination: the
 * atlas, atlas_w x atlas_h pixels (each in [1, 32768]) whose first pixel d_accum addresses, rows row_pitch
 * pixels apart (>= atlas_w); window pixel (i, j) of view v lives at
 * d_accum + 3*((dst_y + j)*row_pitch + dst_x + i); in/out; nothing outside the views' destination
 * rectangles (dst_x, dst_y, win.w, win.h) is read or written.
 * Every such pixel gets exactly the bits pt_render_window[_async](meta_v, win_v, frame0_v, nframes,
 * frame_stride, max_depth) would have put there on a scene whose pt_scene_set_camera is cam_v, started from
 * the same values: for a pinhole view the reference's radiance(ray, seed) through the unchanged camera_ray,
 * for a lens view pt_scene_set_camera's contract — a sample whose direction is not admitted leaves the
 * accumulator's bits alone and counts nothing.  The counters are the sum over the views' paths.  The scene's
 * own pt_scene_set_camera setting is not read (the views carry theirs); its other settings (vertex normals)
 * apply as to any render.
 * Shared by all views of a call, because the kernels after the generate kernel take them once per launch:
 * max_depth, meta[45] (the continuation probability) and meta[46] > 0 (direct lighting only).  Views whose
 * meta[45] differs bitwise from view 0's, or whose direct-only flag differs, are refused.
 * A path's id is f * npix + q: npix the sum of the views' window areas ("paths per frame" for the batches
 * and the counters), q the pixel's position in the concatenation of the views in list order, row-major
 * inside each window; its salt is t = u32(f32(frame0_v + f * frame_stride)).  The route is always the
 * wavefront pipeline with camera paths from the generate kernel: mode and the options kernel, fuse_gen and
 * regen do not apply, as under a lens camera.
 * views NULL, n = 0, n > 65536, npix >= 2^31, a meta[0..1] that pt_render refuses, a window of no area or
 * outside its image, a destination rectangle outside the atlas, row_pitch < atlas_w, any two destination
 * rectangles that share a pixel (two slots on one word would race), a view whose last frame index is
 * >= 2^24, reserved != 0, a pt_camera that pt_scene_set_camera would refuse, and the shared-field
 * mismatches above fail with PT_ERR_INVALID before anything is launched or copied; pt_last_error() names
 * the offending view(s).  The view table lives in device memory of the scene and is written on `stream`
 * before the first launch. */
int pt_render_views_async(pt_scene* scene, const pt_view* views, size_t n, uint32_t atlas_w, uint32_t atlas_h,
                          uint32_t nframes, uint32_t frame_stride, int max_depth, int mode, float* d_accum,
                          size_t row_pitch, pt_counters* d_counters, void* stream);
/* Blocking, host buffers: accum dense [atlas_h][atlas_w][3], in/out. */
int pt_render_views(pt_scene* scene, const pt_view* views, size_t n, uint32_t atlas_w, uint32_t atlas_h,
                    uint32_t nframes, uint32_t frame_stride, int max_depth, int mode, float* accum,
                    pt_counters* counters);
/* Host only, for tests: validates a list as a one-frame call does and writes each view's first slot (prefix
 * sum of win.w * win.h in list order) and *npix_out = the paths per frame.  first_out, npix_out: nullable. */
int pt_selftest_view_plan(const pt_view* views, size_t n, uint32_t atlas_w, uint32_t atlas_h, uint64_t* first_out,
                          uint64_t* npix_out);

/* A tile's noise verdict: its pixels, how many of them are noisy, and the largest error estimate. */
typedef struct { uint32_t noisy, pixels; double max_err; } pt_tile_noise; /* 16 B */

/* Noise estimate per tile from the two accumulators.  Tiles of tile_w x tile_h over a w x h buffer
 * (rows row_pitch pixels apart; w, h in [1, 32768]); the right and bottom tiles are as small as the
 * buffer leaves them.  TX = ceil(w / tile_w), TY likewise.  frames[ty * TX + tx] is the tile's sample
 * count n, out[ty * TX + tx] its verdict.  Per pixel, in double, every operation rounded once, with
 * S_c, Q_c the pixel's accum and m2 values:
 *   d_c = Q_c - (S_c * S_c) / n;  v_c = d_c > 0 ? d_c : 0  (NaN -> 0);  V = (v_r + v_g) + v_b
 *   se = sqrt(V / (n * (n - 1)));  mu = ((S_r + S_g) + S_b) / n;  err = se / (mu > floor ? mu : floor)
 * — the standard error of the pixel's mean relative to its brightness.  A pixel is noisy iff
 * err > tol; max_err is the running (err > m ? err : m) from 0.  Tiles with n < 2 report noisy =
 * pixels and max_err = +inf.  tol and floor: finite, > 0.  Asynchronous on `stream`. */
int pt_noise_tiles_async(pt_scene* scene, const float* d_accum, const float* d_m2, uint32_t w, uint32_t h,
                         size_t row_pitch, uint32_t tile_w, uint32_t tile_h, const uint32_t* d_frames, double tol,
                         double floor, pt_tile_noise* d_out, void* stream);
/* The same on dense host buffers.  Blocking. */
int pt_noise_tiles(pt_scene* scene, const float* accum, const float* m2, uint32_t w, uint32_t h, uint32_t tile_w,
                   uint32_t tile_h, const uint32_t* frames, double tol, double floor, pt_tile_noise* out);

/* mean[p] = accum[p] / (float)frames[tile of p]: one correctly rounded f32 division; 0 where the
 * tile's frames are 0.  d_mean is laid out like d_accum (row_pitch).  Asynchronous on `stream`. */
int pt_tile_mean_async(pt_scene* scene, const float* d_accum, uint32_t w, uint32_t h, size_t row_pitch,
                       uint32_t tile_w, uint32_t tile_h, const uint32_t* d_frames, float* d_mean, void* stream);

/* Adaptive render: frames only where the image is still noisy. */
typedef struct {
    uint32_t tile_w, tile_h; /* >= 1 */
    uint32_t min_frames;     /* >= 2: first pass, every tile */
    uint32_t step_frames;    /* >= 1: per refinement pass */
    uint32_t max_frames;     /* >= min_frames: cap per tile */
    double tol, floor;       /* finite, > 0 (pt_noise_tiles_async) */
    double noisy_fraction;   /* in [0, 1): a tile is done when noisy <= (uint32_t)(noisy_fraction * pixels) */
} pt_adaptive;

/* Pass 0 renders frames frame0 .. frame0 + min_frames - 1 of the whole window (NULL = the image)
 * with moments.  After each pass pt_noise_tiles_async judges every tile; a tile stays active iff
 * noisy > (uint32_t)(noisy_fraction * pixels) and its frames < max_frames, and every active tile gets
 * the next min(step_frames, max_frames - frames) frames (a tile that stops never restarts, so the
 * active tiles share one frame count) as ONE in-place list render (pt_render_rects_async) of the
 * active set's rectangles (pt_selftest_tile_rects).  A tile with n frames holds the bits of that rectangle of a plain n-frame
 * render.  Outputs (host, written, not read): accum and m2 [h][w][3], tile_frames [TY][TX],
 * tile_noise [TY][TX] (the last verdicts), rgba [h][w][4] = the display transform of the per-tile
 * mean (pt_tile_mean_async, then sample_runs = 1), counters = the sum over all passes, passes = the
 * number of render passes; m2, tile_noise, rgba, counters, passes: nullable.  frame0 + max_frames
 * must not exceed 2^24.  Blocking. */
int pt_render_adaptive(pt_scene* scene, const float meta[48], const pt_window* win, const pt_adaptive* ad,
                       uint32_t frame0, int max_depth, int mode, float* accum, float* m2, uint32_t* tile_frames,
                       pt_tile_noise* tile_noise, uint8_t* rgba, pt_counters* counters, uint32_t* passes);

/* Host only, for tests: the rectangles pt_render_adaptive renders for a mask of active tiles
 * (active[ty * tx_count + tx] != 0), four u32 per rectangle (tx0, ty0, width, height, in tiles).
 * Tile rows top to bottom, the maximal runs of active tiles in each; a run with the same [tx0, tx1)
 * as a rectangle still open from the row above extends it, any other opens a new one.  *n_out = the
 * rectangles; more than cap: PT_ERR_INVALID (rects holds the first cap). */
int pt_selftest_tile_rects(const uint8_t* active, uint32_t tx, uint32_t ty, uint32_t* rects, size_t cap,
                           size_t* n_out);

/* Guide buffers of the first hit, for the denoiser below.  For the frames k = frame0 + i*frame_stride,
 * i < nframes (salt t_k = u32(f32(k)) as everywhere), and every pixel of the window (NULL = the whole
 * image), the SAME jittered camera ray the render traces for that pixel and frame is traced to its
 * closest hit, and the hit is added into two f32 buffers of FOUR floats per pixel, in/out, in frame
 * order from the values already there, each component one f32 addition:
 *   geo += (n.x, n.y, n.z, t)   n: the hit's shading normal (pt_scene_set_vertex_normals is honoured),
 *                               t: the hit distance
 *   alb += (a.r, a.g, a.b, 1)   a = Ke where (Ke.r + Ke.g) + Ke.b > 0, else Kd + Ks
 * A miss adds nothing, so alb's fourth component counts the hits.  d_geo / d_alb address the window's
 * first pixel in device memory, 16-byte aligned; rows are row_pitch pixels apart (>= the window's
 * width; in pixels, as for the accumulator).  Window and pitch are checked as by
 * pt_render_window_async; failures of earlier asynchronous renders surface here as there.
 * Counters (nullable, added to): samples = ext_queries = w*h*nframes, shadow_queries = 0, nodes,
 * tri_tests and box_tests the traversal's. */
int pt_render_features_async(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t frame0,
                             uint32_t nframes, uint32_t frame_stride, float* d_geo, float* d_alb, size_t row_pitch,
                             pt_counters* d_counters, void* stream);
/* The same on dense host buffers geo, alb [h][w][4], in/out.  Blocking. */
int pt_render_features(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t frame0, uint32_t nframes,
                       uint32_t frame_stride, float* geo, float* alb, pt_counters* counters);

/* Denoiser: the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) steered by the guide
 * buffers and by the variance of the mean (the luminance weight of SVGF). */
typedef struct {
    uint32_t iters;                           /* 1..5 passes; the step of pass i is s = 2^i */
    float sigma_n, sigma_a, sigma_z, sigma_l; /* normal, albedo, depth, luminance: finite, > 0 */
} pt_denoise_params;
void pt_denoise_defaults(pt_denoise_params* p); /* 4, 0.5, 0.3, 0.1, 4.0 */

/* d_accum, d_m2: the accumulators of a w x h buffer ([h][w][3]); tile_w, tile_h, d_frames: the frame
 * count n of every tile, as for pt_noise_tiles_async (a uniform n-frame render is tile_w = w,
 * tile_h = h, frames = {n}); d_geo, d_alb: pt_render_features' buffers ([h][w][4], 16-byte aligned)
 * summed over feature_frames >= 1 frames.  Outputs: d_out [h][w][3] the filtered mean, d_var_out
 * (nullable) [h][w] the filtered variance of the mean.  Rows of ALL six buffers are row_pitch pixels
 * apart (>= w).  p NULL = pt_denoise_defaults.  Asynchronous on `stream`; the scratch (four w*h
 * float4 planes) belongs to the scene, so calls on one scene must be in stream order.
 *
 * Every operation is f32, rounded once, no FMA, in the order written, except where marked double.
 * Prepare, per pixel (n = the frames of the pixel's tile, nf = (float)feature_frames):
 *   c = acc / (float)n per channel (n = 0: 0)
 *   in double, S_c, Q_c the pixel's accum and m2: d_c = Q_c - (S_c * S_c) / n; v_c = d_c > 0 ? d_c : 0;
 *   V = (v_r + v_g) + v_b; var = (float)(V / (n * (n - 1)))  (n < 2: 0)
 *   N = geo.xyz / nf (not renormalised); Z = geo.w / nf; A = alb.xyz / nf
 *   isn = (float)(1.0 / ((double)sigma_n * (double)sigma_n)), isa likewise, isz = (float)(1.0 / (double)sigma_z)
 * Pass i = 0 .. iters - 1, s = 2^i, for pixel p: the taps q = p + s * (dx, dy), dy = -2..2 outermost,
 * dx = -2..2 inside; taps outside the w x h buffer are skipped; h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *   l_x = (c_x.r + c_x.g) + c_x.b;  den_p = sigma_l * sqrtf(var_p) + 1e-6f
 *   tn = ((dN.x*dN.x + dN.y*dN.y) + dN.z*dN.z) * isn   with dN = N_p - N_q;  ta likewise with A and isa
 *   zs = Z_p + Z_q;  tz = (|Z_p - Z_q| / (zs > 1e-6f ? zs : 1e-6f)) * isz;  tl = |l_p - l_q| / den_p
 *   e = (tn + ta) + (tz + tl);  e = e < 126 ? e : 126;  wgt = (h[dy+2] * h[dx+2]) * exp2(-e)
 *   sw += wgt;  sc += wgt * c_q (per channel);  sv += (wgt * wgt) * var_q
 *   c'_p = sc / sw;  var'_p = sv / (sw * sw)
 * with the pinned exp2 (the sigmas absorb the base).  A pass reads the previous pass's c and var of
 * every pixel; N, Z, A stay.  The centre tap has e = 0, so sw >= 9/64.  Inputs are assumed finite;
 * other inputs do not fault and give unspecified values.  Option "denoise_lds" chooses how the passes
 * read their taps, never the bits. */
int pt_denoise_async(pt_scene* scene, const float* d_accum, const float* d_m2, uint32_t w, uint32_t h, size_t row_pitch,
                     uint32_t tile_w, uint32_t tile_h, const uint32_t* d_frames, const float* d_geo, const float* d_alb,
                     uint32_t feature_frames, const pt_denoise_params* p, float* d_out, float* d_var_out, void* stream);
/* The same on dense host buffers (frames [TY][TX]; var_out nullable).  Blocking. */
int pt_denoise(pt_scene* scene, const float* accum, const float* m2, uint32_t w, uint32_t h, uint32_t tile_w,
               uint32_t tile_h, const uint32_t* frames, const float* geo, const float* alb, uint32_t feature_frames,
               const pt_denoise_params* p, float* out, float* var_out);

/* A denoised image in one call: a moments render of frames frame0 + i*stride (i < nframes, nframes >= 2)
 * of the whole image from zero, the guide buffers of frames frame0 .. frame0 + feature_frames - 1
 * (stride 1, feature_frames >= 1), pt_denoise_async (params NULL = the defaults), the device tone map
 * with sample_runs = 1, and the RGBA image [H][W][4] copied to the host.  counters: nullable, the
 * render's plus the guide pass's.  Blocking. */
int pt_render_denoised_image(pt_scene* scene, const float meta[48], uint32_t frame0, uint32_t nframes,
                             uint32_t frame_stride, int max_depth, int mode, uint32_t feature_frames,
                             const pt_denoise_params* params, uint8_t* rgba_out, pt_counters* counters);

/* The denoiser for a caller that already has the mean and the variance of the mean: d_c [h][w][3] and
 * d_var [h][w] take the place of accum, m2, the tiles and their frame counts.  Prepare is c and var as given,
 * N, Z, A as above; the constants and the passes are pt_denoise_async's, so with the c and var of its prepare
 * the result has pt_denoise_async's bits.  Rows of ALL six buffers are row_pitch pixels apart; d_geo and
 * d_alb 16-byte aligned; d_var_out nullable; the scratch is the scene's, as there. */
int pt_denoise_mean_async(pt_scene* scene, const float* d_c, const float* d_var, uint32_t w, uint32_t h, size_t row_pitch,
                          const float* d_geo, const float* d_alb, uint32_t feature_frames, const pt_denoise_params* p,
                          float* d_out, float* d_var_out, void* stream);
/* The same on dense host buffers (var_out nullable).  Blocking. */
int pt_denoise_mean(pt_scene* scene, const float* c, const float* var, uint32_t w, uint32_t h, const float* geo,
                    const float* alb, uint32_t feature_frames, const pt_denoise_params* p, float* out, float* var_out);

/* Temporal accumulation: the temporal stage of SVGF (Schied et al. 2017) for a static
 * scene.  What one image learned is carried to the next camera: the history of the pixel's surface point is
 * looked up where the PREVIOUS camera saw it and blended with the current step.
 *
 * The state is three planes of [h][w][4] f32, 16-byte aligned:
 *   hist = (c.r, c.g, c.b, N)   the accumulated mean radiance per sample; N: the history length in steps
 *                               (a float; 0: none)
 *   mom  = (q.r, q.g, q.b, 0)   the accumulated mean of the squared per-sample radiance
 *   gbuf = (n.x, n.y, n.z, Z)   this step's mean shading normal (not renormalised) and mean hit distance;
 *                               Z = 0: the pixel saw no hit
 * A step reads the previous set and writes a new one; the two sets must not overlap. */
typedef struct {
    float alpha;       /* the blend's floor, in (0, 1] */
    float normal_min;  /* a tap's least dot(N_cur, n_tap) */
    float depth_tol;   /* a tap's largest |Z_tap - Ze| / Ze, > 0 */
    float max_history; /* N is clamped to this, >= 1 */
} pt_temporal_params;                               /* 16 B; all finite */
void pt_temporal_defaults(pt_temporal_params* p); /* 0.2, 0.9, 0.1, 64 */

/* One step over the whole w x h image of meta_cur (w = meta[0], h = meta[1] of both metas, else
 * PT_ERR_INVALID).  d_accum, d_m2 [h][w][3]: the sums of an n-frame moments render from zero, n >= 1;
 * d_geo, d_alb [h][w][4]: pt_render_features' sums (16-byte aligned).  meta_prev and the three d_*_prev
 * planes: the previous step's camera and state, ALL NULL for a first step (a mixed set is PT_ERR_INVALID).
 * Outputs: the three new planes and, both nullable, d_out [h][w][3] = c' and d_var [h][w], the variance of
 * the accumulated mean.  Rows of ALL buffers are row_pitch pixels apart (>= w).  p NULL =
 * pt_temporal_defaults.  The scene's camera model (pt_scene_set_camera) is not consulted: the warp is the
 * pinhole's.  Asynchronous on `stream`; no scratch.
 *
 * Every operation is f32, rounded once, in the order written; fmaf where written and nowhere else; / and
 * sqrtf correctly rounded.  Per pixel (x, y), fn = (float)n:
 *  1. c_k = acc / fn, q_k = m2 / fn per channel; hits = alb.w;
 *     hits > 0: Ncur = geo.xyz / hits, Z = geo.w / hits; else Ncur = 0, Z = 0.  gbuf' = (Ncur, Z).
 *  2. With cur's W, H, inv_w, inv_h, aspect, focal, cam, M = cam_to_world (meta[28..43], column-major) and
 *     vhh = its view_half_h (pt_selftest_view_half_h), camera_ray's chain at the pixel's centre:
 *       norm_x = fmaf((float)x + 0.5f, inv_w, -0.5f);  norm_y = fmaf(((H - 1) - (float)y) + 0.5f, inv_h, -0.5f)
 *       vx = (vhh * aspect) * norm_x;  vy = vhh * norm_y;  pz = -focal
 *       p_k = fmaf(M[12+k], 1, fmaf(M[8+k], pz, fmaf(M[4+k], vy, M[k] * vx)))   k = 0..3
 *       d_k = p_k - cam[k];  len = sqrtf(fmaf(d_3, d_3, fmaf(d_2, d_2, fmaf(d_1, d_1, d_0 * d_0))))
 *       P_k = fmaf(Z, d_k / len, cam[k])   k = 0..2
 *  3. With prev's V = world_to_cam (meta[12..27], column-major), focal', aspect', vhh', cam':
 *       pc_k = fmaf(V[12+k], 1, fmaf(V[8+k], P_2, fmaf(V[4+k], P_1, V[k] * P_0)))   k = 0..2
 *       zc = -pc_2;  vx' = (pc_0 * focal') / zc;  vy' = (pc_1 * focal') / zc
 *       u = ((vx' / (vhh' * aspect')) + 0.5f) * W - 0.5f
 *       v = (H - 1) - (((vy' / vhh') + 0.5f) * H - 0.5f)
 *       e_k = P_k - cam'[k];  Ze = sqrtf(fmaf(e_2, e_2, fmaf(e_1, e_1, e_0 * e_0)))
 *  4. fu = floorf(u), fx = u - fu, x0 = (int)fu; likewise fv, fy, y0.  Taps (x0 + i, y0 + j), j = 0, 1
 *     outermost, i = 0, 1 inside, weight (i ? fx : 1 - fx) * (j ? fy : 1 - fy).  With (c_q, N_q) = hist_prev,
 *     q_q = mom_prev, (n_q, Z_q) = gbuf_prev at the tap, it is valid iff it lies inside the image and
 *       N_q > 0  &&  Z_q > 0  &&  |Z_q - Ze| <= depth_tol * Ze
 *           &&  (Ncur.x * n_q.x + Ncur.y * n_q.y) + Ncur.z * n_q.z >= normal_min
 *     For the valid taps in order: sw += wgt; sc += wgt * c_q; sq += wgt * q_q (per channel); sn += wgt * N_q.
 *  5. No history — c' = c_k, q' = q_k, N' = 1, a = 1 — unless ALL of: the previous set is given; Z > 0;
 *     zc > 0; u > -1 && u < W && v > -1 && v < H (tested in float before any conversion to an integer);
 *     sw > 1e-6f.  Every comparison is written so that a NaN means no history, or an invalid tap.
 *  6. Otherwise c_h = sc / sw, q_h = sq / sw, t = sn / sw + 1, N' = t < max_history ? t : max_history,
 *     r = 1 / N', a = alpha > r ? alpha : r,  c' = c_h + a * (c_k - c_h),  q' = q_h + a * (q_k - q_h).
 *     hist' = (c', N'), mom' = (q', 0).
 *  7. out = c';  d_c = q'_c - c'_c * c'_c, v_c = d_c > 0 ? d_c : 0;  var = (((v_r + v_g) + v_b) * a) / fn, a
 *     NaN stored as 0: the variance of the accumulated mean with 1 / a steps of n samples as the effective
 *     count.
 * Inputs are assumed finite; other inputs do not fault.  The result does not depend on the launch. */
int pt_reproject_async(pt_scene* scene, const float* d_accum, const float* d_m2, uint32_t n, const float* d_geo,
                       const float* d_alb, const float meta_cur[48], const float* meta_prev, const float* d_hist_prev,
                       const float* d_mom_prev, const float* d_gbuf_prev, uint32_t w, uint32_t h, size_t row_pitch,
                       const pt_temporal_params* p, float* d_hist, float* d_mom, float* d_gbuf, float* d_out, float* d_var,
                       void* stream);
/* The same on dense host buffers.  Blocking. */
int pt_reproject(pt_scene* scene, const float* accum, const float* m2, uint32_t n, const float* geo, const float* alb,
                 const float meta_cur[48], const float* meta_prev, const float* hist_prev, const float* mom_prev,
                 const float* gbuf_prev, uint32_t w, uint32_t h, const pt_temporal_params* p, float* hist, float* mom,
                 float* gbuf, float* out, float* var);

/* The state on the device between calls: two sets of the three planes for a w x h image, the previous
 * step's meta, and the step's working buffers, all counted in the scene's device_bytes while held.  One
 * history per camera path; calls on one scene stay in stream order, as for pt_denoise.  A history whose scene
 * was destroyed first has lost its buffers: every call on it but pt_history_destroy returns PT_ERR_INVALID. */
typedef struct pt_history pt_history;
int pt_history_create(pt_scene* scene, uint32_t w, uint32_t h, pt_history** hist_out);
int pt_history_reset(pt_history* hist); /* the next step is a first step */
void pt_history_destroy(pt_history* hist);
/* One step, in order: a moments render of frames frame0 + i*stride (i < nframes, nframes >= 1) of the whole
 * image of meta from zero; the guide buffers of frames frame0 .. frame0 + feature_frames - 1 (stride 1,
 * feature_frames >= 1); pt_reproject_async against the stored meta and planes (tparams NULL = the
 * defaults), after which the two sets swap; with dparams, pt_denoise_mean_async of the step's out and var on
 * the step's guides (dparams NULL: unfiltered); the device tone map with sample_runs = 1 of the filtered
 * (or accumulated) mean; the copies.  Outputs, all nullable, on the host: mean_out [h][w][3] and var_out
 * [h][w] the filtered (or accumulated) mean and its variance, rgba_out [h][w][4], history_len_out [h][w]
 * the new N.  counters: nullable, the render's plus the guide pass's.  meta's W, H must be the history's.
 * Blocking.  The sets swap only when the whole step has succeeded: a step that fails leaves the history as the
 * step before left it. */
int pt_history_step(pt_history* hist, const float meta[48], uint32_t frame0, uint32_t nframes, uint32_t frame_stride,
                    int max_depth, int mode, uint32_t feature_frames, const pt_temporal_params* tparams,
                    const pt_denoise_params* dparams, float* mean_out, float* var_out, uint8_t* rgba_out,
                    float* history_len_out, pt_counters* counters);

/* Ray queries: the traversal itself, for rays the caller supplies — what does this ray hit, is this
 * segment blocked.  The answers are the reference's intersect() (src/wgsl-util/intersection-logic.wgsl),
 * bit for bit, whatever kernel, grid or option computes them.
 *
 * The ray is (o, d) exactly as given: d is NOT normalised, and every t is in units of d — a ray with
 * d = target - o and tmax = 1 asks the visibility question between two points.  The traversal takes
 * inv = 1 / d per component by IEEE division (a zero component gives +-inf, as in the reference), and
 * the triangle test takes 1 / det by IEEE division too.  `reserved` is ignored (it need not be 0). */
typedef struct { float o[3]; float tmax; float d[3]; uint32_t reserved; } pt_ray;   /* 32 B */
typedef struct { float p[3]; float t;    float n[3]; int32_t  material; } pt_hit;   /* 32 B */

/* Closest hits.  For ray i, h = the reference's intersect(ray): its marker-stack order, its pruning of
 * a child whose box distance exceeds the closest t so far (the exit distance for an origin inside the
 * box: the reference's quirk, kept), a triangle taken on strict t < closest, so the first of equal t.
 *   h.intersected and h.t < tmax:  hits[i] = { p = o + t*d (one fma per component, as the reference's
 *       hit point), t, n = the shading normal (pt_scene_set_vertex_normals is honoured), material }
 *   otherwise (no hit, t >= tmax, or tmax NaN — the comparison is false):
 *       hits[i] = { p = 0, t = -1, n = 0, material = -1 }
 * tmax = +inf asks for the closest hit without a limit.  tmax only filters the REPORT; the traversal
 * and its counters are those of the unlimited query.
 * Counters (nullable, added to): ext_queries += n; nodes, tri_tests and box_tests the traversal's;
 * samples and shadow_queries untouched.
 * n = 0: PT_OK, nothing is touched.  n > 2^30, a null pointer with n > 0, or (the _async forms) d_rays
 * or d_hits not 16-byte aligned: PT_ERR_INVALID.  The _async forms take device pointers and run on
 * `stream`; a device-side failure of an earlier asynchronous call on the scene surfaces here as in
 * pt_render_async.  The blocking forms copy the rays in, run on the scene's own stream and copy the
 * results out (host buffers of any alignment the types allow); their device scratch belongs to the scene
 * (grown on demand, counted in device_bytes while held, freed by pt_scene_destroy).
 * A batch is traced in launches of at most 2^22 rays, in order on the stream.  Every wave of a launch
 * reaches an exit: one that is still tracing after option trace_watchdog iterations (default 2^24) or
 * 5 s of wall clock gives up, the call's results are invalid, later query launches of the scene skip,
 * and pt_scene_check or the next call on the scene reports PT_ERR_HIP (as for a traversal wave of a
 * render).  The limit is per launch, so it does not bound the batch: 2^22 rays in 5 s is 0.8 Mrays/s,
 * two orders of magnitude below the slowest rate measured. */
int pt_query_hits(pt_scene* scene, const pt_ray* rays, size_t n, pt_hit* hits, pt_counters* counters);
int pt_query_hits_async(pt_scene* scene, const pt_ray* d_rays, size_t n, pt_hit* d_hits, pt_counters* d_counters,
                        void* stream);

/* Occlusion.  occluded[i] = 1 iff the reference's intersect(ray i) reports a hit with t < tmax, else 0:
 * DEFINED by the closest-hit result above, COMPUTED with early exit.  During the reference's traversal
 * the closest t so far only decreases (a triangle replaces it on strict <).  So
 *   - if any triangle test of the traversal succeeds with t < tmax, the final closest t is < tmax: 1;
 *   - if none does, the traversal ends without a hit or with every accepted t >= tmax: 0.
 * A ray may therefore stop at its first successful test with t < tmax: up to that test its traversal is
 * the reference's (same order, same pruning), and the value is decided — whichever traversal flavour
 * runs.  With tmax = +inf the query stops at the first hit of any kind; tmax <= 0 or NaN never stops
 * early and gives 0.
 * Counters (nullable, added to): shadow_queries += n; nodes, tri_tests and box_tests what the shortened
 * traversals did (<= pt_query_hits' on the same rays); samples and ext_queries untouched.
 * Arguments and errors as pt_query_hits (occluded: n bytes, any alignment). */
int pt_query_occluded(pt_scene* scene, const pt_ray* rays, size_t n, uint8_t* occluded, pt_counters* counters);
int pt_query_occluded_async(pt_scene* scene, const pt_ray* d_rays, size_t n, uint8_t* d_occluded,
                            pt_counters* d_counters, void* stream);

/* The camera rays of a window (NULL = the whole image), w * h records, row-major: ray (y - y0) * w +
 * (x - x0) is the ray the render and pt_render_features trace for pixel (x, y) in frame `frame` — the
 * jittered pinhole ray of salt t = u32(f32(frame)), a unit direction — with tmax = +inf and
 * reserved = 0.  frame >= 2^24 is rejected, as everywhere.  d_rays: device memory, 16-byte aligned. */
int pt_camera_rays(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t frame, pt_ray* rays);
int pt_camera_rays_async(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t frame, pt_ray* d_rays,
                         void* stream);

/* Radiance queries: full paths from rays the caller supplies — how bright is it along this ray.  For
 * ray i and sample s, L(i, s) is the reference's radiance(ray, seed) (program-raymarch.wgsl:104-303),
 * bit for bit, whatever kernel, batch size or option computes it, called with
 *   ray.p = (o, 1), ray.d = (d, 0), d_inv = 1 / d per component by IEEE division;
 *   rr_prob, direct_only != 0 and max_depth from the params;
 *   seed_in = (int32)seeds[i] for s = 0, and (int32)hash1u(seeds[i] + s * 16787u) (u32 wrap) for s >= 1.
 * tmax and reserved of the ray are ignored.  pt_scene_set_vertex_normals is honoured.
 *   accum[3 i + c] += (L_c >= 0 ? L_c : 0)   for s = 0 .. nsamples - 1, in that order
 * — the render's rule, so calls compose as renders of frame ranges do; the caller divides by its total
 * sample count.  (Sample s >= 1 of a call is NOT sample 0 of a call with other seeds unless the caller
 * derives them by the rule above.)
 * Directions must be unit: the kernels are the render's, proved for the directions a render makes.  A
 * ray is ADMITTED iff q = fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x)) in f32 satisfies |q - 1| <= 2^-18
 * (a NaN q fails) — wider than any f32 normalisation leaves.  A ray that is not admitted
 * is never traced: it contributes exactly nothing — its three accumulator words keep their bits — and
 * adds to no counter.
 * Counters (nullable, added to): samples += admitted rays * nsamples; ext_queries, shadow_queries, nodes,
 * tri_tests and box_tests the paths' sums, with the render's exception (a cooperative big-leaf turn counts
 * by wave).
 * n = 0 or nsamples = 0: PT_OK, nothing is touched.  PT_ERR_INVALID: params NULL; n > 2^26 (one sample of
 * every ray must fit a wavefront batch); max_depth < 0 or > 1024 (the render's limit; -1 is NOT "default"
 * here); a null pointer with n > 0; and, in the _async form, d_rays not 16-byte aligned or d_seeds /
 * d_accum not 4-byte aligned.  rr_prob is taken as the render takes meta[45]: unchecked, a NaN included
 * (roulette then never ends a path and the throughput becomes NaN, as in the reference).
 * The call always runs the wavefront pipeline, in batches of whole samples of all n rays: option wf_paths
 * or the default target, never fewer than min(nsamples, 2) samples per batch while memory allows, halved
 * down to one sample per batch when the device is short of memory, then PT_ERR_NOMEM.  Options as for a
 * render, except kernel=mega|literal, regen and fuse_gen, which do not apply, and leaf_pre, whose default
 * (a probe from the render's camera) is off here: leaf_pre=1 turns the leaf pass on.
 * The blocking form copies rays, seeds and accum through scene-owned scratch (counted in device_bytes
 * while held) on the scene's own stream; the _async form takes device pointers.  Device-side failures and
 * the watchdog surface as in pt_render_async / pt_scene_check. */
typedef struct { float rr_prob; int32_t direct_only; int32_t max_depth; uint32_t nsamples; } pt_radiance_params;
int pt_query_radiance(pt_scene* scene, const pt_ray* rays, const uint32_t* seeds, size_t n,
                      const pt_radiance_params* params, float* accum, pt_counters* counters);
int pt_query_radiance_async(pt_scene* scene, const pt_ray* d_rays, const uint32_t* d_seeds, size_t n,
                            const pt_radiance_params* params, float* d_accum, pt_counters* d_counters, void* stream);

/* The radiance seeds of a window, laid out as pt_camera_rays lays out its rays and under its argument
 * rules: seeds[(y - y0) * w + (x - x0)] is the value the reference's main() hands to radiance() for pixel
 * (x, y) in frame `frame`.  So pt_camera_rays + pt_camera_seeds + pt_query_radiance(nsamples = 1, the
 * meta's rr_prob and direct_only) into a zeroed buffer equals pt_frame_window with negative components
 * clamped to 0, bit for bit.  d_seeds: device memory, 4-byte aligned. */
int pt_camera_seeds(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t frame, uint32_t* seeds);
int pt_camera_seeds_async(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t frame, uint32_t* d_seeds,
                          void* stream);

/* Irradiance gathers: lightmap texels and spherical-harmonic probes sampled on the device.  A radiance
 * query needs one direction per (point, sample) from the caller; a gather draws them itself, with the
 * reference's own samplers, and reduces the paths' radiance per point.  Every float operation below is
 * f32 and as written; an FMA appears only where fmaf is written.
 * Seeds.  For point i and sample s = sample0 .. sample0 + nsamples - 1:
 *   sd = s == 0 ? seed : hash1u(seed + s * 16787u)   (u32 wrap; the radiance queries' rule);
 *   the direction is drawn with sd; the path gets seed_in = (int32)hash1u(sd + 7u), the reference's own
 *   idiom for "the next decision".
 * PT_GATHER_COSINE.  nn = fmaf(n.z, n.z, fmaf(n.y, n.y, n.x * n.x)); the point is ADMITTED iff
 *   2^-80 <= nn <= 2^80 (a NaN fails).  nh = n / sqrt(nn) per component by IEEE division (the reference's
 *   normalize: the call normalises itself, since a normal off unit length by 2^-21 already pushes the
 *   generated direction to the admission band's edge).  The ray is the reference's
 *   sample_hemisphere((p, 1), (nh, 0), sd) (samplers.wgsl:15-46), origin fma(0.001, d, p) included: the
 *   reference's diffuse bounce from that point.  Its pdf is not used: the estimator's weight is pi.
 * PT_GATHER_SH9.  The normal is ignored and every point is admitted.  xi = hash2(sd * 7u + 11u);
 *   phi = (2 * 3.14159f) * xi[0]; z = fmaf(-2, xi[1], 1); r = sqrt(max(fmaf(-z, z, 1), 0)); (s, c) = the
 *   pinned sincos of phi; d = (r * c, r * s, z); the origin is p itself.
 * Sample admission.  Each generated direction takes pt_query_radiance's test (|q - 1| <= 2^-18).  A sample
 * or point that is not admitted is never traced, adds to no counter, and leaves every accumulator word it
 * would have touched with its bits unchanged (-0, NaN and infinities included).
 * The path.  L = the reference's radiance(ray, seed_in) with the params' rr_prob, direct_only != 0 and
 * max_depth, bit for bit; pt_scene_set_vertex_normals is honoured.  Lc = (L_c >= 0 ? L_c : 0).
 *   COSINE: accum[3 i + c] += Lc, in sample order; the irradiance is pi / N times the sum.
 *   SH9:    accum[27 i + 9 c + k] = fmaf(Lc, Y_k, accum[..]), in sample order, with
 *           Y0 = 0.282095f            Y1 = 0.488603f * y        Y2 = 0.488603f * z
 *           Y3 = 0.488603f * x        Y4 = 1.092548f * (x * y)  Y5 = 1.092548f * (y * z)
 *           Y6 = 0.315392f * fmaf(3 * z, z, -1)                 Y7 = 1.092548f * (x * z)
 *           Y8 = 0.546274f * fmaf(x, x, -(y * y));              the caller scales by 4 pi / N.
 * Composition.  Two calls over samples [0, a) and [a, b) equal one call over [0, b), bit for bit.
 * pt_gather_rays hands out sample `sample` of every point as pt_ray {o, +inf, d, 0} and seeds[i] =
 * hash1u(sd + 7u); a point or sample that is not admitted gets d = 0 (o = p) and seed 0, which
 * pt_query_radiance also rejects.  So pt_gather_rays + pt_query_radiance(nsamples = 1) over the samples
 * in order repeats a COSINE gather, bit for bit.
 * Counters (nullable, added to): as pt_query_radiance; samples += admitted samples.
 * n = 0 or nsamples = 0: PT_OK, nothing is touched.  PT_ERR_INVALID: params NULL; an unknown mode;
 * n > 2^26; sample0 + nsamples > 2^31 (pt_gather_rays: sample >= 2^31); max_depth < 0 or > 1024; a null
 * pointer with n > 0; and, in the _async forms, points or rays not 16-byte aligned, or accum / seeds not
 * 4-byte aligned.  rr_prob is unchecked, as in pt_query_radiance.
 * Batching, options, watchdog and the blocking form's scratch are pt_query_radiance's: always the
 * wavefront pipeline, whole samples of all n points per batch, leaf_pre off unless set to 1;
 * kernel=mega|literal, regen and fuse_gen do not apply. */
typedef struct { float p[3]; uint32_t seed; float n[3]; uint32_t reserved; } pt_gather_point; /* 32 B */
enum { PT_GATHER_COSINE = 0, PT_GATHER_SH9 = 1 };
typedef struct {
    float rr_prob; int32_t direct_only; int32_t max_depth;
    uint32_t sample0; uint32_t nsamples; uint32_t mode;
} pt_gather_params;
int pt_gather(pt_scene* scene, const pt_gather_point* pts, size_t n, const pt_gather_params* params, float* accum,
              pt_counters* counters);
int pt_gather_async(pt_scene* scene, const pt_gather_point* d_pts, size_t n, const pt_gather_params* params, float* d_accum,
                    pt_counters* d_counters, void* stream);
int pt_gather_rays(pt_scene* scene, const pt_gather_point* pts, size_t n, uint32_t mode, uint32_t sample, pt_ray* rays,
                   uint32_t* seeds);
int pt_gather_rays_async(pt_scene* scene, const pt_gather_point* d_pts, size_t n, uint32_t mode, uint32_t sample,
                         pt_ray* d_rays, uint32_t* d_seeds, void* stream);

/* Completion check of the asynchronous calls: waits for every render of the scene to finish
 * (blocking) and reports a device-side failure of any of them — a wavefront traversal wave that
 * gave up after its watchdog limit leaves a flag instead of hanging, and the accumulators of
 * that render are invalid — as PT_ERR_HIP with the wave's state in pt_last_error().  The flag is
 * cleared.  The blocking calls (pt_render, pt_frame, pt_render_image) check it themselves. */
int pt_scene_check(pt_scene* scene);

/* Explicit opt-in (no load-time side effect): ask HIP for `n` hardware queues per process by
 * setting GPU_MAX_HW_QUEUES, which the HIP runtime reads once, when it starts.  Call before any
 * HIP use in the process (the first pt_* call that touches a device starts it); afterwards it
 * has no effect and returns PT_ERR_INVALID.  Hosts that put many streams of their own beside the
 * wavefront's two part streams (e.g. torch) want 8 so the parts do not share a queue. */
int pt_set_hw_queues(int n);

/* Options (process-wide; the library reads no environment variable).  Every value renders the
 * same bits — the parity suite checks each — so they choose kernels and batch shapes only; the
 * defaults are the measured best.  value NULL = back to the default; unknown names and malformed
 * values fail with PT_ERR_INVALID.  Render calls read the options when they start.
 *   "kernel"        auto | mega | wavefront | literal    pipeline (auto = PT_MODE_* and the scene)
 *   "trav"          nested|flat1|pred|lean|lean2|lean4|lean8|lean16|lean32   traversal flavour
 *   "lds" "fastrcp" "dual" "fuse" "fuse_gen" "bf" "mailbox" "bf_stackless" "region_perm"
 *   "leaf_walk" "leaf_pool" "leaf_skip"                                     0 | 1 switches (default 1)
 *   "parts" "sort" "node_bias" "big_leaf" "bf_slots" "wf_paths" "wf_trace_blocks" "trace_sparse"
 *   "trace_ring" "trace_watchdog" "node_steps" "regen"                      integers
 *                                       (defaults: parts 2, sort 512, node_bias 4 / 1 by kernel
 *                                        instance (megakernel 8), big_leaf 128, bf_slots 8, wf_paths
 *                                        64 Mi, wf_trace_blocks 0 = by occupancy, trace_sparse 4,
 *                                        trace_ring 0 = by occupancy, trace_watchdog 2^24;
 *                                        node_steps 1..8: node steps per node turn of the lean
 *                                        traversal, default 4, megakernel 1; regen: camera batches
 *                                        per region admitted by every extension launch of the
 *                                        fused kernel, default 0 = off)
 *   "bf_narrow"     0 | 1               (default 1: scenes of <= 32 distinct entries and <= 32 internal
 *                                        nodes run the fused kernel's 32-bit instance — narrow sets and
 *                                        the replay's subtree pruning; 0 keeps the 64-bit one: tests)
 *   "step_addr64"   0 | 1               (default 0; 1: the fused kernel addresses its queues with 64-bit
 *                                        indices whatever the part's size, as parts beyond 4 GiB do: tests)
 *   "mb_uid_order"  forward | reverse   (read by pt_scene_create: uid numbering of mailbox scenes)
 *   "leaf_bvh"      integer             (read by pt_scene_create: leaves with a leaf BVH, >= this many entries)
 *   "pool_run"      2 | 4               (entries per run of the pooled leaf turns; default per scene)
 *   "leaf_pre"      0 | 1 | 2           (big leaves resolved before the traversal: never, always,
 *                                        2 = default: where the scene's probe finds it pays)
 *   "pre_ratio"     integer percent     (leaf_pre=2's bar: visited / filtered leaf work, default 50)
 *   "leaf_blocks" "leaf_pairs"          integers (the leaf pass's grid; its pair walk: 0 | 1 | 2)
 *   "leaf_refine"   0 | 1               (the pair walk's second check with the entries' normals)
 *   "reduce"        rccl | ordered      (pt_render_multi's reduction)
 *   "denoise_lds"   0 | 1 | 2 | 3 | 4   (pt_denoise_async: the first that many passes — steps 1, 2, 4, 8 — stage
 *                                        their block's (16 + 4 s)^2 region in LDS, the others load their taps
 *                                        from global memory; default 2, the measured best)
 *   "query_refill"  0 | 1               (pt_query_*: 1 = default, a lane that finishes its ray takes the next ray of
 *                                        its wave's window at once; 0: a wave takes new rays only when all its 64
 *                                        lanes are idle — the one-lane-per-pixel kernels' scheme, kept for A/B runs)
 *   "query_blocks"  integer             (pt_query_*: the grid in blocks of 4 waves; 0 = default, by occupancy and
 *                                        batch size; tests use 1 to make a small batch run many windows per wave)
 * DESIGN.md §6 describes each.  pt_get_option writes the current value ("" = default) into buf. */
int pt_set_option(const char* name, const char* value);
int pt_get_option(const char* name, char* buf, size_t cap);
void pt_reset_options(void);

/* Which instance of the fused step kernel this process launched last: 32 (option bf_narrow), 64, or
 * 0 (none yet, a counting instance, or the stack walk of bf_stackless=0).  For tests. */
int pt_last_bf_width(void);
/* How that launch addressed its queues: 32 (byte offsets of 32 bits: the default while a part's queue
 * arrays stay below 4 GiB), 64 (larger parts, or option step_addr64), or 0 (none yet).  For tests. */
int pt_last_step_addr(void);

/* Destroys the RCCL communicators pt_render_multi made (they are cached per device list; the
 * library also destroys them when the process exits).  Not concurrent with pt_render_multi. */
int pt_release_communicators(void);

/* Identity of the build: the SHA-256 of the sources it was compiled from (csrc/Makefile), so a
 * host can refuse a library that was not built from the tree it runs in. */
const char* pt_build_id(void);

/* Multi-GPU render of one image (the `n_gpus` of §8(b)): scenes[g] is the same
 * packed scene uploaded to device g (pt_scene_create per device, any devices, repeats allowed).
 * Frames k = frame0 + i*frame_stride (i < nframes) are dealt round-robin: scene g renders the i
 * with i % n == g (frame-interleaved: every device sees the same mix of path lengths), each into
 * an f32 accumulator on its own device (scenes[0]'s starts from accum, the others from zero), on
 * one host thread per device; the partial accumulators are then summed onto scenes[0]'s device
 * and copied to accum (host f32 [H][W][3], in/out).
 * Reduction (option "reduce"): "rccl" (default when the devices are distinct and
 * librccl.so.1 loads) = ONE ncclReduce(sum, f32) to device 0 over a communicator made once per
 * device list (ncclCommInitAll, single process) — the summation order is RCCL's; "ordered" (and
 * always with repeated devices) = peer copies added on device 0 in device order,
 * deterministic.  n == 1 is exactly pt_render (with option reduce=rccl: the render and a one-rank
 * RCCL communicator's reduce, the same bits).  counters: nullable, summed over devices.
 * Blocking; the scenes must not be in use by other calls meanwhile. */
int pt_render_multi(pt_scene* const* scenes, int n, const float meta[48], uint32_t frame0, uint32_t nframes,
                    uint32_t frame_stride, int max_depth, int mode, float* accum, pt_counters* counters);

/* One reference dispatch: radiance[H][W][3] = radiance() of every pixel for RNG salt t
 * (the resultMatrix of program-raymarch.wgsl:82-84, before host clamping). */
int pt_frame(pt_scene* scene, const float meta[48], uint32_t t, int max_depth, float* radiance);
int pt_frame_async(pt_scene* scene, const float meta[48], uint32_t t, int max_depth, float* d_radiance, void* stream);

/* pt_frame for a window: radiance is host f32 [h][w][3], the same bits as that rectangle of
 * pt_frame's result (the salt t and each pixel's seed are the full image's). */
int pt_frame_window(pt_scene* scene, const float meta[48], const pt_window* win, uint32_t t, int max_depth,
                    float* radiance);

/* Display transform of program-raymarch.ts:295-316 on the host (JS double semantics):
 * raw = acc/sample_runs, lum = mean(raw), out = raw * (lum/(lum+1))^0.01, u8 = ToInt32(out*255)
 * clamped; rgba[i*4+3] = 255. */
int pt_tonemap(const float* accum, size_t npix, uint32_t sample_runs, uint8_t* rgba_out);

/* The same display transform on the device (double, as the JS): d_accum f32 [npix][3] ->
 * d_rgba u8 [npix][4], asynchronous on `stream` (hipStream_t; NULL = default), on the scene's
 * device. */
int pt_tonemap_async(pt_scene* scene, const float* d_accum, size_t npix, uint32_t sample_runs, uint8_t* d_rgba,
                     void* stream);

/* The accumulator (or any n floats) from device memory to PINNED host memory, asynchronous on
 * `stream`: the reference maps its accumulation buffer back to the host after every frame
 * (program-raymarch.ts:262-293).  A copy kernel of a few blocks, so that a readback pipelined
 * with the next render holds few of its CU slots (the runtime's blit copy holds ~512 blocks for
 * the whole PCIe transfer).  Both pointers 16-byte aligned; h_dst must be page-locked
 * (hipHostMalloc / torch pin_memory), else PT_ERR_INVALID. */
int pt_readback_async(pt_scene* scene, const float* d_src, size_t n, float* h_dst, void* stream);

/* programEntry's result in one call: render frames frame0 + i*stride (i < nframes) into a
 * zeroed accumulator and return the displayed image (tone map with sample_runs = nframes)
 * as host RGBA u8 [H][W][4] — only the image crosses PCIe.  counters: nullable.  Blocking. */
int pt_render_image(pt_scene* scene, const float meta[48], uint32_t frame0, uint32_t nframes, uint32_t frame_stride,
                    int max_depth, int mode, uint8_t* rgba_out, pt_counters* counters);

/* Native BVH build (host only, no GPU): the reference's f64 builder
 * (src/ts-util/bvh.ts:14-188) and packer (src/packer.ts:83-137) in C++, byte-identical to them.
 * vertices: x,y,z per vertex in double — the values the host's JS holds after the CTM, not the
 * f32 copies in triangle_data; tris: (i0, i1, i2, material) per triangle, vertex indices
 * 1-based as in the OBJ.  Writes the packed bvh_data floats; *bvh_len = their count.  bvh_cap
 * = 0 asks for the size only; a smaller non-zero bvh_cap fails with PT_ERR_INVALID. */
int pt_bvh_build(const double* vertices, size_t vertex_count, const int32_t* tris, size_t tri_count, float* bvh_out,
                 size_t bvh_cap, size_t* bvh_len);

/* Fast BVH build (SURVEY.md §8(f) row 2's flagged mode; gives up topology parity with the
 * reference's builder): binned SAH over triangle centroids, each triangle in one leaf of at most 8
 * (depth-capped), tight child boxes, written in the same packed layout (src/packer.ts:83-137) so the
 * unchanged traversal runs on it.  Same arguments and size query as pt_bvh_build; fails with
 * PT_ERR_INVALID when the packed buffer would exceed 2^24 floats (offsets are stored as f32). */
int pt_bvh_build_sah(const double* vertices, size_t vertex_count, const int32_t* tris, size_t tri_count, float* bvh_out,
                     size_t bvh_cap, size_t* bvh_len);

/* pt_bvh_build_sah with the triangles of flagged materials (isolate_material[m] != 0 for material
 * id m < material_count; hosts flag the emitters, sum(Ke) > 0) in the root's left child — ONE leaf
 * however many they are, which the traversal tests whenever a ray meets its box (leaf children are
 * never pruned), so the exit-distance pruning of intersection-logic.wgsl:178-181 cannot hide the
 * lights — and the rest of the scene in its right child.  material_count = 0: exactly
 * pt_bvh_build_sah. */
int pt_bvh_build_sah2(const double* vertices, size_t vertex_count, const int32_t* tris, size_t tri_count,
                      const uint8_t* isolate_material, size_t material_count, float* bvh_out, size_t bvh_cap,
                      size_t* bvh_len);

/* ---------------------------------------------------------------------------------------------
 * The LBVH (SURVEY.md §8(f)'s fast mode beside SAH): a linear BVH over Morton keys, built from the
 * packed triangle_data alone — on the host by pt_bvh_build_lbvh, on the device by pt_scene_create_mesh.
 * Both write the SAME tree, byte for byte; the rules below define it without reference to how either
 * computes it.  f32 arithmetic throughout, every operation rounded once (no contraction), IEEE division.
 *
 * Input.  triangle_data as src/packer.ts:4-81 packs it: the 16-float header, nverts = tri[0] f32
 *   vertices from tri[2], the index records (i0, i1, i2, material) of all objects contiguous from tri[3]
 *   to tri[4], nobj = tri[1] materials of 15 floats from tri[4], vertex normals from tri[5].  Record r is
 *   the r-th group of four floats of the index section and T = (tri[4] - tri[3]) / 4 their count.  The
 *   header is checked as pt_scene_create checks it, and: tri[3] >= 16, tri[3] <= tri[4], the section a
 *   whole number of records, T >= 1.  A vertex index (1-based, read as WGSL i32(f32)) outside [1, nverts],
 *   a material outside [0, nobj), or a non-finite coordinate of a referenced vertex: PT_ERR_INVALID.
 * Order of floats.  Every min and max below is taken in the total order of the finite floats in which
 *   -0 < +0 (so neither depends on the order of evaluation); NaN coordinates of vertices no record
 *   references are skipped.
 * Flagged materials.  Material m is an emitter when Ke.x + Ke.y + Ke.z > 0, summed in f32 from left to
 *   right (the Node host's rule, program-raymarch.wgsl:136).  With isolate_emitters set and both flagged
 *   and unflagged records present, the root's left child is ONE leaf of all flagged records in record
 *   order and its right child the tree over the rest (pt_bvh_build_sah2's convention and reason).
 *   Otherwise the tree is over all records.
 * Keys.  lo, hi: min and max over all vertices of the vertex section; they are also the outer bounds
 *   bvh[0..5], unpadded.  Per record and axis: c = (mn + mx) * 0.5f of its three vertices' box;
 *   ext = hi - lo; inv = ext > 0 ? 1024.0f / ext : 0.0f; x = (c - lo) * inv;
 *   q = x >= 0 ? (uint32_t)fminf(x, 1023.0f) : 0   (a NaN x, from inf * 0, gives 0);
 *   morton = spread(qx) << 2 | spread(qy) << 1 | spread(qz), spread moving bit k to bit 3k;
 *   key = (uint64_t)morton << 32 | r.  Keys are unique, so their sorted order is unique.
 * Topology.  The binary radix tree of the sorted keys of the records the tree is over: for sorted
 *   positions [a, b], a < b, let p = clz64(key[a] ^ key[b]); the split is after the largest s in [a, b)
 *   with clz64(key[a] ^ key[s]) > p (clz64(0) = 64); the left child is [a, s], the right [s + 1, b].
 * Leaves.  The tree's top node has depth 1; under an emitter root the radix root has depth 2.  A radix
 *   node of at most max_leaf records (1..8) whose parent holds more than max_leaf is a leaf of its records
 *   in sorted order (an emitter root always counts as such a parent).  A radix node at depth PT_LBVH_MAX_DEPTH is
 *   a leaf whatever it holds, so max_stack <= PT_LBVH_MAX_DEPTH - 1 stays below the device stack.  If the
 *   whole tree would be one leaf of n records, the root gets two leaves instead, the first n / 2 records
 *   and the rest, each with the box of all n (pt_bvh_build_sah's rule; n = 1: an empty left leaf, zero box).
 * Boxes.  A child's box is the min and max of the f32 vertices of the records below it, then moved one
 *   f32 ulp outward on every axis (nextafterf towards -inf / +inf).  An empty child keeps zeros.
 * Packed form.  src/packer.ts:83-137 as pt_bvh_build_sah writes it: bounds, then pre-order nodes of 17
 *   floats, the left child at o + 17: (0, 0, o + 17, right offset, -2, left box, right box); a leaf is
 *   (1, 0, -1, -1, 4n), twelve zeros, then its records' four floats as triangle_data holds them.
 * --------------------------------------------------------------------------------------------- */
#define PT_LBVH_MAX_DEPTH 28
typedef struct {
    uint32_t max_leaf;          /* 1..8 */
    uint32_t isolate_emitters;  /* 0 | 1 */
    uint32_t profile;           /* 0 | 1: pt_scene_create_mesh times its kernels as if pt_profile_enable(scene, 1) had
                                   been called before the build — pt_profile_read then gives the time per stage
                                   ("k_build_bounds", "_keys", "_sort", "_karras", "_depth", "_level", "_offsets",
                                   "_emit"; a stage's launches share its name) — and leaves the timing enabled */
    uint32_t reserved;          /* 0 */
} pt_build_params;              /* 16 B */
/* max_leaf 4, isolate_emitters 1, profile 0. */
int pt_build_defaults(pt_build_params* params);

/* The LBVH above, built on the host (no GPU) top-down from its definition.  params NULL = the defaults;
 * max_leaf outside 1..8, isolate_emitters or profile > 1 (profile is ignored here) or the reserved word set:
 * PT_ERR_INVALID.  Size query and
 * 2^24-float limit as pt_bvh_build_sah. */
int pt_bvh_build_lbvh(const float* triangle_data, size_t triangle_len, const pt_build_params* params, float* bvh_out,
                      size_t bvh_cap, size_t* bvh_len);

/* A scene from the mesh alone: triangle_data is uploaded once and the LBVH above, its device records
 * (nodes, triangle records, vertex normals) and its packed form are built ON THE DEVICE; materials and the
 * light table, O(objects + emitters), on the host as pt_scene_create makes them (a mesh without emissive
 * triangles is PT_ERR_INVALID here).  No 2^24-float limit.  The scene is a traversal scene: no mailbox,
 * replay tree, leaf chunks, leaf pass or leaf remainders — the configuration options leaf_skip=0 and
 * leaf_bvh=0 run on a packed scene — so even a Cornell box made this way runs k_wf_trace, not the fused
 * step kernel; small scenes build on the host in microseconds and pt_scene_create remains their route.
 * Every render, query and gather call takes the scene as any other.  params as pt_bvh_build_lbvh. */
int pt_scene_create_mesh(const float* triangle_data, size_t triangle_len, const pt_build_params* params, int device,
                         pt_scene** scene_out);
/* The packed tree of a scene made by pt_scene_create_mesh (size query as pt_bvh_build): what
 * pt_bvh_build_lbvh returns for the same input.  PT_ERR_INVALID for a scene made by pt_scene_create, and
 * at or above 2^24 floats, where the format's f32 offsets stop being exact. */
int pt_scene_export_bvh(pt_scene* scene, float* bvh_out, size_t bvh_cap, size_t* bvh_len);

/* Kernel timing (no counterpart in the reference, which has no GPU timing): while enabled,
 * every kernel the scene launches is bracketed by two HIP events on the launch stream (no
 * synchronisation, a few microseconds per launch).  enable != 0 also discards earlier
 * records.  pt_profile_read waits for the recorded events and writes per-kernel totals
 * (at most max_entries; *n_out = entries written). */
int pt_profile_enable(pt_scene* scene, int enable);
/* Record only the launches of one kernel ("k_wf_trace", ...; NULL = all, the default): fewer
 * events in the stream when only one kernel's duration is wanted. */
int pt_profile_select(pt_scene* scene, const char* kernel);
int pt_profile_read(pt_scene* scene, pt_kernel_time* out, int max_entries, int* n_out);

/* Numerics self-test: out[i] = f(a[i], b[i]) evaluated ON THE DEVICE with the core's
 * pinned f32 math (fn ids: 0 sin, 1 cos, 2 tan, 3 acos, 4 log2, 5 exp2, 6 pow, 7 sqrt,
 * 8 div, 9 hash1u, 10 hash1, 11 hash2.x, 12 hash2.y, 13 min, 14 max; hash inputs are the
 * bit patterns of a[i]).  15 ray_inv: a holds n / 3 triples (x, y, z) and out their 1 / x, 1 / y, 1 / z from
 * the fused kernel's ray_inv, triple i on thread i — a wave votes on 64 consecutive triples (b unused). */
int pt_selftest_math(int device, int fn, const float* a, const float* b, float* out, size_t n);

/* Exhaustive self-test of the core's division-free reciprocal (pt_math.h rcp_rn, used by the
 * triangle test for 1/det): compares it with IEEE 1.0f/x on the device for every float x whose
 * magnitude bit pattern lies in [lo_bits, hi_bits] (< 0x80000000), both signs.  steps: Newton
 * steps (0..2), -1 = the core's own.  *mismatches = number of differing results;
 * *failing_bits = one failing input (nullable). */
int pt_selftest_rcp(int device, int steps, uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches,
                    uint32_t* failing_bits);

/* VALU issue calibration: `reps` timed launches (after one untimed) of a kernel whose threads run 8
 * independent v_fma_f32 chains (packed 1: v_pk_fma_f32, two FMAs per lane each; 2: packed and plain
 * chains interleaved 1 : 2; 32 instructions
 * per iteration, `iters` iterations, no memory operation) at 8 waves per SIMD — the SIMDs issue VALU
 * at their peak rate.  *ms_out = the timed launches' event time; *fma_wave_instr_out (nullable) =
 * their FMA wave-instructions.  Profiled with rocprofv3 PMC it pins the counter formula for the
 * fraction of VALU issue (scripts/calibrate_valu.sh). */
int pt_selftest_valu(int device, int iters, int reps, int packed, double* ms_out, uint64_t* fma_wave_instr_out);

/* Leaf chunks (option leaf_bvh, read by pt_scene_create: leaves of at least that many entries,
 * default 128, 0 = none): leaf `leaf`'s first record, entries and chunks.
 * PT_ERR_INVALID past the last one. */
int pt_scene_leaf_bvh(const pt_scene* scene, int leaf, int32_t* first_record, int32_t* entries, int32_t* nodes);

/* Leaf chunk stress test: nrays rays of family `mode` (0 near the leaf's entries, uniform
 * directions; 1 aimed at them; 2 grazing their planes; 3 leaving their surfaces), each tested
 * against chunked leaf `leaf` by the reference's sequential loop over all entries and by the
 * chunk scheme the traversal uses, with the same closest-t-so-far.  out (host, nrays x 6): loop
 * (position taken or -1, t bits), chunks (position or -1, t bits), entries tested and chunks
 * opened.  mode + 4: the same families through the walk that several rays parked at one leaf share
 * (chunk_leaf_multi), out columns 4-5 zero.  mode 16 + (method << 2 | family): `leaf` indexes the
 * scene's leaves the leaf pass can resolve (the 8 largest; PT_ERR_INVALID past the last) and the
 * pass's own code resolves them — method 0 resolve_leaf one ray per lane, 1 resolve_leaf 8 rays per
 * wave, 2 the (ray, chunk) pair walk without its second check, 3 with it (methods 2-3 need the
 * leaf's pass chunks: PT_ERR_INVALID without) — out columns 2-3 = its key as (position or -1, t
 * bits), 4-5 zero.  Blocking. */
int pt_selftest_leaf(pt_scene* scene, int leaf, int mode, uint32_t seed, uint32_t nrays, int32_t* out);

/* Light sampling self-test: the shade code's sample_area_lights ON THE DEVICE for n caller-supplied
 * (seeds[i], points[3i..3i+2]): the direction from the point to the sampled point of the emissive
 * triangle the seed draws.  out (host, n x 4 f32): the direction, then the bit pattern of the int32
 * slot k = i32(hash1(seed * 7 + 11) * Ntri) it read, 0 <= k <= Ntri (k == Ntri, when hash1 is exactly
 * 1, is the reference's out-of-range branch resolved with clamped reads).  Blocking. */
int pt_selftest_lights(pt_scene* scene, const uint32_t* seeds, const float* points, size_t n, float* out);

/* Camera self-test, host only (needs no device): out[i] = the view_half_h = 2 * focal * tan(vfov / 2)
 * that every render, frame, feature and camera-ray call derives ON THE HOST from metas[48 i ..
 * 48 i + 47] (meta[2] and meta[3]; the kernels take it as a uniform), for n meta blocks.  The blocks
 * pass the same checks as a render's (meta[0..1] integral resolutions). */
int pt_selftest_view_half_h(const float* metas, size_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif /* PT_HIP_H */
