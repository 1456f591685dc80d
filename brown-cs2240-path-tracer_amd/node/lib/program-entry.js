'use strict';
// programEntry counterpart (src/program-raymarch.ts:50-357) on the HIP core.
//   * meta block: program-raymarch.ts:55-92 (48 f32, layout SURVEY.md §8a A2)
//   * scene buffers: pt_scene_create replaces the storage buffers of :109-131
//   * render_loop (:226-335): all spp frames in one device call (or `chunk`-sized calls
//     reporting progress), t_k = k instead of the wall-clock ms, host accumulation moved
//     onto the device; the display transform (:295-316) is `tonemap`.
const { camera_matrices } = require('./geometry');
const { load } = require('./addon');

const MODE = { auto: 0, megakernel: 1, wavefront: 2 };

/** program-raymarch.ts:55-92 */
function make_meta(screenDimension, camera_data, scene_description, time_elapsed) {
    const [W, H] = screenDimension;
    const screen_dimension_inv = [1 / W, 1 / H];
    const camera_position = camera_data.pos;
    const camera_look = camera_data.focus.sub_v(camera_position).normalize();
    const FOV = camera_data.heightangle;
    const focal_length = 1;
    const aspect_ratio = W / H;
    const { world_to_cam, cam_to_world } = camera_matrices(camera_position, camera_look, camera_data.up);
    const s = scene_description.Settings;
    return new Float32Array([
        W, H, focal_length, FOV * Math.PI / 180, ...camera_position.toArray(), 1,
        ...screen_dimension_inv, aspect_ratio, time_elapsed || 0,
        ...world_to_cam, ...cam_to_world,
        s.samplesPerPixel, s.pathContinuationProb, s.directLightingOnly ? 1 : -1, 0,
    ]);
}

/** [x0, y0, w, h] as four non-negative integers (w, h >= 1), else an Error; null/undefined: none */
function check_window(window) {
    if (window === undefined || window === null) return null;
    if (!Array.isArray(window) || window.length !== 4 || !window.every((v) => Number.isInteger(v) && v >= 0 && v <= 0xffffffff) ||
        window[2] < 1 || window[3] < 1)
        throw Error(`window must be [x0, y0, w, h] (non-negative integers, w and h at least 1), not ${JSON.stringify(window)}`);
    return window.slice();
}

/** [[x0, y0, w, h], ...]: a non-empty list of windows (the library checks them against the image and for
 *  overlaps), else an Error; null/undefined: none */
function check_rects(rects) {
    if (rects === undefined || rects === null) return null;
    if (!Array.isArray(rects) || rects.length < 1) throw Error(`rects must be a non-empty list of [x0, y0, w, h], not ${JSON.stringify(rects)}`);
    return rects.map((r) => {
        try { return check_window(r || []); } catch (e) { throw Error('rects: ' + e.message); }
    });
}

/** The native scene of one packed primitive: from its tree (sceneCreate), or — bvh_data null or absent, as
 *  load_scene_* leaves it under bvh 'device' — built on the device from the mesh alone (sceneCreateMesh;
 *  build = {maxLeaf, isolateEmitters} over the library's defaults). */
function scene_of(pt, primitive, device, build) {
    return primitive.bvh_data ? pt.sceneCreate(primitive.triangle_data, primitive.bvh_data, device)
                              : pt.sceneCreateMesh(primitive.triangle_data, build || null, device);
}

/**
 * programEntry(screenDimension, primitive_data, camera_data, scene_description, options?)
 *   -> Promise<{accum: Float32Array(W*H*3), sample_runs, rgba: Uint8ClampedArray(W*H*4), counters, scene_info}>
 * options: {device=0, devices=[...] (several GPUs: pt_render_multi), maxDepth=16, mode='auto', frame0=0, chunk=spp,
 *           onFrames(done, total), imageOnly=false,
 *           build={maxLeaf=4, isolateEmitters=true} (a primitive without bvh_data: its tree is built on the device),
 *           vertexNormals=false (the reference's commented-out smooth-normal branch; changes results),
 *           camera={model: 'thin_lens'|'ortho'|'equirect'|'pinhole', lensRadius=0, focusDistance=1} (a lens camera
 *           evaluated on the device, pt_scene_set_camera: combines with every other option),
 *           counters=false (work counters: the kernels' counting builds, slower; counters is null without),
 *           window=[x0, y0, w, h] (render that rectangle of the image only: accum is w*h*3 and rgba w*h*4, the
 *           crop of the windowless result — every pixel's samples and its tone map are the full image's; not
 *           with imageOnly or several devices),
 *           rects=[[x0, y0, w, h], ...] (render those disjoint rectangles of the image only, all in one pass per
 *           chunk (pt_render_rects): accum and rgba stay the full image's size, the rectangles hold the windowless
 *           result's pixels and everything else is black; not with window, imageOnly or several devices),
 *           denoise={iters=0 (the library's default), featureFrames=4} (the displayed image through the
 *           variance-guided a-trous denoiser, pt_render_denoised_image: returns only {rgba, ...} like imageOnly;
 *           samplesPerPixel >= 2; one device call, so not with window, rects, counters, imageOnly, chunk,
 *           onFrames or several devices: each of those combinations is an Error)}
 * imageOnly: render and tone-map on the device in one call and return only {rgba, counters, ...}
 * (no accumulator crosses PCIe; pt_render_image).
 * As in the reference only primitive_data[0] is rendered (program-raymarch.wgsl:31,33).
 */
async function programEntry(screenDimension, primitive_data, camera_data, scene_description, options) {
    const o = Object.assign({ device: 0, maxDepth: 16, mode: 'auto', frame0: 0 }, options || {});
    const pt = load();
    const [W, H] = screenDimension;
    const meta = make_meta(screenDimension, camera_data, scene_description, 0);
    const mode = typeof o.mode === 'number' ? o.mode : MODE[o.mode];
    if (mode === undefined) throw Error(`unknown mode ${o.mode}`);
    const win = check_window(o.window);
    if (win && (o.imageOnly || (o.devices && o.devices.length > 1))) throw Error('window: not with imageOnly or several devices');
    const rects = check_rects(o.rects);
    if (rects && (win || o.imageOnly || (o.devices && o.devices.length > 1))) throw Error('rects: not with window, imageOnly or several devices');
    if (o.denoise && (win || rects || o.counters || o.imageOnly || o.chunk || o.onFrames || (o.devices && o.devices.length > 1)))
        throw Error('denoise: not with window, rects, counters, imageOnly, chunk, onFrames or several devices');
    if (o.devices && o.devices.length > 1) return programEntryMulti(pt, meta, W, H, primitive_data, scene_description, o, mode);
    const scene = scene_of(pt, primitive_data[0], o.devices && o.devices.length ? o.devices[0] : o.device, o.build);
    // the scene's device memory (scene + wavefront state) is released when the call ends, not
    // when V8 happens to collect the handle
    try {
        if (o.vertexNormals) pt.sceneSetVertexNormals(scene, true);
        if (o.camera) pt.sceneSetCamera(scene, o.camera);
        const spp = scene_description.Settings.samplesPerPixel;
        const chunk = Math.max(1, o.chunk || spp);
        const scene_info = pt.sceneInfo(scene);
        if (o.denoise) {
            const d = Object.assign({ iters: 0, featureFrames: 4 }, o.denoise === true ? {} : o.denoise);
            const rgba = new Uint8ClampedArray(W * H * 4);
            pt.renderDenoised(scene, meta, o.frame0, spp, 1, o.maxDepth, mode, d.featureFrames, d.iters, new Uint8Array(rgba.buffer));
            return { accum: null, sample_runs: spp, rgba, counters: null, scene_info, denoise: d };
        }
        if (o.imageOnly) {
            const rgba = new Uint8ClampedArray(W * H * 4);
            const c = await pt.renderImage(scene, meta, o.frame0, spp, 1, o.maxDepth, mode, new Uint8Array(rgba.buffer),
                                           !!o.counters);
            return { accum: null, sample_runs: spp, rgba, counters: c, scene_info };
        }
        const npix = win ? win[2] * win[3] : W * H;
        const accum = new Float32Array(npix * 3);
        const counters = { samples: 0, ext_queries: 0, shadow_queries: 0, nodes: 0, tri_tests: 0, box_tests: 0 };
        for (let done = 0; done < spp; done += chunk) {
            const n = Math.min(chunk, spp - done);
            const c = rects ? await pt.renderRects(scene, meta, null, rects, o.frame0 + done, n, 1, o.maxDepth, mode, accum, !!o.counters)
                    : win ? await pt.renderWindow(scene, meta, win, o.frame0 + done, n, 1, o.maxDepth, mode, accum, !!o.counters)
                          : await pt.render(scene, meta, o.frame0 + done, n, 1, o.maxDepth, mode, accum, !!o.counters);
            if (c) for (const k of Object.keys(counters)) counters[k] += c[k];
            if (o.onFrames) o.onFrames(done + n, spp);
        }
        const rgba = new Uint8ClampedArray(npix * 4);
        pt.tonemap(accum, spp, rgba);
        return { accum, sample_runs: spp, rgba, counters: o.counters ? counters : null, scene_info, window: win, rects };
    } finally {
        pt.sceneDestroy(scene);
    }
}

// options.devices = [d0, d1, ...]: the scene on every device, frames dealt round-robin and the
// partial accumulators reduced onto d0 (pt_render_multi: RCCL over xGMI for distinct devices)
async function programEntryMulti(pt, meta, W, H, primitive_data, scene_description, o, mode) {
    const scenes = [];
    try {
        for (const d of o.devices) scenes.push(scene_of(pt, primitive_data[0], d, o.build));
        if (o.vertexNormals) for (const s of scenes) pt.sceneSetVertexNormals(s, true);
        if (o.camera) for (const s of scenes) pt.sceneSetCamera(s, o.camera);
        const spp = scene_description.Settings.samplesPerPixel;
        const scene_info = pt.sceneInfo(scenes[0]);
        const accum = new Float32Array(W * H * 3);
        const counters = await pt.renderMulti(scenes, meta, o.frame0, spp, 1, o.maxDepth, mode, accum, !!o.counters);
        if (o.onFrames) o.onFrames(spp, spp);
        const rgba = new Uint8ClampedArray(W * H * 4);
        pt.tonemap(accum, spp, rgba);
        return { accum, sample_runs: spp, rgba, counters: o.counters ? counters : null, scene_info, devices: o.devices.slice() };
    } finally {
        for (const s of scenes) pt.sceneDestroy(s);
    }
}

/** A shelf packing of rectangles [[w, h], ...] in list order: rows of `cols` rectangles (default ceil(sqrt(n))), each
 *  row as tall as its tallest -> { dsts: [[x, y], ...], atlasW, atlasH } (pt_amd.view_atlas's rule) */
function view_atlas(sizes, cols) {
    if (!Array.isArray(sizes) || sizes.length < 1) throw Error('views: the list is empty (n must be at least 1)');
    const per = cols === undefined || cols === null ? Math.ceil(Math.sqrt(sizes.length)) : cols;
    if (!Number.isInteger(per) || per < 1) throw Error(`cols must be a positive integer, not ${cols}`);
    const dsts = [];
    let x = 0, y = 0, rowH = 0, atlasW = 0;
    sizes.forEach(([w, h], k) => {
        if (k && k % per === 0) { x = 0; y += rowH; rowH = 0; }
        dsts.push([x, y]);
        x += w;
        rowH = Math.max(rowH, h);
        atlasW = Math.max(atlasW, x);
    });
    return { dsts, atlasW, atlasH: y + rowH };
}

/**
 * renderViews(scene, views, {atlasW, atlasH, nframes, stride=1, maxDepth=16, mode='auto', accum, counters=false})
 *   -> Promise<{accum: Float32Array(atlasH*atlasW*3), counters, atlasW, atlasH, dsts}>
 * Many images of one native scene handle (native().sceneCreate) in ONE pass through the pipeline
 * (pt_render_views): views = [{meta: Float32Array(48), window: [x0, y0, w, h] (default: the image), camera:
 * {model, lensRadius, focusDistance} (default: the pinhole), dst: [x, y], frame0 = 0}, ...].  View v's window lands at
 * dst in the atlas accumulator (given, in/out; default zeros) and holds the bits render / renderWindow give under
 * sceneSetCamera(camera).  Without atlasW, atlasH and any dst the views are packed by view_atlas.
 */
async function renderViews(scene, views, options) {
    const o = Object.assign({ stride: 1, maxDepth: 16, mode: 'auto', counters: false }, options || {});
    if (!Array.isArray(views) || views.length < 1) throw Error('views must be a non-empty list of {meta, window, camera, dst, frame0}');
    const mode = typeof o.mode === 'number' ? o.mode : MODE[o.mode];
    if (mode === undefined) throw Error(`unknown mode ${o.mode}`);
    const list = views.map((v, k) => {
        if (!v || !(v.meta instanceof Float32Array) || v.meta.length < 48) throw Error(`views[${k}]: meta must be a Float32Array of 48`);
        const window = check_window(v.window) || [0, 0, v.meta[0], v.meta[1]];
        return { meta: v.meta, window, camera: v.camera || undefined, dst: v.dst, frame0: v.frame0 || 0 };
    });
    let { atlasW, atlasH } = o;
    const packed = list.every((v) => v.dst === undefined || v.dst === null) && atlasW === undefined && atlasH === undefined;
    if (packed) {
        const a = view_atlas(list.map((v) => [v.window[2], v.window[3]]));
        a.dsts.forEach((d, k) => { list[k].dst = d; });
        ({ atlasW, atlasH } = a);
    }
    if (!Number.isInteger(atlasW) || !Number.isInteger(atlasH) || atlasW < 1 || atlasH < 1 || list.some((v) => !Array.isArray(v.dst)))
        throw Error('views: give every view a dst and the call atlasW and atlasH, or none of them');
    const accum = o.accum || new Float32Array(atlasW * atlasH * 3);
    const counters = await load().renderViews(scene, list, atlasW, atlasH, o.nframes, o.stride, o.maxDepth, mode, accum, !!o.counters);
    return { accum, counters, atlasW, atlasH, dsts: list.map((v) => v.dst.slice()) };
}

/** N cameras on a turntable: the camera's position rotated about the axis through `focus` along `up`, in N equal
 *  steps of 2 pi / N (Rodrigues' formula in doubles); step 0 is camera_data itself */
function turntable_cameras(camera_data, n) {
    const P = camera_data.pos.toArray(), C = camera_data.focus.toArray(), U = camera_data.up.toArray();
    const ul = Math.hypot(U[0], U[1], U[2]);
    const k = U.map((v) => v / ul), r = P.map((v, c) => v - C[c]);
    const Vertex = camera_data.pos.constructor;
    const out = [camera_data];
    for (let s = 1; s < n; ++s) {
        const th = 2 * Math.PI * s / n, cs = Math.cos(th), sn = Math.sin(th);
        const kr = k[0] * r[0] + k[1] * r[1] + k[2] * r[2];
        const x = [k[1] * r[2] - k[2] * r[1], k[2] * r[0] - k[0] * r[2], k[0] * r[1] - k[1] * r[0]];
        const p = r.map((v, c) => C[c] + v * cs + x[c] * sn + k[c] * kr * (1 - cs));
        out.push({ focus: camera_data.focus, heightangle: camera_data.heightangle, up: camera_data.up, pos: new Vertex(p[0], p[1], p[2]) });
    }
    return out;
}

module.exports = { programEntry, make_meta, check_window, check_rects, MODE, renderViews, view_atlas, turntable_cameras, scene_of };
