'use strict';
// Node host of the MI355X path-tracing core.  Same module surface as the reference's
// TypeScript host (src/index.ts, src/packer.ts, src/ts-util/*.ts, src/program-raymarch.ts),
// with programEntry rendering through the HIP core (N-API addon -> libpt_hip.so).
const { parse_ini_file, ini_file_to_ini_scene } = require('./lib/parse-ini');
const { parse_obj } = require('./lib/parse-obj');
const { BVH } = require('./lib/bvh');
const { pack_scene_object_group, pack_bvh } = require('./lib/packer');
const { mat4_rot_axis, bounds_of_vec3, chunk_into_3, bounds_bounds_intersection_3d, bounds_surface_area } = require('./lib/math');
const geometry = require('./lib/geometry');
const { xml2js } = require('./lib/xml');
const scene = require('./lib/scene');
const { programEntry, make_meta, check_window, check_rects, MODE, renderViews, view_atlas, turntable_cameras, scene_of } = require('./lib/program-entry');
const { encode_png } = require('./lib/png');
const addon = require('./lib/addon');

// Ray queries on a native scene handle (native().sceneCreate): rays are 8 floats each — origin, tmax,
// direction (not normalised; t is in its units), reserved — in one Float32Array.
//   queryHits(scene, rays) -> Float32Array[8n]: (p.xyz, t, n.xyz, material as int32 bits) of the closest hit
//       with t < tmax; a miss is t = -1, material = -1, p = n = 0
//   queryOccluded(scene, rays) -> Uint8Array[n]: 1 where the closest hit lies below tmax (early exit)
//   cameraRays(scene, meta, frame, window?) -> Float32Array[8 w h]: the rays the render traces for the
//       window's pixels ([x0, y0, w, h], default the whole image) in that frame, tmax = +Infinity
const queryHits = (scene, rays) => addon.load().queryHits(scene, rays);
const queryOccluded = (scene, rays) => addon.load().queryOccluded(scene, rays);
const cameraRays = (scene, meta, frame, window) => addon.load().cameraRays(scene, meta, frame, check_window(window));
// Radiance queries: full paths from the caller's rays (unit directions: unitRays makes them).
//   queryRadiance(scene, rays, seeds, { nsamples = 1, maxDepth = 8, rr = 0.9, directOnly = false, accum }) ->
//       Float32Array[3n]: per ray the clamped radiance of nsamples paths, summed (onto a copy of accum if given);
//       seeds: Uint32Array[n], the seed of sample 0 (sample s >= 1 takes hash1u(seed + s * 16787)); a ray whose
//       |d|^2 is further than 2^-18 from 1 is not traced and adds nothing
//   cameraSeeds(scene, meta, frame, window?) -> Uint32Array[w h]: the seeds the render hands to its paths there;
//       with cameraRays and queryRadiance({ nsamples: 1 }) they repeat that frame of the render
//   unitRays(o, d) -> Float32Array[8n]: rays with d normalised in f32 (o, d: arrays of 3n numbers)
const queryRadiance = (scene, rays, seeds, params = {}) => {
    const { nsamples = 1, maxDepth = 8, rr = 0.9, directOnly = false, accum = null } = params;
    return addon.load().queryRadiance(scene, rays, seeds, nsamples, maxDepth, rr, !!directOnly, accum);
};
const cameraSeeds = (scene, meta, frame, window) => addon.load().cameraSeeds(scene, meta, frame, check_window(window));
const unitRays = (o, d) => {
    const n = Math.floor(d.length / 3), rays = new Float32Array(8 * n), v = new Float32Array(3), f = Math.fround;
    for (let i = 0; i < n; ++i) {
        // scaled by a power of two so that no square overflows, then the reference's normalize in f32: the
        // squares and sums are taken in doubles and rounded to f32 after each step, as one fused multiply-add is
        const m = Math.max(Math.abs(d[3 * i]), Math.abs(d[3 * i + 1]), Math.abs(d[3 * i + 2]));
        const k = m > 0 && isFinite(m) ? Math.pow(2, -Math.floor(Math.log2(m))) : 1;
        for (let c = 0; c < 3; ++c) v[c] = d[3 * i + c] * k;
        const len = f(Math.sqrt(f(v[2] * v[2] + f(v[1] * v[1] + f(v[0] * v[0])))));
        rays.set([o[3 * i], o[3 * i + 1], o[3 * i + 2], Infinity, f(v[0] / len), f(v[1] / len), f(v[2] / len), 0], 8 * i);
    }
    return rays;
};
// Irradiance gathers: the directions are drawn on the device (include/pt_hip.h pt_gather).
//   gatherPoints(p, n, seeds) -> Float32Array[8k]: pt_gather_point records from 3k coordinates, 3k normal
//       components (any admitted length; ignored by 'sh9') and k uint32 seeds
//   gather(scene, points, { nsamples, sample0 = 0, mode = 'cosine' | 'sh9', maxDepth = 8, rr = 0.9, directOnly = false,
//       accum }) -> Float32Array[3k | 27k]: per point the clamped radiance of samples sample0 .. sample0 + nsamples - 1,
//       summed ('cosine': irradiance = pi / N times it) or weighted by the nine SH basis values of the direction
//       ('sh9': coefficient j of channel c at 9 c + j, scale by 4 pi / N), onto a copy of accum if given
//   gatherRays(scene, points, sample, mode = 'cosine') -> { rays, seeds }: that sample of every point as the
//       inputs of queryRadiance({ nsamples: 1 })
const GATHER_MODES = ['cosine', 'sh9'];
const gatherMode = (mode) => {
    const m = typeof mode === 'string' ? GATHER_MODES.indexOf(mode) : mode;
    if (m !== 0 && m !== 1) throw new TypeError(`gather mode must be 'cosine' or 'sh9', not ${mode}`);
    return m;
};
const gatherPoints = (p, n, seeds) => {
    const k = seeds.length, out = new Float32Array(8 * k), bits = new Uint32Array(out.buffer);
    if (p.length !== 3 * k || n.length !== 3 * k) throw new TypeError('gatherPoints(p[3k], n[3k], seeds[k])');
    for (let i = 0; i < k; ++i) {
        out.set([p[3 * i], p[3 * i + 1], p[3 * i + 2]], 8 * i);
        out.set([n[3 * i], n[3 * i + 1], n[3 * i + 2]], 8 * i + 4);
        bits[8 * i + 3] = seeds[i];
    }
    return out;
};
const gather = (scene, points, params = {}) => {
    const { nsamples = 1, sample0 = 0, mode = 'cosine', maxDepth = 8, rr = 0.9, directOnly = false, accum = null } = params;
    return addon.load().gather(scene, points, nsamples, sample0, gatherMode(mode), maxDepth, rr, !!directOnly, accum);
};
const gatherRays = (scene, points, sample = 0, mode = 'cosine') => addon.load().gatherRays(scene, points, sample, gatherMode(mode));

// Temporal accumulation (include/pt_hip.h pt_reproject, pt_denoise_mean, pt_history_*): the history of a pixel's
// surface point carried across a camera move.  params: null (the library's defaults) or any of { alpha, normalMin,
// depthTol, maxHistory } over them (0.2, 0.9, 0.1, 64).
//   reproject(scene, { accum, m2, n, geo, alb, meta }, prev = null, params = null) -> { meta, hist, mom, gbuf, out, var }:
//       one step from an n-frame moments render and its guide sums; prev: null or an earlier step's result
//   denoiseMean(scene, c, var, w, h, geo, alb, { featureFrames = 4, iters = 0 }) -> { out, var }: the a-trous filter on a
//       given mean and variance of the mean (reproject's out and var)
//   historyCreate(scene, w, h) -> history; historyReset(history); historyDestroy(history)
//   historyStep(history, meta, { frame0 = 0, nframes, stride = 1, maxDepth = 16, mode = 'auto', featureFrames = 4,
//       params = null, denoise = null | true | { iters } }) -> { mean, var, rgba, historyLen }: render, guides,
//       reprojection against the previous step, optionally the filter, the tone map
const temporalParams = (p) => {
    if (p === null || p === undefined) return null;
    const known = ['alpha', 'normalMin', 'depthTol', 'maxHistory'];
    for (const k of Object.keys(p)) if (!known.includes(k)) throw new TypeError(`temporal params: unknown field ${k}`);
    const { alpha = 0.2, normalMin = 0.9, depthTol = 0.1, maxHistory = 64 } = p;
    const v = [alpha, normalMin, depthTol, maxHistory];
    if (!v.every((x) => typeof x === 'number' && Number.isFinite(x)) || !(alpha > 0 && alpha <= 1) || !(depthTol > 0) || !(maxHistory >= 1))
        throw new RangeError('temporal params: alpha in (0, 1], normalMin finite, depthTol > 0, maxHistory >= 1');
    return Float32Array.from(v);
};
const reproject = (scene, step, prev = null, params = null) => {
    const r = addon.load().reproject(scene, step.accum, step.m2, step.n, step.geo, step.alb, step.meta, prev ? prev.meta : null,
        prev ? prev.hist : null, prev ? prev.mom : null, prev ? prev.gbuf : null, temporalParams(params));
    r.meta = Float32Array.from(step.meta);
    return r;
};
const denoiseMean = (scene, c, variance, w, h, geo, alb, params = {}) => {
    const { featureFrames = 4, iters = 0 } = params;
    return addon.load().denoiseMean(scene, c, variance, w, h, geo, alb, featureFrames, iters);
};
const historyCreate = (scene, w, h) => addon.load().historyCreate(scene, w, h);
const historyReset = (history) => addon.load().historyReset(history);
const historyDestroy = (history) => addon.load().historyDestroy(history);
const historyStep = (history, meta, options = {}) => {
    const { frame0 = 0, nframes, stride = 1, maxDepth = 16, mode = 'auto', featureFrames = 4, params = null, denoise = null } = options;
    const m = typeof mode === 'number' ? mode : MODE[mode];
    if (m === undefined) throw new TypeError(`historyStep: unknown mode ${mode}`);
    const iters = denoise === null || denoise === undefined || denoise === false ? -1 : (denoise === true ? 0 : (denoise.iters || 0));
    return addon.load().historyStep(history, meta, frame0, nframes, stride, maxDepth, m, featureFrames, temporalParams(params), iters);
};

module.exports = {
    parse_ini_file, ini_file_to_ini_scene, parse_obj, BVH, pack_scene_object_group, pack_bvh,
    mat4_rot_axis, bounds_of_vec3, chunk_into_3, bounds_bounds_intersection_3d, bounds_surface_area,
    Vertex: geometry.Vertex, Bounds: geometry.Bounds, xml2js,
    parse_scene_xml: scene.parse_scene_xml, pack_primitive: scene.pack_primitive,
    screen_dimension: scene.screen_dimension, load_scene_from_ini: scene.load_scene_from_ini,
    load_scene_xml_file: scene.load_scene_xml_file,
    programEntry, make_meta, check_window, check_rects, MODE, encode_png, native: addon.load, scene_of,
    renderViews, view_atlas, turntable_cameras,
    queryHits, queryOccluded, cameraRays, queryRadiance, cameraSeeds, unitRays,
    gather, gatherRays, gatherPoints,
    reproject, denoiseMean, historyCreate, historyStep, historyReset, historyDestroy,
};
