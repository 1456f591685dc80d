#!/usr/bin/env node
'use strict';
// pt-render: the reference's browser entry (src/index.ts) as a CLI.  Loads the .ini,
// renders samplesPerPixel frames on the GPU, writes the tone-mapped PNG to IO.output
// (relative to --out-root, default cwd).  Usage: pt-render.js <scene.ini> [--web-root DIR]
// [--out-root DIR] [--max-depth D] [--mode auto|megakernel|wavefront] [--device N] [--spp N]
// [--vertex-normals 1] (smooth shading from the OBJ normals: the reference's commented-out branch)
// [--counters 1] (work counters in the JSON line; runs the kernels' counting builds)
// [--window x0,y0,w,h] (render and write only that rectangle of the image: the crop of the full PNG)
// [--window "x0,y0,w,h;x0,y0,w,h;..."] (several disjoint rectangles, rendered in one pass: the PNG keeps the
//  image's size, the rectangles hold the full PNG's pixels and everything else is black)
// [--denoise [iters]] (the variance-guided a-trous denoiser, pt_render_denoised_image: 1..5 passes, default the
//  library's; the whole image only, without --counters, --spp at least 2) [--feature-frames N] (frames of its guide buffers, default 4)
// [--pick x,y] (print what the frame-0 camera ray of pixel (x, y) hits — point, distance, normal, material —
//  as one JSON line and render nothing: pt_camera_rays + pt_query_hits)
// [--irradiance x,y,z,nx,ny,nz] [--probe x,y,z] [--samples N] [--seed S] (print, as one JSON line, what pt_gather
//  collects at that point and render nothing: --irradiance the cosine-weighted irradiance at a surface point
//  with normal n (any length), pi / N times the gather's sums; --probe the 27 SH9 radiance coefficients of a
//  probe, 4 pi / N times the sums, channel c's coefficient k at 9 c + k; N = --samples, default 256)
// [--camera thinlens|ortho|equirect] [--aperture R] [--focus-distance F] (a lens camera evaluated on the device,
//  pt_scene_set_camera: jittered like the pinhole, thinlens with depth of field from a lens of radius R (default 0)
//  focused at distance F (default |focus - position| of the scene's camera); combines with --window, the rectangle
//  list, --denoise and --counters; --dump-accum FILE writes the accumulator, 3 f32 per pixel, before the tone map)
// [--projection pinhole|equirect|ortho] (pinhole: the render above, the default.  The other two trace rays made
//  here through pt_query_radiance, the whole image only, one ray per pixel through its centre (u, v) = ((x + 0.5) / W,
//  (y + 0.5) / H), with the camera's axes R, U, B = columns 0..2 of cam_to_world (look L = -B) and its position P:
//    equirect  the full sphere: azimuth phi = (u - 0.5) 2 pi about U from L, elevation th = (0.5 - v) pi;
//              d = cos th (sin phi R + cos phi L) + sin th U, from P
//    ortho     d = L from P + (u - 0.5) a h R + (0.5 - v) h U, h = 2 tan(heightangle / 2) |focus - P| (what the pinhole
//              sees in the plane through the focus), a = W / H
//  all in doubles, then unitRays' f32 normalisation.  Seeds: pixel index i = x + y W has seed hash1u(hash1u(i * 16787))
//  for its sample 0 and, the library's rule, hash1u(seed + s * 16787) for sample s of --spp, frame after frame.)
//  (--camera ortho|equirect renders these projections on the device, jittered, with every other option.)
// [--turntable N[,cols]] (N cameras — the scene's own position rotated about the axis through its focus along its up,
//  in N equal steps, step 0 the scene's camera — rendered in ONE renderViews call (pt_render_views) into a contact
//  sheet of `cols` tiles per row (default ceil(sqrt(N))), which is the PNG; combines with --camera, --counters 1 and
//  --dump-accum FILE (the sheet's accumulator); not with --window, --denoise or --projection)
// [--turntable N[,cols] --temporal [alpha]] (the N views rendered IN ORDER through one history, pt_history_step: view k
//  takes the next --spp frames (frames k spp .. k spp + spp - 1) and starts from what the views before it accumulated,
//  reprojected into its camera; alpha in (0, 1] is the blend's floor, default the library's 0.2.  The sheet holds the
//  accumulated tiles, with --denoise [iters] [--feature-frames N] filtered by the a-trous denoiser on each view's guides;
//  not with --window, --counters 1, --camera, --projection or --dump-accum)
// [--bvh device] (no tree is built or packed here: the scene builds the linear BVH of include/pt_hip.h on the GPU from
//  the mesh alone, pt_scene_create_mesh; every other option as usual)
// [--dump-rays FILE] (with equirect or ortho: the rays, 8 f32 each, then the seeds, one u32 each, as made)
// [--dump-accum FILE] (with equirect or ortho: the accumulator, 3 f32 per pixel, before the tone map)
const fs = require('fs');
const path = require('path');
const host = require('..');

async function main(argv) {
    const args = { _: [] };
    for (let i = 0; i < argv.length; i++) {
        if ((argv[i] === '--denoise' || argv[i] === '--temporal') && (i + 1 >= argv.length || argv[i + 1].startsWith('--'))) args[argv[i].slice(2)] = '';
        else if (argv[i].startsWith('--')) args[argv[i].slice(2).replace(/-/g, '_')] = argv[++i];
        else args._.push(argv[i]);
    }
    if (!args._.length) { console.error('usage: pt-render.js <scene.ini> [options]'); process.exit(2); }
    if (args.bvh !== undefined && args.bvh !== 'device') { console.error('usage: pt-render.js <scene.ini> --bvh device'); process.exit(2); }
    let window = null, rects = null;
    if (args.window !== undefined) {
        try {
            const list = String(args.window).split(';').map((one) => {
                const parts = one.split(',');
                if (!parts.every((v) => /^\d+$/.test(v))) throw Error(`--window ${args.window}`);
                return host.check_window(parts.map(Number));
            });
            if (list.length > 1) rects = list;
            else window = list[0];
        } catch (e) {
            console.error(`usage: pt-render.js <scene.ini> --window x0,y0,w,h[;x0,y0,w,h...] (four non-negative integers, w and h at least 1): ${e.message}`);
            process.exit(2);
        }
    }
    let denoise = null;
    if (args.denoise !== undefined || args.feature_frames !== undefined) {
        const it = args.denoise === undefined || args.denoise === '' ? '0' : String(args.denoise);
        const ff = args.feature_frames === undefined ? '4' : String(args.feature_frames);
        if (args.denoise === undefined || !/^\d+$/.test(it) || !/^\d+$/.test(ff) || (it !== '0' && !(+it >= 1 && +it <= 5)) ||
            (args.denoise !== '' && it === '0') || !(+ff >= 1 && +ff <= 0xffffffff) || window || rects || args.counters === '1') {
            console.error('usage: pt-render.js <scene.ini> --denoise [iters] [--feature-frames N] (iters 1..5, N at least 1; ' +
                          `not with --window or --counters 1): --denoise ${args.denoise} --feature-frames ${args.feature_frames}`);
            process.exit(2);
        }
        denoise = { iters: +it, featureFrames: +ff };
    }
    let temporal = null;
    if (args.temporal !== undefined) {
        const a = args.temporal === '' ? undefined : Number(args.temporal);
        if (args.turntable === undefined || (a !== undefined && !(/^[0-9.eE+-]+$/.test(String(args.temporal)) && a > 0 && a <= 1)) ||
            window || rects || args.counters === '1' || args.camera !== undefined || args.projection !== undefined || args.dump_accum !== undefined) {
            console.error('usage: pt-render.js <scene.ini> --turntable N[,cols] --temporal [alpha] (alpha in (0, 1]; with --turntable only, ' +
                          `not with --window, --counters 1, --camera, --projection or --dump-accum): --temporal ${args.temporal}`);
            process.exit(2);
        }
        temporal = { alpha: a };
    }
    let turntable = null;
    if (args.turntable !== undefined) {
        const parts = String(args.turntable).split(',');
        if (parts.length < 1 || parts.length > 2 || !parts.every((v) => /^\d+$/.test(v)) || !(+parts[0] >= 1 && +parts[0] <= 65536) ||
            (parts.length > 1 && !(+parts[1] >= 1)) || window || rects || (denoise && !temporal) || args.projection !== undefined) {
            console.error('usage: pt-render.js <scene.ini> --turntable N[,cols] (N in 1..65536, cols at least 1; ' +
                          `not with --window or --projection, with --denoise only under --temporal): --turntable ${args.turntable}`);
            process.exit(2);
        }
        turntable = { n: +parts[0], cols: parts.length > 1 ? +parts[1] : undefined };
    }
    if (args.pick !== undefined) return pick(args);
    if (args.irradiance !== undefined || args.probe !== undefined) return gather(args);
    const projection = args.projection === undefined ? 'pinhole' : String(args.projection);
    if (!['pinhole', 'equirect', 'ortho'].includes(projection) ||
        (projection !== 'pinhole' && (window || rects || denoise || args.counters === '1'))) {
        console.error(`usage: pt-render.js <scene.ini> --projection pinhole|equirect|ortho (equirect and ortho: the whole image, ` +
                      `not with --window, --denoise or --counters 1): --projection ${args.projection}`);
        process.exit(2);
    }
    if (projection !== 'pinhole') return project(args, projection);
    const models = { thinlens: 'thin_lens', thin_lens: 'thin_lens', ortho: 'ortho', equirect: 'equirect' };
    const num = (v) => (v === undefined ? undefined : Number(v));
    if ((args.camera !== undefined && !models[args.camera]) || (args.camera === undefined && (args.aperture !== undefined || args.focus_distance !== undefined)) ||
        [args.aperture, args.focus_distance].some((v) => v !== undefined && !Number.isFinite(Number(v)))) {
        console.error(`usage: pt-render.js <scene.ini> --camera thinlens|ortho|equirect [--aperture R] [--focus-distance F]: ` +
                      `--camera ${args.camera} --aperture ${args.aperture} --focus-distance ${args.focus_distance}`);
        process.exit(2);
    }
    const t0 = Date.now();
    const s = host.load_scene_from_ini(args._[0], { web_root: args.web_root, quiet: true, bvh: args.bvh === 'device' ? 'device' : undefined });
    if (args.spp) s.scene_description.Settings.samplesPerPixel = parseInt(args.spp);
    let camera = null;
    if (args.camera !== undefined) {
        const focus = s.camera_data.focus.toArray(), pos = s.camera_data.pos.toArray();
        const dist = Math.hypot(focus[0] - pos[0], focus[1] - pos[1], focus[2] - pos[2]);
        camera = { model: models[args.camera], lensRadius: num(args.aperture) || 0, focusDistance: args.focus_distance === undefined ? dist : num(args.focus_distance) };
    }
    if (turntable && temporal) return turnTemporal(args, s, turntable, temporal, denoise, t0);
    if (turntable) return turn(args, s, turntable, camera, t0);
    const t1 = Date.now();
    const r = await host.programEntry(s.screenDimension, s.primitive_data, s.camera_data, s.scene_description, {
        device: parseInt(args.device || '0'), maxDepth: parseInt(args.max_depth || '16'), mode: args.mode || 'auto',
        vertexNormals: args.vertex_normals === '1', counters: args.counters === '1', window, rects, denoise, camera,
    });
    const t2 = Date.now();
    const [W, H] = window ? [window[2], window[3]] : s.screenDimension;
    const out = path.join(args.out_root || '.', s.scene_description.IO.output || 'out.png');
    fs.mkdirSync(path.dirname(out), { recursive: true });
    fs.writeFileSync(out, host.encode_png(r.rgba, W, H));
    if (args.dump_accum && r.accum) fs.writeFileSync(args.dump_accum, Buffer.from(r.accum.buffer, r.accum.byteOffset, r.accum.byteLength));
    const samples = (rects ? rects.reduce((a, w) => a + w[2] * w[3], 0) : W * H) * r.sample_runs;
    console.log(JSON.stringify({ output: out, width: W, height: H, window, rects, camera, spp: r.sample_runs, scene_ms: t1 - t0,
        denoise, render_ms: t2 - t1, msamples_per_s: samples / ((t2 - t1) / 1000) / 1e6, counters: r.counters }));
}
// --turntable N[,cols]: N metas from make_meta, one renderViews call, the contact sheet as the PNG
async function turn(args, s, turntable, camera, t0) {
    const [W, H] = s.screenDimension;
    const spp = s.scene_description.Settings.samplesPerPixel;
    const cams = host.turntable_cameras(s.camera_data, turntable.n);
    const { dsts, atlasW, atlasH } = host.view_atlas(cams.map(() => [W, H]), turntable.cols);
    const views = cams.map((c, k) => ({ meta: host.make_meta(s.screenDimension, c, s.scene_description, 0), camera, dst: dsts[k], frame0: 0 }));
    const t1 = Date.now();
    const pt = host.native();
    const scene = host.scene_of(pt, s.primitive_data[0], parseInt(args.device || '0'));
    let r;
    try {
        if (args.vertex_normals === '1') pt.sceneSetVertexNormals(scene, true);
        r = await host.renderViews(scene, views, { atlasW, atlasH, nframes: spp, stride: 1, maxDepth: parseInt(args.max_depth || '16'),
            mode: args.mode || 'auto', counters: args.counters === '1' });
    } finally {
        pt.sceneDestroy(scene);
    }
    const t2 = Date.now();
    const rgba = new Uint8ClampedArray(atlasW * atlasH * 4);
    pt.tonemap(r.accum, spp, rgba);
    const out = path.join(args.out_root || '.', s.scene_description.IO.output || 'out.png');
    fs.mkdirSync(path.dirname(out), { recursive: true });
    fs.writeFileSync(out, host.encode_png(rgba, atlasW, atlasH));
    if (args.dump_accum) fs.writeFileSync(args.dump_accum, Buffer.from(r.accum.buffer, r.accum.byteOffset, r.accum.byteLength));
    console.log(JSON.stringify({ output: out, width: atlasW, height: atlasH, turntable: turntable.n, tile: [W, H], dsts, camera, spp,
        scene_ms: t1 - t0, render_ms: t2 - t1, msamples_per_s: W * H * turntable.n * spp / ((t2 - t1) / 1000) / 1e6, counters: r.counters }));
}
// --turntable N[,cols] --temporal [alpha]: the N views in order through one history, the accumulated tiles as the sheet
async function turnTemporal(args, s, turntable, temporal, denoise, t0) {
    const [W, H] = s.screenDimension;
    const spp = s.scene_description.Settings.samplesPerPixel;
    const cams = host.turntable_cameras(s.camera_data, turntable.n);
    const { dsts, atlasW, atlasH } = host.view_atlas(cams.map(() => [W, H]), turntable.cols);
    const t1 = Date.now();
    const pt = host.native();
    const scene = host.scene_of(pt, s.primitive_data[0], parseInt(args.device || '0'));
    const rgba = new Uint8ClampedArray(atlasW * atlasH * 4);
    let history = null;
    try {
        if (args.vertex_normals === '1') pt.sceneSetVertexNormals(scene, true);
        history = host.historyCreate(scene, W, H);
        cams.forEach((c, k) => {
            const r = host.historyStep(history, host.make_meta(s.screenDimension, c, s.scene_description, 0), {
                frame0: k * spp, nframes: spp, maxDepth: parseInt(args.max_depth || '16'), mode: args.mode || 'auto',
                featureFrames: denoise ? denoise.featureFrames : Math.min(4, spp),
                params: temporal.alpha === undefined ? null : { alpha: temporal.alpha }, denoise });
            const [dx, dy] = dsts[k];
            for (let y = 0; y < H; ++y) rgba.set(r.rgba.subarray(4 * y * W, 4 * (y + 1) * W), 4 * ((dy + y) * atlasW + dx));
        });
    } finally {
        if (history) host.historyDestroy(history);
        pt.sceneDestroy(scene);
    }
    const t2 = Date.now();
    const out = path.join(args.out_root || '.', s.scene_description.IO.output || 'out.png');
    fs.mkdirSync(path.dirname(out), { recursive: true });
    fs.writeFileSync(out, host.encode_png(rgba, atlasW, atlasH));
    console.log(JSON.stringify({ output: out, width: atlasW, height: atlasH, turntable: turntable.n, tile: [W, H], dsts, temporal, denoise, spp,
        scene_ms: t1 - t0, render_ms: t2 - t1, msamples_per_s: W * H * turntable.n * spp / ((t2 - t1) / 1000) / 1e6 }));
}
// hash.wgsl's hash1u in u32 arithmetic
function hash1u(n) {
    n = ((n << 13) ^ n) >>> 0;
    return ((Math.imul(n, (Math.imul(Math.imul(n, n), 15731) + 789221) | 0) + 1376312589) >>> 0) & 0x7fffffff;
}
// --projection equirect|ortho: the rays and seeds the header documents, through queryRadiance
function project(args, projection) {
    const t0 = Date.now();
    const s = host.load_scene_from_ini(args._[0], { web_root: args.web_root, quiet: true, bvh: args.bvh === 'device' ? 'device' : undefined });
    if (args.spp) s.scene_description.Settings.samplesPerPixel = parseInt(args.spp);
    const [W, H] = s.screenDimension;
    const spp = s.scene_description.Settings.samplesPerPixel;
    const meta = host.make_meta(s.screenDimension, s.camera_data, s.scene_description, 0);
    const M = meta.subarray(28, 44), P = [meta[4], meta[5], meta[6]];
    const R = [M[0], M[1], M[2]], U = [M[4], M[5], M[6]], L = [-M[8], -M[9], -M[10]];
    const focus = s.camera_data.focus.toArray(), pos = s.camera_data.pos.toArray();
    const dist = Math.hypot(focus[0] - pos[0], focus[1] - pos[1], focus[2] - pos[2]);
    const h = 2 * Math.tan(s.camera_data.heightangle * Math.PI / 360) * dist, a = W / H;
    const o = new Float64Array(3 * W * H), d = new Float64Array(3 * W * H), seeds = new Uint32Array(W * H);
    for (let y = 0; y < H; ++y) {
        for (let x = 0; x < W; ++x) {
            const i = x + y * W, u = (x + 0.5) / W, v = (y + 0.5) / H;
            for (let c = 0; c < 3; ++c) {
                if (projection === 'equirect') {
                    const phi = (u - 0.5) * 2 * Math.PI, th = (0.5 - v) * Math.PI;
                    o[3 * i + c] = P[c];
                    d[3 * i + c] = Math.cos(th) * (Math.sin(phi) * R[c] + Math.cos(phi) * L[c]) + Math.sin(th) * U[c];
                } else {
                    o[3 * i + c] = P[c] + (u - 0.5) * a * h * R[c] + (0.5 - v) * h * U[c];
                    d[3 * i + c] = L[c];
                }
            }
            seeds[i] = hash1u(hash1u(Math.imul(i, 16787) >>> 0));
        }
    }
    const rays = host.unitRays(o, d);
    const t1 = Date.now();
    const pt = host.native();
    const scene = host.scene_of(pt, s.primitive_data[0], parseInt(args.device || '0'));
    let accum;
    try {
        if (args.vertex_normals === '1') pt.sceneSetVertexNormals(scene, true);
        accum = host.queryRadiance(scene, rays, seeds, { nsamples: spp, maxDepth: parseInt(args.max_depth || '16'), rr: meta[45], directOnly: meta[46] > 0 });
    } finally {
        pt.sceneDestroy(scene);
    }
    const t2 = Date.now();
    const rgba = new Uint8Array(W * H * 4);
    pt.tonemap(accum, spp, rgba);
    const out = path.join(args.out_root || '.', s.scene_description.IO.output || 'out.png');
    fs.mkdirSync(path.dirname(out), { recursive: true });
    fs.writeFileSync(out, host.encode_png(rgba, W, H));
    const bytes = (ta) => Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength);
    if (args.dump_rays) fs.writeFileSync(args.dump_rays, Buffer.concat([bytes(rays), bytes(seeds)]));
    if (args.dump_accum) fs.writeFileSync(args.dump_accum, bytes(accum));
    console.log(JSON.stringify({ output: out, width: W, height: H, projection, spp, scene_ms: t1 - t0, render_ms: t2 - t1,
        msamples_per_s: W * H * spp / ((t2 - t1) / 1000) / 1e6 }));
}
// --pick x,y: what the camera ray of pixel (x, y), frame 0, hits (pt_camera_rays + pt_query_hits), as one
// JSON line; nothing is rendered or written.  `bits`: the eight 32-bit words of the hit record.
function pick(args) {
    const parts = String(args.pick).split(',');
    if (parts.length !== 2 || !parts.every((v) => /^\d+$/.test(v))) {
        console.error(`usage: pt-render.js <scene.ini> --pick x,y (two non-negative integers): --pick ${args.pick}`);
        process.exit(2);
    }
    const [x, y] = parts.map(Number);
    const s = host.load_scene_from_ini(args._[0], { web_root: args.web_root, quiet: true, bvh: args.bvh === 'device' ? 'device' : undefined });
    const [W, H] = s.screenDimension;
    if (x >= W || y >= H) { console.error(`--pick ${x},${y}: outside the ${W}x${H} image`); process.exit(2); }
    const pt = host.native();
    const meta = host.make_meta(s.screenDimension, s.camera_data, s.scene_description, 0);
    const scene = host.scene_of(pt, s.primitive_data[0], parseInt(args.device || '0'));
    try {
        if (args.vertex_normals === '1') pt.sceneSetVertexNormals(scene, true);
        const ray = host.cameraRays(scene, meta, 0, [x, y, 1, 1]);
        const h = host.queryHits(scene, ray);
        const material = new Int32Array(h.buffer, h.byteOffset, 8)[7];
        console.log(JSON.stringify({ pick: [x, y], width: W, height: H, hit: material >= 0,
            ray: { o: Array.from(ray.subarray(0, 3)), d: Array.from(ray.subarray(4, 7)) },
            p: Array.from(h.subarray(0, 3)), t: h[3], n: Array.from(h.subarray(4, 7)), material,
            bits: Array.from(new Uint32Array(h.buffer, h.byteOffset, 8)) }));
    } finally {
        pt.sceneDestroy(scene);
    }
}
// --irradiance x,y,z,nx,ny,nz | --probe x,y,z: one gather point through pt_gather, scaled, as one JSON line
function gather(args) {
    const probe = args.probe !== undefined, text = String(probe ? args.probe : args.irradiance);
    const v = text.split(',').map(Number), ns = args.samples === undefined ? 256 : Number(args.samples);
    const seed = args.seed === undefined ? 1 : Number(args.seed);
    if (v.length !== (probe ? 3 : 6) || !v.every(Number.isFinite) || !(Number.isInteger(ns) && ns >= 1 && ns <= 0x7fffffff) ||
        !(Number.isInteger(seed) && seed >= 0 && seed <= 0xffffffff) || (args.probe !== undefined && args.irradiance !== undefined)) {
        console.error('usage: pt-render.js <scene.ini> --irradiance x,y,z,nx,ny,nz | --probe x,y,z [--samples N] [--seed S]: ' + text);
        process.exit(2);
    }
    const s = host.load_scene_from_ini(args._[0], { web_root: args.web_root, quiet: true, bvh: args.bvh === 'device' ? 'device' : undefined });
    const meta = host.make_meta(s.screenDimension, s.camera_data, s.scene_description, 0);
    const pt = host.native();
    const scene = host.scene_of(pt, s.primitive_data[0], parseInt(args.device || '0'));
    try {
        if (args.vertex_normals === '1') pt.sceneSetVertexNormals(scene, true);
        const points = host.gatherPoints(v.slice(0, 3), probe ? [0, 0, 0] : v.slice(3, 6), [seed]);
        const sums = host.gather(scene, points, { nsamples: ns, mode: probe ? 'sh9' : 'cosine', maxDepth: parseInt(args.max_depth || '16'),
            rr: meta[45], directOnly: meta[46] > 0 });
        const k = (probe ? 4 : 1) * Math.PI / ns;
        const scaled = Array.from(sums, (x) => x * k);
        console.log(JSON.stringify(probe ? { probe: v, samples: ns, seed, sh9: scaled }
                                         : { irradiance: scaled, point: v.slice(0, 3), normal: v.slice(3, 6), samples: ns, seed }));
    } finally {
        pt.sceneDestroy(scene);
    }
}

main(process.argv.slice(2)).catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
