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
const { programEntry, make_meta, check_window, check_rects, MODE } = require('./lib/program-entry');
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

module.exports = {
    parse_ini_file, ini_file_to_ini_scene, parse_obj, BVH, pack_scene_object_group, pack_bvh,
    mat4_rot_axis, bounds_of_vec3, chunk_into_3, bounds_bounds_intersection_3d, bounds_surface_area,
    Vertex: geometry.Vertex, Bounds: geometry.Bounds, xml2js,
    parse_scene_xml: scene.parse_scene_xml, pack_primitive: scene.pack_primitive,
    screen_dimension: scene.screen_dimension, load_scene_from_ini: scene.load_scene_from_ini,
    load_scene_xml_file: scene.load_scene_xml_file,
    programEntry, make_meta, check_window, check_rects, MODE, encode_png, native: addon.load,
    queryHits, queryOccluded, cameraRays,
};
