"""Seeded ray batches and their oracle answers for the ray queries (include/pt_hip.h pt_query_hits,
pt_query_occluded), shared by test_query_cpu.py, test_gpu_query.py and test_gpu_node_query.py.

The reference of every ray is ONE oracle.intersect call (po_intersect: the reference's intersect()); a
ray is a reported hit iff the oracle hits and its t < tmax.  batch(scene, packed) builds, once per
session and scene:

  the hits batch, in a seeded random order (so that every prefix and every wave mixes the families):
    camera   the 40 x 24 image of test_gpu_window.py, frame 3 (denoise_ref.camera_ray); MedievalBoat 24 x 16
    inside   1,031 rays from uniform points of the scene's vertex bounding box, uniform directions
    scaled   the first 256 camera rays with d * 0.25 and again with d * 3 (the oracle's own answers)
    axis     128 rays along +-x, +-y, +-z (zero components: inv = +-inf, NaN slabs), 16 of them from
             camera hit points, the others from `inside` origins
    odd      d = 0, a NaN origin, an infinite direction component, and a hitting camera ray with
             tmax = 0, tmax < 0 and tmax = NaN — only when the oracle terminates on each
             (oracle_terminates: a child process with a time limit; test_query_cpu.py asserts it does)
  the occlusion batch, derived: for every ray above that the oracle hits at t, four rays with
    tmax = t / 2 -> 0, t -> 0 (strict <), nextafter(t, +inf) -> 1, 2 t -> 1; for every miss tmax = +inf -> 0;
    also in a seeded random order.

Shares counted on the CPU with the oracle alone (test_query_cpu.py asserts the bounds: hits batch at
least 10 % hits and 10 % misses, occlusion batch at least 25 % of each value):

    scene               rays   hits   misses   occlusion rays   ones    zeros
    CornellBox          2637   65.3 %  34.7 %        7815       44.2 %  55.8 %
    CornellBox-Glossy   2637   54.3 %  45.7 %        6939       41.3 %  58.7 %
    CornellBox-Sphere   2637   54.2 %  45.8 %        6936       41.3 %  58.7 %
    MedievalBoat        2061   38.0 %  62.0 %        4419       35.6 %  64.4 %

(hits per family on CornellBox: camera 493 of 960, inside 889 of 1,031, scaled 238 of 512, axis 103 of
128; the six odd rays are reported misses on every scene.)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

import denoise_ref as dr
import oracle

F = np.float32
FRAME = 3
CAMERA_SIZE = {"MedievalBoat": (24, 16)}  # the others: test_gpu_window.py's 40 x 24
N_INSIDE, N_SCALED, N_AXIS, N_AXIS_HITPOINTS = 1031, 256, 128, 16
SEED = 20261020
MISS = np.array([0, 0, 0, -1, 0, 0, 0, 0], F)
MISS[7:8].view(np.int32)[0] = -1


def camera_size(scene):
    return CAMERA_SIZE.get(scene, (40, 24))


def make_ray(o, d, tmax=np.inf, reserved=0):
    r = np.zeros(8, F)
    r[0:3], r[3], r[4:7] = o[:3], tmax, d[:3]
    r[7:8].view(np.uint32)[0] = reserved
    return r


def hit_record(out):
    """po_intersect's eight floats (p, n, t, material) as a pt_hit record (p, t, n, material as int32)."""
    h = np.zeros(8, F)
    h[0:3], h[3], h[4:7] = out[0:3], out[6], out[3:6]
    h[7:8].view(np.int32)[0] = int(out[7])
    return h


def vertex_bounds(tri):
    v = np.asarray(tri, F)[16:16 + 3 * int(tri[0])].reshape(-1, 3)
    return v.min(axis=0), v.max(axis=0)


def odd_rays(hitting):
    """The odd rays; `hitting`: a camera ray (8 floats) the oracle hits."""
    o, d = hitting[0:3], hitting[4:7]
    return [make_ray(o, (0, 0, 0)),
            make_ray((np.nan, o[1], o[2]), d),
            make_ray(o, (np.inf, d[1], d[2])),
            make_ray(o, d, 0.0), make_ray(o, d, -1.0), make_ray(o, d, np.nan)]


_TERMINATES = {}


def oracle_terminates(scene, packed, rays, limit=120):
    """True when the oracle answers every ray within the time limit (a child process)."""
    key = (scene, np.asarray(rays, F).tobytes())
    if key not in _TERMINATES:
        with tempfile.TemporaryDirectory() as td:
            np.save(os.path.join(td, "tri.npy"), packed.triangle_data)
            np.save(os.path.join(td, "bvh.npy"), packed.bvh_data)
            np.save(os.path.join(td, "rays.npy"), np.asarray(rays, F))
            code = ("import sys, numpy as np\n"
                    f"sys.path.insert(0, {os.path.dirname(oracle.__file__)!r})\n"
                    "import oracle\n"
                    f"t, b, r = (np.load({td!r} + '/' + n + '.npy') for n in ('tri', 'bvh', 'rays'))\n"
                    "for x in r: oracle.intersect(t, b, x[0:3], x[4:7])\n"
                    "print('done')\n")
            try:
                p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=limit)
                _TERMINATES[key] = p.returncode == 0 and "done" in p.stdout
            except subprocess.TimeoutExpired:
                _TERMINATES[key] = False
    return _TERMINATES[key]


class Batch:
    """rays [n, 8], ref [n, 8] (pt_hit records, MISS for a miss), hit [n] bool, family [n] names,
    counters (the oracle's summed over the hits batch, with ext_queries = n), occ_rays [m, 8], occ [m] uint8."""

    def __init__(self, scene, packed, vertex_normals=False):
        tri, bvh = packed.triangle_data, packed.bvh_data
        w, h = camera_size(scene)
        meta = packed.meta_for(w, h)
        rng = np.random.default_rng(SEED)
        rays, fam = [], []
        for y in range(h):
            for x in range(w):
                o, d = dr.camera_ray(meta, x, y, FRAME)
                rays.append(make_ray(o, d))
                fam.append("camera")
        self.camera = np.array(rays, F).reshape(h, w, 8)
        lo, hi = vertex_bounds(tri)
        org = (lo + (hi - lo) * rng.random((N_INSIDE, 3))).astype(F)
        dirs = rng.standard_normal((N_INSIDE, 3))
        dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F)
        for o, d in zip(org, dirs):
            rays.append(make_ray(o, d))
            fam.append("inside")
        for k in (F(0.25), F(3.0)):
            for r in rays[:N_SCALED]:
                rays.append(make_ray(r[0:3], r[4:7] * k))
                fam.append("scaled")
        oracle.set_vertex_normals(vertex_normals)
        try:
            cam_hits = []
            for r in rays[:w * h]:
                ok, out, _ = oracle.intersect(tri, bvh, r[0:3], r[4:7])
                if ok:
                    cam_hits.append((r, out[0:3].copy()))
            assert len(cam_hits) >= N_AXIS_HITPOINTS, (scene, len(cam_hits))
            step = len(cam_hits) // N_AXIS_HITPOINTS
            axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], F)
            for i in range(N_AXIS):
                o = cam_hits[i * step][1] if i < N_AXIS_HITPOINTS else org[i]
                rays.append(make_ray(o, axes[i % 6]))
                fam.append("axis")
            odd = odd_rays(cam_hits[len(cam_hits) // 2][0])
            self.odd_terminate = oracle_terminates(scene, packed, odd)
            if self.odd_terminate:
                rays += odd
                fam += ["odd"] * len(odd)
            rays = np.array(rays, F)
            perm = rng.permutation(len(rays))
            self.rays, self.family = rays[perm], np.array(fam)[perm]
            n = len(self.rays)
            self.ref = np.tile(MISS, (n, 1))
            self.hit = np.zeros(n, bool)
            self.counters = dict(samples=0, ext_queries=n, shadow_queries=0, nodes=0, tri_tests=0, box_tests=0)
            occ_rays, occ = [], []
            for i, r in enumerate(self.rays):
                ok, out, cnt = oracle.intersect(tri, bvh, r[0:3], r[4:7])
                for key in ("nodes", "tri_tests", "box_tests"):
                    self.counters[key] += cnt[key]
                if ok and out[6] < r[3]:
                    self.hit[i] = True
                    self.ref[i] = hit_record(out)
                if ok:
                    t = F(out[6])
                    for tmax, v in ((t / F(2), 0), (t, 0), (np.nextafter(t, F(np.inf)), 1), (t * F(2), 1)):
                        occ_rays.append(make_ray(r[0:3], r[4:7], tmax))
                        occ.append(v)
                else:
                    occ_rays.append(make_ray(r[0:3], r[4:7]))
                    occ.append(0)
        finally:
            oracle.set_vertex_normals(False)
        perm = rng.permutation(len(occ))
        self.occ_rays, self.occ = np.array(occ_rays, F)[perm], np.array(occ, np.uint8)[perm]

    def shares(self):
        return dict(rays=len(self.rays), hits=float(self.hit.mean()), misses=float(1 - self.hit.mean()),
                    occ_rays=len(self.occ), ones=float(self.occ.mean()), zeros=float(1 - self.occ.mean()))


_BATCHES = {}


def batch(scene, packed, vertex_normals=False):
    key = (scene, bool(vertex_normals))
    if key not in _BATCHES:
        _BATCHES[key] = Batch(scene, packed[scene], vertex_normals)
    return _BATCHES[key]


def hits_mismatch(got, b, n=None):
    """'' when got ([n, 8] f32, pt_hit records) equals the reference bit for bit, else a description."""
    ref = b.ref if n is None else b.ref[:n]
    g, r = np.ascontiguousarray(got, F).view(np.uint32), np.ascontiguousarray(ref, F).view(np.uint32)
    if g.shape != r.shape:
        return f"shape {g.shape} != {r.shape}"
    bad = np.flatnonzero((g != r).any(axis=1))
    if bad.size == 0:
        return ""
    i = int(bad[0])
    return (f"{bad.size} of {len(r)} records differ; first: ray {i} ({b.family[i]}) {b.rays[i]} got {got[i]} "
            f"/ {g[i]} want {ref[i]} / {r[i]}")
