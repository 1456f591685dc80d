"""Reference and inputs of the radiance queries (include/pt_hip.h pt_query_radiance, pt_camera_seeds),
shared by test_radiance_cpu.py and test_gpu_radiance.py.

The reference is tests/radiance_ref.c: the oracle's own radiance() — the file #includes oracle/pt_oracle.c
— looped over rays and samples with the call's seed rule, admission test and clamp-accumulate.  build(dir)
compiles it with the flags of oracle/Makefile's BASE (x86-64-v3) into `dir` (pytest's temporary
directory) and loads it with ctypes.

Ray families, 331 rays each, seeded per scene (family(scene, packed, name)):
  texel    points of surfaces — the oracle's hits of seeded rays (surface_points) — lifted 1e-3 along the
           hit's geometric normal, direction -n: the baking case
  probe    origins: such surface points lifted 0.05 .. 0.5 along the normal (irradiance probes sit near
           surfaces), uniform unit directions
  camera   331 camera rays (the middle rows) of frame 3 of view_meta's camera at camera_size(scene), with
           the seeds the render hands to radiance() (camera_rays_seeds)
  mixed    the three interleaved, with the rays of rejected_rays at every 23rd position from 5
The boat's surface points and camera are the `rigging` camera's (cam_cases.py): from uniform points of its
bounds, or through the scene file's camera, fewer than 0.12 of the rays gather any light (measured: texel
0.051, probe 0.015, camera 0.115), and the families must not pass on black.
Conditions on every family and scene, asserted on the reference alone by test_radiance_cpu.py (depth 8,
3 samples): at least 0.25 of the admitted rays gather light, at least one path ends by a miss, and
shadow rays are traced.
"""
import ctypes
import os
import subprocess

import numpy as np

import cam_cases as cc
import denoise_ref as dr
import oracle
import pt_amd
import query_ref as qr

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-fopenmp", "-march=x86-64-v3"]
N = 331
FRAME = 3
SEED = 20261021
FAMILIES = ("texel", "probe", "camera", "mixed")
BAND = F(2.0 ** -18)
_M32 = 0xFFFFFFFF

_lib = None


def build(build_dir):
    """The reference library, compiled once per process into build_dir."""
    global _lib
    if _lib is None:
        so = os.path.join(str(build_dir), "libradiance_ref.so")
        subprocess.run([os.environ.get("CC", "gcc"), *FLAGS, "-shared", "-o", so, os.path.join(HERE, "radiance_ref.c"), "-lm"],
                       check=True)
        L = ctypes.CDLL(so)
        p, u32, u64, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        L.rr_radiance.argtypes = [p, u32, p, u32, p, p, u64, ctypes.c_float, i, i, u32, p, p, p, p]
        L.rr_radiance.restype = None
        L.rr_set_vertex_normals.argtypes = [i]
        L.rr_hash1u.argtypes = [u32]
        L.rr_hash1u.restype = u32
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def radiance(lib, packed_scene, rays, seeds, nsamples=1, max_depth=8, rr=0.9, direct_only=False, out=None,
             vertex_normals=False):
    """(accum [n, 3] f32, admitted [n] bool, counters dict, miss_ends) of the reference for the call
    pt_query_radiance(rays, seeds, nsamples, ...) into `out` (default: zeros; left untouched)."""
    tri = np.ascontiguousarray(packed_scene.triangle_data, F)
    bvh = np.ascontiguousarray(packed_scene.bvh_data, F)
    r = np.ascontiguousarray(rays, F).reshape(-1, 8)
    sd = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
    n = r.shape[0]
    assert sd.shape[0] == n
    acc = np.zeros((n, 3), F) if out is None else np.array(out, F, copy=True, order="C")
    adm = np.zeros(n, np.uint8)
    cnt = oracle.Counters()
    miss = ctypes.c_uint64(0)
    lib.rr_set_vertex_normals(1 if vertex_normals else 0)
    try:
        lib.rr_radiance(_ptr(tri), tri.size, _ptr(bvh), bvh.size, _ptr(r), _ptr(sd), n, float(rr), 1 if direct_only else 0,
                        int(max_depth), int(nsamples), _ptr(acc), _ptr(adm), ctypes.byref(cnt), ctypes.byref(miss))
    finally:
        lib.rr_set_vertex_normals(0)
    return acc, adm.astype(bool), cnt.as_dict(), int(miss.value)


def sample_seeds(lib, seeds, s):
    """seed_in of sample s of every ray: the seed itself for s = 0, hash1u(seed + s * 16787) after."""
    sd = np.ascontiguousarray(seeds, np.uint32)
    if s == 0:
        return sd.copy()
    return np.array([lib.rr_hash1u((int(v) + s * 16787) & _M32) for v in sd], np.uint32)


def admitted(rays):
    """The admission test of include/pt_hip.h in f32, fused multiply-adds as written there."""
    d = np.ascontiguousarray(rays, F).reshape(-1, 8)[:, 4:7]
    with np.errstate(all="ignore"):
        q = np.array([dr.fmaf(z, z, dr.fmaf(y, y, x * x)) for x, y, z in d], F)
        return np.abs(q - F(1.0)) <= BAND


def camera_seed(meta, x, y, t):
    """The value pixel_sample hands to radiance() for pixel (x, y) and salt t (camera_ray's seed_out)."""
    index = (x + y * int(meta[0])) & _M32
    ts = oracle.hash1u(oracle.hash1u((index * 16787 + t) & _M32))
    ts = oracle.hash1u(ts)
    return oracle.hash1u((ts + ((index * 67 + t) & _M32)) & _M32)


def camera_rays_seeds(meta, frame, window=None):
    """(rays [h, w, 8] f32, seeds [h, w] uint32) of the window (x0, y0, w, h; None: the image) in `frame`:
    a numpy restatement of pixel_sample's first half (denoise_ref.camera_ray and the seed chain)."""
    x0, y0, w, h = window or (0, 0, int(meta[0]), int(meta[1]))
    rays, seeds = np.zeros((h, w, 8), F), np.zeros((h, w), np.uint32)
    t = int(F(frame))
    for j in range(h):
        for i in range(w):
            o, d = dr.camera_ray(meta, x0 + i, y0 + j, t)
            rays[j, i] = qr.make_ray(o, d)
            seeds[j, i] = camera_seed(meta, x0 + i, y0 + j, t)
    return rays, seeds


def rejected_rays(o, u):
    """Rays that are not admitted, and the two sides of the band's edge, from an admitted ray (o, u):
    [(name, ray, admitted)]."""
    u = np.asarray(u, F)
    # |d|^2 = 1 + 2^-18 exactly (the edge, admitted), and one f32 step of |d|^2 beyond on either side
    hi, lo = np.sqrt(1.0 + 2.0 ** -18), np.sqrt(1.0 - 2.0 ** -18)
    out = [("zero", qr.make_ray(o, (0, 0, 0)), False),
           ("nan", qr.make_ray(o, (np.nan, u[1], u[2])), False),
           ("inf", qr.make_ray(o, (np.inf, u[1], u[2])), False),
           ("double", qr.make_ray(o, u * F(2)), False),
           ("long", qr.make_ray(o, u * F(1 + 2.0 ** -10)), False),
           ("short", qr.make_ray(o, u * F(1 - 2.0 ** -10)), False)]
    for name, s in (("edge_hi", hi), ("edge_lo", lo)):
        for k, f in ((name + "_in", 1 - 2.0 ** -21), (name + "_out", 1 + 2.0 ** -21)):
            axis = qr.make_ray(o, (0, F(s * (f if "hi" in name else 1 / f)), 0))
            out.append((k, axis, bool(admitted(axis)[0])))
    return out


class Family:
    def __init__(self, rays, seeds, rejected=()):
        self.rays, self.seeds = np.ascontiguousarray(rays, F), np.ascontiguousarray(seeds, np.uint32)
        self.rejected = np.array(sorted(rejected), np.int64)  # positions of rays known not to be admitted


_SURF, _FAM, _REF = {}, {}, {}


def camera_size(scene):
    return qr.camera_size(scene)


def view_meta(scene, packed_scene):
    """The camera of the scene's `camera` family at camera_size(scene): the scene file's — the boat: the
    `rigging` camera of cam_cases.py, which looks at lit geometry (the file's sees mostly sea and sky)."""
    w, h = camera_size(scene)
    return cc.meta_of(scene, "rigging", (w, h)) if scene == "MedievalBoat" else packed_scene.meta_for(w, h)


def surface_points(scene, packed_scene, count, rng):
    """count (point, unit geometric normal) pairs: oracle hits of seeded rays — from uniform points inside
    the bounds in uniform directions; the boat: rays of its view_meta camera through random pixels, since
    most of what its bounds hold is unlit sea."""
    tri, bvh = packed_scene.triangle_data, packed_scene.bvh_data
    lo, hi = qr.vertex_bounds(tri)
    boat = scene == "MedievalBoat"
    meta = view_meta(scene, packed_scene)
    pts = []
    while len(pts) < count:
        if boat:
            o, d = dr.camera_ray(meta, int(rng.integers(0, int(meta[0]))), int(rng.integers(0, int(meta[1]))),
                                 int(rng.integers(0, 1 << 20)))
            o, d = o[:3], d[:3]
        else:
            o = (lo + (hi - lo) * rng.random(3)).astype(F)
            d = rng.standard_normal(3)
            d = (d / np.linalg.norm(d)).astype(F)
        ok, out, _ = oracle.intersect(tri, bvh, o, d)
        if ok and np.isfinite(out[:6]).all() and np.abs(out[3:6]).max() > 0:
            pts.append((out[0:3].copy(), out[3:6].copy()))
    return pts


def family(scene, packed, name):
    """The family's rays and seeds for the scene (memoised; vertex normals never enter the inputs)."""
    key = (scene, name)
    if key in _FAM:
        return _FAM[key]
    ps = packed[scene]
    rng = np.random.default_rng([SEED, sorted(packed).index(scene), FAMILIES.index(name)])
    if name == "texel":
        pts = surface_points(scene, ps, N, rng)
        o = np.array([p + n * F(1e-3) for p, n in pts], F)
        fam = Family(pt_amd.unit_rays(o, np.array([-n for _, n in pts], F)), rng.integers(0, 2 ** 32, N, dtype=np.uint32))
    elif name == "probe":
        pts = surface_points(scene, ps, N, rng)
        o = np.array([p + n * F(rng.uniform(0.05, 0.5)) for p, n in pts], F)
        fam = Family(pt_amd.unit_rays(o, rng.standard_normal((N, 3))), rng.integers(0, 2 ** 32, N, dtype=np.uint32))
    elif name == "camera":
        w, h = camera_size(scene)
        rows = -(-N // w)
        rays, seeds = camera_rays_seeds(view_meta(scene, ps), FRAME, (0, (h - rows) // 2, w, rows))
        fam = Family(rays.reshape(-1, 8)[:N], seeds.reshape(-1)[:N])
    else:
        parts = [family(scene, packed, f) for f in ("texel", "probe", "camera")]
        rays = np.stack([parts[i % 3].rays[i // 3] for i in range(N)])
        seeds = np.array([parts[i % 3].seeds[i // 3] for i in range(N)], np.uint32)
        rej, pos = rejected_rays(rays[0, 0:3], rays[0, 4:7]), []
        for k, i in enumerate(range(5, N, 23)):
            nm, ray, adm = rej[k % len(rej)]
            ray = ray.copy()
            ray[0:3] = rays[i, 0:3]
            rays[i] = ray
            if not adm:
                pos.append(i)
        fam = Family(rays, seeds, pos)
    _FAM[key] = fam
    return fam


def initial_accum(n=N):
    """The non-zero accumulator the parity tests add into: seeded, positive and negative values."""
    return np.random.default_rng(SEED + 1).uniform(-2.0, 4.0, (n, 3)).astype(F)


def reference(lib, scene, packed, name, nsamples, vertex_normals=False, max_depth=8, init=False):
    """radiance() of the family into zeros or (init) into initial_accum(), memoised."""
    key = (scene, name, nsamples, bool(vertex_normals), max_depth, bool(init))
    if key not in _REF:
        fam = family(scene, packed, name)
        _REF[key] = radiance(lib, packed[scene], fam.rays, fam.seeds, nsamples, max_depth, float(packed[scene].meta[45]),
                             False, initial_accum() if init else None, vertex_normals)
    return _REF[key]
