"""Reference and inputs of the irradiance gathers (include/pt_hip.h pt_gather, pt_gather_rays), shared by
test_gather_cpu.py, test_gpu_gather.py and test_gpu_node_gather.py.

The reference is tests/gather_ref.c: the oracle's own sample_hemisphere, radiance, po_hash2 and po_sincosf
— the file #includes oracle/pt_oracle.c — looped over points and samples with the call's seed rule,
admission tests and accumulation.  build(dir) compiles it as radiance_ref.build does.

Points: 129 per scene, seeded — radiance_ref.surface_points (the boat's from its `rigging` camera) with
their geometric normals; the SH probes are those points lifted 0.25 along the normal.  Sample counts of the
parity tests: 1 and 3, the boat 1 and 8 (samples(scene)): with 3 samples barely a quarter of the boat's
texels gather light.
"""
import ctypes
import os
import subprocess

import numpy as np

import oracle
import pt_amd
import radiance_ref as rr

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
N = 129
SEED = 20261022
MODES = ("cosine", "sh9")
LIFT = F(0.25)

_lib = None
_PTS, _REF = {}, {}


def build(build_dir):
    """The reference library, compiled once per process into build_dir."""
    global _lib
    if _lib is None:
        so = os.path.join(str(build_dir), "libgather_ref.so")
        subprocess.run([os.environ.get("CC", "gcc"), *rr.FLAGS, "-shared", "-o", so, os.path.join(HERE, "gather_ref.c"), "-lm"],
                       check=True)
        L = ctypes.CDLL(so)
        p, u32, u64, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        L.gr_gather.argtypes = [p, u32, p, u32, p, u64, ctypes.c_float, i, i, u32, u32, i, p, p, p, p]
        L.gr_rays.argtypes = [p, u64, i, u32, p, p]
        L.gr_dirs.argtypes = [p, u64, i, u32, p]
        L.gr_sh9_basis.argtypes = [p, p]
        L.gr_set_vertex_normals.argtypes = [i]
        for fn in (L.gr_gather, L.gr_rays, L.gr_dirs, L.gr_sh9_basis, L.gr_set_vertex_normals):
            fn.restype = None
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def width(mode):
    return 27 if mode == "sh9" else 3


def samples(scene):
    """The sample counts of the parity tests."""
    return (1, 8) if scene == "MedievalBoat" else (1, 3)


def gather(lib, packed_scene, pts, nsamples, sample0=0, mode="cosine", max_depth=8, rr_prob=0.9, direct_only=False, out=None,
           vertex_normals=False):
    """(accum [n, 3 | 27] f32, admitted samples per point [n], counters dict, miss_ends) of the reference
    for the call pt_gather(pts, ...) into `out` (default: zeros; left untouched).  pts: [n, 8] f32
    (pt_amd.gather_points)."""
    tri = np.ascontiguousarray(packed_scene.triangle_data, F)
    bvh = np.ascontiguousarray(packed_scene.bvh_data, F)
    g = np.ascontiguousarray(pts, F).reshape(-1, 8)
    n, w = g.shape[0], width(mode)
    acc = np.zeros((n, w), F) if out is None else np.array(out, F, copy=True, order="C")
    assert acc.shape == (n, w)
    adm = np.zeros(n, np.uint32)
    cnt = oracle.Counters()
    miss = ctypes.c_uint64(0)
    lib.gr_set_vertex_normals(1 if vertex_normals else 0)
    try:
        lib.gr_gather(_ptr(tri), tri.size, _ptr(bvh), bvh.size, _ptr(g), n, float(rr_prob), 1 if direct_only else 0,
                      int(max_depth), int(sample0), int(nsamples), MODES.index(mode), _ptr(acc), _ptr(adm), ctypes.byref(cnt),
                      ctypes.byref(miss))
    finally:
        lib.gr_set_vertex_normals(0)
    return acc, adm, cnt.as_dict(), int(miss.value)


def rays(lib, pts, sample, mode="cosine"):
    """(rays [n, 8] f32, seeds [n] uint32): the reference's restatement of pt_gather_rays."""
    g = np.ascontiguousarray(pts, F).reshape(-1, 8)
    r, sd = np.zeros((g.shape[0], 8), F), np.zeros(g.shape[0], np.uint32)
    lib.gr_rays(_ptr(g), g.shape[0], MODES.index(mode), int(sample), _ptr(r), _ptr(sd))
    return r, sd


def dirs(lib, pts, sample, mode="cosine"):
    """[n, 3] f32: the generated directions, admitted or not (NaN: the point is not admitted)."""
    g = np.ascontiguousarray(pts, F).reshape(-1, 8)
    d = np.zeros((g.shape[0], 3), F)
    lib.gr_dirs(_ptr(g), g.shape[0], MODES.index(mode), int(sample), _ptr(d))
    return d


def sh9_basis(lib, d):
    v = np.ascontiguousarray(d, F).reshape(-1, 3)
    out = np.zeros((v.shape[0], 9), F)
    for k in range(v.shape[0]):
        lib.gr_sh9_basis(_ptr(v[k]), _ptr(out[k]))
    return out


class Points:
    def __init__(self, p, n, seeds):
        self.p, self.n, self.seeds = np.ascontiguousarray(p, F), np.ascontiguousarray(n, F), np.ascontiguousarray(seeds, np.uint32)
        self.packed = pt_amd.gather_points(self.p, self.n, self.seeds)


def points(scene, packed, mode="cosine"):
    """The scene's gather points (memoised): surface points and normals; "sh9": lifted 0.25 along the normal."""
    key = (scene, mode)
    if key not in _PTS:
        rng = np.random.default_rng([SEED, sorted(packed).index(scene)])
        surf = rr.surface_points(scene, packed[scene], N, rng)
        seeds = rng.integers(0, 2 ** 32, N, dtype=np.uint32)
        nrm = np.array([n for _, n in surf], F)
        p = np.array([q for q, _ in surf], F)
        _PTS[(scene, "cosine")] = Points(p, nrm, seeds)
        _PTS[(scene, "sh9")] = Points((p + nrm * LIFT).astype(F), nrm, seeds)
    return _PTS[key]


def scaled_normals(normals, seeds, scale, p=None):
    """(points with the normals scaled, points with those normals' normalised copies, fixed): fixed marks
    the normals whose normalised copy n / sqrt(nn) is its own normalised copy, bit for bit — there the two
    sets of points draw the same directions (the call normalises whatever normal it is given)."""
    n = len(normals)
    p = np.zeros((n, 3), F) if p is None else p
    big = (np.asarray(normals, F) * F(scale)).astype(F)
    unit = pt_amd.unit_rays(np.zeros((n, 3), F), big)[:, 4:7]
    twice = pt_amd.unit_rays(np.zeros((n, 3), F), unit)[:, 4:7]
    fixed = (unit.view(np.uint32) == twice.view(np.uint32)).all(axis=1)
    return pt_amd.gather_points(p, big, seeds), pt_amd.gather_points(p, unit, seeds), fixed


def initial_accum(n=N, w=3):
    """radiance_ref.initial_accum's recipe, w words per point: seeded, positive and negative values."""
    return np.random.default_rng(rr.SEED + 1).uniform(-2.0, 4.0, (n, w)).astype(F)


def reference(lib, scene, packed, mode, nsamples, vertex_normals=False, max_depth=8, init=False, sample0=0):
    """gather() of the scene's points into zeros or (init) into initial_accum(), memoised."""
    key = (scene, mode, nsamples, bool(vertex_normals), max_depth, bool(init), sample0)
    if key not in _REF:
        _REF[key] = gather(lib, packed[scene], points(scene, packed, mode).packed, nsamples, sample0, mode, max_depth,
                           float(packed[scene].meta[45]), False, initial_accum(N, width(mode)) if init else None, vertex_normals)
    return _REF[key]
