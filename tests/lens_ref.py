"""numpy/ctypes restatement of the lens cameras (include/pt_hip.h pt_scene_set_camera),
shared by test_lens_cpu.py and test_gpu_lens.py.

The prologue is denoise_ref.camera_ray's, statement for statement (the oracle's hashes and view_half_h, C
fmaf from libm); the models follow the header operation by operation: numpy f32 scalars (every operation
rounded once), fmaf where the header writes one, numpy's correctly rounded sqrt and division, the oracle's
pinned po_sinf / po_cosf.  The reference image of a frame is radiance_ref.radiance — the oracle's own
radiance() with the call's admission test and clamp-accumulate — on these rays and seeds."""
import ctypes

import numpy as np

import denoise_ref as dr
import oracle
import query_ref as qr
import radiance_ref as rr

F = np.float32
_M32 = 0xFFFFFFFF
KPI = F(3.14159)
MODELS = ("pinhole", "thin_lens", "ortho", "equirect")
fmaf = dr.fmaf

# The cases the CPU and GPU tests share: (scene, camera of cam_cases.py, cam = (model, lens_radius,
# focus_distance)).  40 x 32, the boat 24 x 16 (cam_cases.size_of); 3 frames from FRAME0, depth 8.  Every case
# carries light in >= 0.25 of its pixels (test_lens_cpu.py; the shares are in DESIGN.md §5.12).
FRAME0, NFRAMES, DEPTH = 2, 3, 8
BOAT_FOCUS = 1.63  # |focus - pos| of the boat's `rigging` camera
CASES = [
    ("CornellBox", "xml", ("thin_lens", 0.05, 3.6)),
    ("CornellBox", "xml", ("thin_lens", 0.3, 3.6)),
    ("CornellBox", "xml", ("ortho", 0.0, 3.6)),
    ("CornellBox", "oblique", ("thin_lens", 0.05, 3.6)),
    ("CornellBox", "oblique", ("thin_lens", 0.3, 3.6)),
    ("CornellBox", "oblique", ("ortho", 0.0, 3.6)),
    ("CornellBox", "inside_in", ("equirect", 0.0, 1.0)),
    ("CornellBox-Glossy", "oblique", ("thin_lens", 0.3, 3.6)),
    ("CornellBox-Glossy", "inside_in", ("equirect", 0.0, 1.0)),
    ("CornellBox-Sphere", "oblique", ("ortho", 0.0, 3.6)),
    ("CornellBox-Sphere", "oblique", ("thin_lens", 0.05, 3.6)),
    ("MedievalBoat", "rigging", ("thin_lens", 0.05, BOAT_FOCUS)),
    ("MedievalBoat", "rigging", ("thin_lens", 0.3, BOAT_FOCUS)),
    ("MedievalBoat", "rigging", ("ortho", 0.0, BOAT_FOCUS)),
    ("MedievalBoat", "rigging", ("equirect", 0.0, 1.0)),
]


def case_id(case):
    scene, camera, cam = case
    return f"{scene}-{camera}-{cam[0]}" + (f"-r{cam[1]}" if cam[0] == "thin_lens" else "")


_REF = {}


def initial_accum(h, w):
    """A non-zero accumulator to render onto."""
    return np.random.default_rng(20261020).uniform(0.0, 2.0, (h, w, 3)).astype(F)


def reference(lib, packed, case):
    """The case's reference, computed once per process and shared (callers leave it unchanged):
    (meta, accum [h, w, 3] from zeros, counters, [(rays, seeds, admitted) per frame])."""
    if case not in _REF:
        import cam_cases as cc
        scene, camera, cam = case
        meta = cc.meta_of(scene, camera)
        frames = []
        acc, cnt = render(lib, packed[scene], meta, cam, FRAME0, NFRAMES, DEPTH, frames=frames)
        _REF[case] = (meta, acc, cnt, frames)
    return _REF[case]


def reference_onto(lib, packed, case):
    """(accum of the case's NFRAMES frames onto initial_accum, the first frame alone from zeros), once."""
    if ("onto", case) not in _REF:
        meta, acc, _, frames = reference(lib, packed, case)
        h, w = acc.shape[:2]
        onto, _ = accumulate(lib, packed[case[0]], meta, frames, DEPTH, initial_accum(h, w))
        first, _ = accumulate(lib, packed[case[0]], meta, frames[:1], DEPTH, np.zeros((h, w, 3), F))
        _REF[("onto", case)] = (onto, first)
    return _REF[("onto", case)]


def _sincos(x):
    L = oracle.lib()
    return F(L.po_sinf(float(x))), F(L.po_cosf(float(x)))


def X(M, c):
    """cam_to_world applied to the point c: camera_ray's chain."""
    return [fmaf(M[12 + k], F(1.0), fmaf(M[8 + k], c[2], fmaf(M[4 + k], c[1], M[k] * c[0]))) for k in range(3)]


def N3(v):
    with np.errstate(all="ignore"):
        ln = np.sqrt(fmaf(v[2], v[2], fmaf(v[1], v[1], v[0] * v[0])))
        return [v[0] / ln, v[1] / ln, v[2] / ln]


def prologue(meta, x, y, t):
    """(norm_x, norm_y, vx, vy, ts after the third hash, seed_out): camera_ray's own statements."""
    meta = np.ascontiguousarray(meta, F)
    W, H = meta[0], meta[1]
    inv_w, inv_h, aspect = meta[8], meta[9], meta[10]
    index = (x + y * int(W)) & _M32
    ts = (index * 16787 + t) & _M32
    ts = oracle.hash1u(ts)
    ts = oracle.hash1u(ts)
    jit = oracle.hash2(ts)
    gx, gy = F(x) + (jit[0] - F(0.5)), F(y) + (jit[1] - F(0.5))
    norm_x = fmaf(gx + F(0.5), inv_w, F(-0.5))
    norm_y = fmaf(((H - F(1.0)) - gy) + F(0.5), inv_h, F(-0.5))
    vhh = F(oracle.lib().po_view_half_h(meta.ctypes.data_as(ctypes.c_void_p)))
    vhw = vhh * aspect
    vx, vy = vhw * norm_x, vhh * norm_y
    ts = oracle.hash1u(ts)
    seed = oracle.hash1u((ts + ((index * 67 + t) & _M32)) & _M32)
    return norm_x, norm_y, vx, vy, ts, seed


def lens_point(ts, lens_radius):
    """The thin lens's point in camera space (l.x, l.y) for the chain's ts."""
    hl = oracle.hash1u((ts + 0x9E3779B9) & _M32)
    u = oracle.hash2(hl)
    r = F(lens_radius) * np.sqrt(u[0])
    phi = (F(2.0) * KPI) * u[1]
    sn, cs = _sincos(phi)
    return r * cs, r * sn


def camera_ray(meta, cam, x, y, t):
    """(origin[3], direction[3], seed, target) of pixel (x, y) and salt t under cam = (model, lens_radius,
    focus_distance); target: the thin lens's X(c), else None."""
    meta = np.ascontiguousarray(meta, F)
    model, lens_radius, focus = cam[0], F(cam[1]), F(cam[2])
    focal, M = meta[2], meta[28:44]
    norm_x, norm_y, vx, vy, ts, seed = prologue(meta, x, y, t)
    target = None
    with np.errstate(all="ignore"):
        if model == "thin_lens":
            lx, ly = lens_point(ts, lens_radius)
            k = focus / focal
            c = (vx * k, vy * k, -focus)
            o = X(M, (lx, ly, F(0.0)))
            target = X(M, c)
            d = N3([target[i] - o[i] for i in range(3)])
        elif model == "ortho":
            k = focus / focal
            o = X(M, (vx * k, vy * k, F(0.0)))
            d = N3([-M[8], -M[9], -M[10]])
        elif model == "equirect":
            phi = norm_x * (F(2.0) * KPI)
            th = norm_y * KPI
            sp, cp = _sincos(phi)
            st, ct = _sincos(th)
            c = (ct * sp, st, -(ct * cp))
            o = [meta[4], meta[5], meta[6]]
            d = N3([fmaf(M[8 + k], c[2], fmaf(M[4 + k], c[1], M[k] * c[0])) for k in range(3)])
        else:
            raise ValueError(model)
    return np.array(o, F), np.array(d, F), seed, (None if target is None else np.array(target, F))


class FirstHits(dr.FirstHits):
    """denoise_ref.FirstHits with the model's ray for the pinhole's: the guide buffers' reference under cam
    (for cases whose rays are all admitted: features() counts every sample)."""

    def __init__(self, tri, bvh, meta, cam):
        super().__init__(tri, bvh, meta)
        self.cam = cam

    def hit(self, x, y, k):
        key = (x, y, k)
        if key not in self._memo:
            o, d, _, _ = camera_ray(self.meta, self.cam, x, y, int(F(k)) & _M32)
            ok, out, cnt = oracle.intersect(self.tri, self.bvh, o, d)
            if ok:
                a, emits = dr.albedo(self.tri, out[7])
                self._memo[key] = (out[3:6].copy(), F(out[6]), a, emits, cnt)
            else:
                self._memo[key] = (None, None, None, False, cnt)
        return self._memo[key]


def rays_seeds(meta, cam, frame, window=None):
    """(rays [h, w, 8] f32, seeds [h, w] uint32, admitted [h, w] bool) of the window (x0, y0, w, h; None: the
    image) in `frame` under cam."""
    x0, y0, w, h = window or (0, 0, int(meta[0]), int(meta[1]))
    rays, seeds = np.zeros((h, w, 8), F), np.zeros((h, w), np.uint32)
    t = int(F(frame))
    for j in range(h):
        for i in range(w):
            o, d, s, _ = camera_ray(meta, cam, x0 + i, y0 + j, t)
            rays[j, i] = qr.make_ray(o, d)
            seeds[j, i] = s
    return rays, seeds, rr.admitted(rays).reshape(h, w)


def render(lib, packed_scene, meta, cam, frame0, nframes, max_depth=8, acc=None, window=None, stride=1, frames=None):
    """(accum [h, w, 3], counters dict summed over the frames) of the render under cam: per frame,
    radiance_ref.radiance (nsamples = 1) on rays_seeds, added into acc in frame order.  frames (optional):
    collects each frame's (rays, seeds, admitted)."""
    x0, y0, w, h = window or (0, 0, int(meta[0]), int(meta[1]))
    acc = np.zeros((h, w, 3), F) if acc is None else acc
    made = [rays_seeds(meta, cam, frame0 + k * stride, window) for k in range(nframes)]
    if frames is not None:
        frames.extend(made)
    return accumulate(lib, packed_scene, meta, made, max_depth, acc)


def accumulate(lib, packed_scene, meta, frames, max_depth, acc):
    """The frames' samples — [(rays [h, w, 8], seeds, admitted)] — added into a copy of acc [h, w, 3] in
    order: (accum, counters summed)."""
    h, w = frames[0][0].shape[:2]
    acc = np.array(acc, F, copy=True, order="C")
    total = {}
    for rays, seeds, _ in frames:
        out, _, cnt, _ = rr.radiance(lib, packed_scene, rays.reshape(-1, 8), seeds.reshape(-1), nsamples=1,
                                     max_depth=max_depth, rr=float(meta[45]), direct_only=bool(meta[46] > 0),
                                     out=acc.reshape(-1, 3))
        acc = out.reshape(h, w, 3)
        for key, v in cnt.items():
            total[key] = total.get(key, 0) + v
    return acc, total
