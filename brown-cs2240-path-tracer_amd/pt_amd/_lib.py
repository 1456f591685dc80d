"""ctypes binding of include/pt_hip.h (libpt_hip.so, built in-tree by csrc/Makefile)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB_FILE = os.path.join(_PKG_ROOT, "lib", "libpt_hip.so")

ABI_VERSION = 3  # include/pt_hip.h PT_ABI_VERSION
_CSRC = os.path.join(_PKG_ROOT, "csrc")
# csrc/Makefile BUILD_SRCS: the sources whose SHA-256 the library carries as pt_build_id()
_BUILD_SRCS = ["pt_kernels.hip", "pt_wavefront.hip", "pt_wf_source.hip", "pt_wf_trace.hip", "pt_wf_bf.hip", "pt_wf_shade.hip", "pt_leafpass.hip", "pt_image.hip", "pt_features.hip", "pt_denoise.hip", "pt_temporal.hip", "pt_query.hip", "pt_capi.hip", "pt_capi_render.hip",
               "pt_capi_adaptive.hip", "pt_capi_denoise.hip", "pt_capi_query.hip", "pt_capi_radiance.hip", "pt_capi_gather.hip", "pt_capi_selftest.hip",
               "pt_capi_multi.hip", "pt_capi_camera.hip", "pt_capi_views.hip", "pt_capi_temporal.hip", "pt_capi_internal.h", "pt_math.h", "pt_flavour.h", "pt_layout.h",
               "pt_device.h", "pt_path.h", "pt_kernels.h", "../../include/pt_hip.h", "pt_bvh.cpp", "pt_leafbvh.h",
               "pt_leafbvh.cpp", "pt_leafskip.cpp", "pt_scene_layout.h", "pt_scene_layout.cpp", "pt_rect_plan.h",
               "pt_rect_plan.cpp", "pt_view_plan.h", "pt_view_plan.cpp", "pt_query_plan.h", "pt_step_addr.h", "pt_wf_plan.h",
               "pt_wf_queue.h", "pt_wf_stage.h", "pt_occupancy.h", "pt_build.hip", "pt_capi_build.hip", "pt_build.h",
               "pt_lbvh_host.cpp", "Makefile"]
MODE_AUTO, MODE_MEGAKERNEL, MODE_WAVEFRONT = 0, 1, 2
MATH_FNS = ["sin", "cos", "tan", "acos", "log2", "exp2", "pow", "sqrt", "div", "hash1u", "hash1", "hash2x",
            "hash2y", "min", "max", "ray_inv"]

_STATUS = {0: "PT_OK", -1: "PT_ERR_INVALID", -2: "PT_ERR_SCENE", -3: "PT_ERR_NOMEM", -4: "PT_ERR_HIP",
           -5: "PT_ERR_NODEVICE"}


class PtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{_STATUS.get(code, code)}: {msg}")
        self.code = code


class Counters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("samples", "ext_queries", "shadow_queries", "nodes", "tri_tests", "box_tests")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class SceneInfo(ctypes.Structure):
    _fields_ = [("nodes", ctypes.c_uint32), ("leaves", ctypes.c_uint32), ("leaf_refs", ctypes.c_uint32),
                ("max_leaf", ctypes.c_uint32), ("max_stack", ctypes.c_uint32), ("materials", ctypes.c_uint32),
                ("emissive_tris", ctypes.c_uint32), ("vertices", ctypes.c_uint32), ("device_bytes", ctypes.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class BuildParams(ctypes.Structure):
    """pt_build_params (16 B): the LBVH's leaf size and whether the emitters go under the root."""
    _fields_ = [("max_leaf", ctypes.c_uint32), ("isolate_emitters", ctypes.c_uint32), ("profile", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def _build_params(max_leaf, isolate_emitters, profile=False) -> BuildParams:
    return BuildParams(_uint(max_leaf, "max_leaf"), 1 if isolate_emitters else 0, 1 if profile else 0, 0)


class RadianceParams(ctypes.Structure):
    """pt_radiance_params."""
    _fields_ = [("rr_prob", ctypes.c_float), ("direct_only", ctypes.c_int32), ("max_depth", ctypes.c_int32),
                ("nsamples", ctypes.c_uint32)]


class GatherParams(ctypes.Structure):
    """pt_gather_params."""
    _fields_ = [("rr_prob", ctypes.c_float), ("direct_only", ctypes.c_int32), ("max_depth", ctypes.c_int32),
                ("sample0", ctypes.c_uint32), ("nsamples", ctypes.c_uint32), ("mode", ctypes.c_uint32)]


GATHER_MODES = ("cosine", "sh9")  # PT_GATHER_COSINE, PT_GATHER_SH9, by value


CAMERA_MODELS = ("pinhole", "thin_lens", "ortho", "equirect")  # pt_camera_model, by value


class Camera(ctypes.Structure):
    """pt_camera (16 B): the model and its lens (Scene.set_camera)."""
    _fields_ = [("model", ctypes.c_uint32), ("lens_radius", ctypes.c_float), ("focus_distance", ctypes.c_float),
                ("reserved", ctypes.c_uint32)]


class Window(ctypes.Structure):
    """pt_window: pixels [x0, x0 + w) x [y0, y0 + h) of the image."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("x0", "y0", "w", "h")]


def _uint(v, what: str, lo: int = 0) -> int:
    """v as an integer in [lo, 2^32), else PtError(-1): the argument checks of the window calls."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise PtError(-1, f"{what} must be an integer, not {v!r}")
    if not lo <= int(v) <= 0xFFFFFFFF:
        raise PtError(-1, f"{what} must lie in [{lo}, 2^32), not {v!r}")
    return int(v)


def _window(window):
    """A (x0, y0, w, h) window checked on the host (four non-negative integers; the library checks
    it against the image) as a pt_window, or None for the whole image."""
    if window is None:
        return None
    try:
        t = tuple(window)
    except TypeError:
        raise PtError(-1, f"window must be (x0, y0, w, h), not {window!r}") from None
    if len(t) != 4:
        raise PtError(-1, f"window must have four values (x0, y0, w, h), not {len(t)}")
    return Window(*[_uint(v, f"window {n}") for v, n in zip(t, ("x0", "y0", "w", "h"))])


def _rects(rects):
    """A list of (x0, y0, w, h) rectangles checked on the host like _window (the library checks the
    list itself: its length, the areas, the frame, overlaps) as a pt_window array and its length."""
    try:
        items = [tuple(r) for r in rects]
    except TypeError:
        raise PtError(-1, f"rects must be a sequence of (x0, y0, w, h), not {rects!r}") from None
    arr = (Window * max(1, len(items)))()
    for k, t in enumerate(items):
        if len(t) != 4:
            raise PtError(-1, f"rects[{k}] must have four values (x0, y0, w, h), not {len(t)}")
        arr[k] = Window(*[_uint(v, f"rects[{k}] {n}") for v, n in zip(t, ("x0", "y0", "w", "h"))])
    return arr, len(items)


class View(ctypes.Structure):
    """pt_view (240 B): one view of Scene.render_views — its meta, the window of its image, its camera model,
    its place in the atlas, its first frame."""
    _fields_ = [("meta", ctypes.c_float * 48), ("win", Window), ("cam", Camera), ("dst_x", ctypes.c_uint32),
                ("dst_y", ctypes.c_uint32), ("frame0", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def _camera(camera) -> Camera:
    """None, a model's name, or (model, lens_radius, focus_distance) as Scene.set_camera takes them."""
    if camera is None:
        return Camera(0, 0.0, 0.0, 0)
    model, lens_radius, focus_distance = (camera, 0.0, 1.0) if isinstance(camera, (str, int)) else tuple(camera)
    m = CAMERA_MODELS.index(model) if isinstance(model, str) and model in CAMERA_MODELS else model
    if isinstance(m, str):
        raise ValueError(f"unknown camera model {model!r} (one of {CAMERA_MODELS})")
    return Camera(int(m), float(lens_radius), float(focus_distance), 0)


def view_atlas(sizes, cols=None):
    """A shelf packing of rectangles of sizes [(w, h), ...] in list order: rows of `cols` rectangles (None:
    ceil(sqrt(n))), each row as tall as its tallest.  Returns (dsts [(x, y), ...], (atlas_w, atlas_h))."""
    sizes = [(_uint(w, "view width", 1), _uint(h, "view height", 1)) for w, h in sizes]
    if not sizes:
        raise PtError(-1, "views: the list is empty (n must be at least 1)")
    n = len(sizes)
    cols = int(np.ceil(np.sqrt(n))) if cols is None else _uint(cols, "cols", 1)
    dsts, x, y, row_h, aw = [], 0, 0, 0, 0
    for k, (w, h) in enumerate(sizes):
        if k and k % cols == 0:
            x, y, row_h = 0, y + row_h, 0
        dsts.append((x, y))
        x += w
        row_h = max(row_h, h)
        aw = max(aw, x)
    return dsts, (aw, y + row_h)


def _views(views, atlas=None):
    """A list of {meta, window=None, camera=None, dst=None, frame0=0} dicts as a pt_view array, its length and
    the atlas (atlas_w, atlas_h): views without a dst are packed by view_atlas when none has one and no
    atlas is given."""
    try:
        items = [dict(v) for v in views]
    except (TypeError, ValueError):
        raise PtError(-1, f"views must be a sequence of dicts (meta, window, camera, dst, frame0), not {views!r}") from None
    arr = (View * max(1, len(items)))()
    wins = []
    for k, v in enumerate(items):
        unknown = set(v) - {"meta", "window", "camera", "dst", "frame0"}
        if unknown or "meta" not in v:
            raise PtError(-1, f"views[{k}] needs meta and may hold window, camera, dst, frame0; not {sorted(unknown)}")
        meta = _f32(v["meta"])
        if meta.size != 48:
            raise PtError(-1, f"views[{k}] meta must hold 48 floats, not {meta.size}")
        win = _window(v.get("window"))
        if win is None:
            W, H = float(meta[0]), float(meta[1])
            if not (1 <= W <= 32768 and 1 <= H <= 32768):
                raise PtError(-1, f"views[{k}]: meta[0..1] must be integral resolutions in [1, 32768]")
            win = Window(0, 0, int(W), int(H))
        ctypes.memmove(arr[k].meta, meta.ctypes.data, 192)  # the bits, NaN payloads included
        arr[k].win = win
        arr[k].cam = _camera(v.get("camera"))
        arr[k].frame0 = _uint(v.get("frame0", 0), f"views[{k}] frame0")
        wins.append((win.w, win.h))
    dsts = [v.get("dst") for v in items]
    if items and all(d is None for d in dsts) and atlas is None:
        dsts, atlas = view_atlas(wins)
    if atlas is None or any(d is None for d in dsts):
        raise PtError(-1, "views: give every view a dst and the call an atlas=(w, h), or neither")
    for k, d in enumerate(dsts):
        t = tuple(d)
        if len(t) != 2:
            raise PtError(-1, f"views[{k}] dst must be (x, y), not {d!r}")
        arr[k].dst_x, arr[k].dst_y = _uint(t[0], f"views[{k}] dst x"), _uint(t[1], f"views[{k}] dst y")
    aw, ah = (_uint(a, "atlas " + n_, 1) for a, n_ in zip(tuple(atlas), ("w", "h")))
    return arr, len(items), (aw, ah)


class TileNoise(ctypes.Structure):
    """pt_tile_noise: a tile's noisy pixels, its pixels and its largest error estimate (16 bytes)."""
    _fields_ = [("noisy", ctypes.c_uint32), ("pixels", ctypes.c_uint32), ("max_err", ctypes.c_double)]


# numpy's view of an array of pt_tile_noise
TILE_NOISE_DTYPE = np.dtype([("noisy", "<u4"), ("pixels", "<u4"), ("max_err", "<f8")])


class Adaptive(ctypes.Structure):
    """pt_adaptive: the parameters of pt_render_adaptive."""
    _fields_ = [("tile_w", ctypes.c_uint32), ("tile_h", ctypes.c_uint32), ("min_frames", ctypes.c_uint32),
                ("step_frames", ctypes.c_uint32), ("max_frames", ctypes.c_uint32), ("tol", ctypes.c_double),
                ("floor", ctypes.c_double), ("noisy_fraction", ctypes.c_double)]


def _tile(tile):
    """A (tile_w, tile_h) pair checked on the host: two integers >= 1."""
    try:
        t = tuple(tile)
    except TypeError:
        raise PtError(-1, f"tile must be (tile_w, tile_h), not {tile!r}") from None
    if len(t) != 2:
        raise PtError(-1, f"tile must have two values (tile_w, tile_h), not {len(t)}")
    return _uint(t[0], "tile_w", 1), _uint(t[1], "tile_h", 1)


def _real(v, what: str, positive: bool = True) -> float:
    """v as a finite float (> 0 when positive), else PtError(-1)."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise PtError(-1, f"{what} must be a number, not {v!r}")
    f = float(v)
    if not np.isfinite(f) or (positive and not f > 0.0):
        raise PtError(-1, f"{what} must be finite{' and > 0' if positive else ''}, not {v!r}")
    return f


def _adaptive(tile, min_frames, step_frames, max_frames, tol, floor, noisy_fraction, frame0) -> Adaptive:
    """pt_adaptive checked on the host, field by field (the library checks it again)."""
    tw, th = _tile(tile)
    lo = _uint(min_frames, "min_frames", 2)
    step = _uint(step_frames, "step_frames", 1)
    hi = _uint(max_frames, "max_frames", 1)
    if hi < lo:
        raise PtError(-1, f"max_frames must be at least min_frames ({lo}), not {hi}")
    nf = _real(noisy_fraction, "noisy_fraction", positive=False)
    if not 0.0 <= nf < 1.0:
        raise PtError(-1, f"noisy_fraction must lie in [0, 1), not {noisy_fraction!r}")
    if _uint(frame0, "frame0") + hi > 1 << 24:
        raise PtError(-1, f"frame0 + max_frames must not exceed 2^24, not {frame0} + {hi}")
    return Adaptive(tw, th, lo, step, hi, _real(tol, "tol"), _real(floor, "floor"), nf)


class DenoiseParams(ctypes.Structure):
    """pt_denoise_params: the a-trous passes (1..5, step 2^i) and the four sigmas (finite, > 0)."""
    _fields_ = [("iters", ctypes.c_uint32), ("sigma_n", ctypes.c_float), ("sigma_a", ctypes.c_float),
                ("sigma_z", ctypes.c_float), ("sigma_l", ctypes.c_float)]


def denoise_defaults() -> DenoiseParams:
    """pt_denoise_defaults: 4 passes, sigma_n 0.5, sigma_a 0.3, sigma_z 0.1, sigma_l 4.0."""
    p = DenoiseParams()
    load_library().pt_denoise_defaults(ctypes.byref(p))
    return p


def _denoise_params(params):
    """None (the library's defaults), a DenoiseParams, or a mapping / keyword set over the defaults'
    fields, checked on the host (the library checks again)."""
    if params is None:
        return None
    if isinstance(params, DenoiseParams):
        p = DenoiseParams(params.iters, params.sigma_n, params.sigma_a, params.sigma_z, params.sigma_l)
        it = p.iters
    else:
        try:
            kv = dict(params)
        except (TypeError, ValueError):
            raise PtError(-1, f"params must be a DenoiseParams or a mapping of its fields, not {params!r}") from None
        unknown = set(kv) - {n for n, _ in DenoiseParams._fields_}
        if unknown:
            raise PtError(-1, f"params: unknown field(s) {sorted(unknown)}")
        p = denoise_defaults()
        it = _uint(kv.get("iters", p.iters), "iters")
        p.iters = it
        for n in ("sigma_n", "sigma_a", "sigma_z", "sigma_l"):
            if n in kv:
                setattr(p, n, _real(kv[n], n))
    if not 1 <= it <= 5:
        raise PtError(-1, f"iters must lie in [1, 5], not {it}")
    for n in ("sigma_n", "sigma_a", "sigma_z", "sigma_l"):
        _real(getattr(p, n), n)
    return p


class TemporalParams(ctypes.Structure):
    """pt_temporal_params (16 B): the blend's floor alpha in (0, 1], a tap's least normal dot product, its
    largest relative depth difference (> 0) and the clamp of the history length (>= 1); all finite."""
    _fields_ = [("alpha", ctypes.c_float), ("normal_min", ctypes.c_float), ("depth_tol", ctypes.c_float),
                ("max_history", ctypes.c_float)]


def temporal_defaults() -> TemporalParams:
    """pt_temporal_defaults: alpha 0.2, normal_min 0.9, depth_tol 0.1, max_history 64."""
    p = TemporalParams()
    load_library().pt_temporal_defaults(ctypes.byref(p))
    return p


def _temporal_params(params):
    """None (the library's defaults), a TemporalParams, or a mapping over the defaults' fields, checked on
    the host (the library checks again)."""
    if params is None:
        return None
    names = [n for n, _ in TemporalParams._fields_]
    if isinstance(params, TemporalParams):
        p = TemporalParams(*(getattr(params, n) for n in names))
    else:
        try:
            kv = dict(params)
        except (TypeError, ValueError):
            raise PtError(-1, f"params must be a TemporalParams or a mapping of its fields, not {params!r}") from None
        unknown = set(kv) - set(names)
        if unknown:
            raise PtError(-1, f"params: unknown field(s) {sorted(unknown)}")
        p = temporal_defaults()
        for n in names:
            if n in kv:
                setattr(p, n, _real(kv[n], n, positive=False))
    for n in names:
        _real(getattr(p, n), n, positive=False)
    if not 0.0 < p.alpha <= 1.0:
        raise PtError(-1, f"alpha must lie in (0, 1], not {p.alpha!r}")
    if not p.depth_tol > 0.0:
        raise PtError(-1, f"depth_tol must be > 0, not {p.depth_tol!r}")
    if not p.max_history >= 1.0:
        raise PtError(-1, f"max_history must be at least 1, not {p.max_history!r}")
    return p


class Ray(ctypes.Structure):
    """pt_ray (32 B): origin, tmax, direction (not normalised; t is in its units), reserved (ignored)."""
    _fields_ = [("o", ctypes.c_float * 3), ("tmax", ctypes.c_float), ("d", ctypes.c_float * 3),
                ("reserved", ctypes.c_uint32)]


class Hit(ctypes.Structure):
    """pt_hit (32 B): point, t, shading normal, material; a miss is t = -1, material = -1, p = n = 0."""
    _fields_ = [("p", ctypes.c_float * 3), ("t", ctypes.c_float), ("n", ctypes.c_float * 3),
                ("material", ctypes.c_int32)]


RAY_DTYPE = np.dtype([("o", "<f4", 3), ("tmax", "<f4"), ("d", "<f4", 3), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("p", "<f4", 3), ("t", "<f4"), ("n", "<f4", 3), ("material", "<i4")])


def _rays(rays) -> np.ndarray:
    """A batch of rays as one contiguous [n, 8] f32 array (ox, oy, oz, tmax, dx, dy, dz, reserved bits):
    an array of RAY_DTYPE records, or anything of n * 8 f32 values."""
    a = np.asarray(rays)
    if a.dtype == RAY_DTYPE:
        a = np.ascontiguousarray(a).view(np.float32)
    else:
        a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size % 8:
        raise PtError(-1, f"rays must hold 8 floats per ray (o, tmax, d, reserved), not {a.size} values")
    return a.reshape(-1, 8)


def _fma32(a, b, c):
    """fmaf(a, b, c) for f32 arrays, correctly rounded: the product is exact in f64; the sum is taken in f64
    with its rounding error (TwoSum), which decides the one case where rounding f64 -> f32 would round
    twice — an f64 sum that sits exactly half way between two f32 values."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        r = s.astype(np.float32)
        fin = np.isfinite(s) & np.isfinite(r) & (err != 0.0)
        other = np.where(err > 0.0, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf)))
        # r was a tie broken the wrong way when s is the midpoint of r and its neighbour on err's side
        tie = fin & np.isfinite(other) & ((r.astype(np.float64) + other.astype(np.float64)) * 0.5 == s) & \
            (np.sign(s - r.astype(np.float64)) == np.sign(err))
    return np.where(tie, other, r).astype(np.float32)


def _gather_mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in GATHER_MODES:
            raise PtError(-1, f"mode must be one of {GATHER_MODES}, not {mode!r}")
        return GATHER_MODES.index(mode)
    return _uint(mode, "mode")


def gather_points(points, normals, seeds) -> np.ndarray:
    """[n, 8] f32 pt_gather_point records from points and normals ([n, 3]; normals None: zeros, for
    sh9) and seeds ([n] uint32, stored by their bits in column 3); column 7 (reserved) is 0."""
    p32 = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = p32.shape[0]
    n32 = np.zeros((n, 3), np.float32) if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    sd = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
    if n32.shape[0] != n or sd.shape[0] != n:
        raise PtError(-1, f"points, normals and seeds must hold as many entries ({n}, {n32.shape[0]}, {sd.shape[0]})")
    out = np.zeros((n, 8), np.float32)
    out[:, 0:3] = p32
    out[:, 4:7] = n32
    out.view(np.uint32)[:, 3] = sd
    return out


def sh9_basis(d) -> np.ndarray:
    """[n, 9] f32: the nine real SH basis values of the directions d ([n, 3] f32) as pt_gather's SH9 mode
    weights a sample, operation by operation in f32 (include/pt_hip.h)."""
    v = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    f = np.float32
    with np.errstate(all="ignore"):
        out = np.empty((v.shape[0], 9), np.float32)
        out[:, 0] = f(0.282095)
        out[:, 1] = f(0.488603) * y
        out[:, 2] = f(0.488603) * z
        out[:, 3] = f(0.488603) * x
        out[:, 4] = f(1.092548) * (x * y)
        out[:, 5] = f(1.092548) * (y * z)
        out[:, 6] = f(0.315392) * _fma32(f(3.0) * z, z, np.full_like(z, -1.0))
        out[:, 7] = f(1.092548) * (x * z)
        out[:, 8] = f(0.546274) * _fma32(x, x, -(y * y))
    return out


def sh9_irradiance(coeffs, normals) -> np.ndarray:
    """Irradiance [n, 3] (f64) at unit normals ([n, 3]) from SH9 radiance coefficients ([n, 27] or
    [n, 3, 9], already scaled by 4 pi / N): the cosine-lobe convolution of Ramamoorthi and Hanrahan
    (2001) — band l scaled by A_l = pi, 2 pi / 3, pi / 4 — evaluated with the basis of sh9_basis."""
    c = np.asarray(coeffs, np.float64).reshape(-1, 3, 9)
    nrm = np.asarray(normals, np.float64).reshape(-1, 3)
    if nrm.shape[0] != c.shape[0]:
        raise PtError(-1, f"coeffs and normals must hold as many entries ({c.shape[0]} and {nrm.shape[0]})")
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    Y = np.stack([np.full_like(x, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                  0.315392 * (3.0 * z * z - 1.0), 1.092548 * x * z, 0.546274 * (x * x - y * y)], axis=1)
    A = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    return np.einsum("nck,nk->nc", c, Y * A)


def unit_rays(o, d) -> np.ndarray:
    """[n, 8] f32 rays for query_radiance from origins o and directions d (both [n, 3], any length):
    tmax = +inf, reserved = 0, and d normalised in f32 with the reference's operations — d / sqrt(fma(dz,
    dz, fma(dy, dy, dx * dx))) — after a scaling by the power of two that brings the largest
    component into [0.5, 1) (exact but for components 2^-100 below it), so that no square overflows and the
    sum does not underflow.  The result of a
    finite non-zero direction is always admitted (|d|^2 within 2^-18 of 1); a zero or non-finite
    direction gives a ray that is not (NaN or zero direction)."""
    o32 = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
    d32 = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    if o32.shape != d32.shape:
        raise PtError(-1, f"o and d must hold as many vectors ({o32.shape[0]} and {d32.shape[0]})")
    with np.errstate(all="ignore"):
        m = np.max(np.abs(d32), axis=1)
        _, e = np.frexp(np.where(np.isfinite(m) & (m > 0), m, np.float32(1.0)))
        # two exact steps: one power of two of up to 2^149 is not an f32
        h = e // 2
        v = np.ldexp(np.ldexp(d32, -h[:, None]), -(e - h)[:, None]).astype(np.float32)
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        q = _fma32(z, z, _fma32(y, y, (x * x).astype(np.float32)))
        ln = np.sqrt(q, dtype=np.float32)
        u = (v / ln[:, None]).astype(np.float32)
    rays = np.zeros((o32.shape[0], 8), np.float32)
    rays[:, 0:3] = o32
    rays[:, 3] = np.inf
    rays[:, 4:7] = u
    return rays


def _extent(meta, win):
    """(w, h) of a call's result: the window's, or the image's of meta[0..1]."""
    return (int(win.w), int(win.h)) if win is not None else (int(meta[0]), int(meta[1]))


class KernelTime(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("launches", ctypes.c_uint64), ("total_ms", ctypes.c_double),
                ("min_ms", ctypes.c_double), ("max_ms", ctypes.c_double), ("busy_ms", ctypes.c_double)]


_lib = None


def lib_path() -> str:
    return _LIB_FILE


def _bind_torch_hip_runtime():
    """PyTorch-ROCm ships its own libamdhip64.so (SONAME libamdhip64.so.7, like /opt/rocm's).
    Loading libpt_hip.so first would pull /opt/rocm's runtime and torch would then load a
    second HIP/HSA runtime that finds no GPU.  Importing torch first makes libpt_hip.so bind to
    the runtime already in the process, so device pointers and streams are shared with torch.
    PT_AMD_NO_TORCH=1 skips this (standalone use on /opt/rocm's runtime)."""
    if os.environ.get("PT_AMD_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def source_hash() -> str:
    """SHA-256 of the library's sources as csrc/Makefile computes it (names sorted, contents
    concatenated); pt_build_id() of a library built from this tree returns the same digest."""
    import hashlib
    h = hashlib.sha256()
    for name in sorted(_BUILD_SRCS):
        with open(os.path.join(_CSRC, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def load_library():
    """Load libpt_hip.so; raise if it was not built, or was built from other sources than the
    tree it sits in (no silent fallback, no stale binary)."""
    global _lib
    if _lib is not None:
        return _lib
    _bind_torch_hip_runtime()
    if not os.path.exists(_LIB_FILE):
        raise PtError(-4, f"{_LIB_FILE} not built (run __graft_entry__.build() or make -C csrc)")
    L = ctypes.CDLL(_LIB_FILE)
    if L.pt_abi_version() != ABI_VERSION:
        raise PtError(-1, f"{_LIB_FILE} has ABI {L.pt_abi_version()}, this binding expects {ABI_VERSION} (rebuild)")
    L.pt_build_id.restype = ctypes.c_char_p
    built, here = L.pt_build_id().decode(), source_hash()
    if built != here:
        raise PtError(-1, f"{_LIB_FILE} was built from other sources (build id {built[:16]}, tree {here[:16]}): "
                          f"run __graft_entry__.build()")
    p, i, u32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t
    L.pt_abi_version.restype = i
    L.pt_last_error.restype = ctypes.c_char_p
    L.pt_device_count.argtypes = [ctypes.POINTER(i)]
    L.pt_scene_create.argtypes = [p, sz, p, sz, i, ctypes.POINTER(p)]
    L.pt_scene_destroy.argtypes = [p]
    L.pt_scene_destroy.restype = None
    L.pt_scene_get_info.argtypes = [p, ctypes.POINTER(SceneInfo)]
    L.pt_render.argtypes = [p, p, u32, u32, u32, i, i, p, p]
    L.pt_render_async.argtypes = [p, p, u32, u32, u32, i, i, p, p, p]
    L.pt_frame.argtypes = [p, p, u32, i, p]
    wp = ctypes.POINTER(Window)
    L.pt_render_window.argtypes = [p, p, wp, u32, u32, u32, i, i, p, p]
    L.pt_render_window_async.argtypes = [p, p, wp, u32, u32, u32, i, i, p, sz, p, p]
    L.pt_frame_window.argtypes = [p, p, wp, u32, i, p]
    L.pt_frame_async.argtypes = [p, p, u32, i, p, p]
    dbl = ctypes.c_double
    L.pt_render_moments.argtypes = [p, p, wp, u32, u32, u32, i, i, p, p, p]
    L.pt_render_moments_async.argtypes = [p, p, wp, u32, u32, u32, i, i, p, p, sz, p, p]
    L.pt_render_rects.argtypes = [p, p, wp, wp, sz, u32, u32, u32, i, i, p, p, p]
    L.pt_render_rects_async.argtypes = [p, p, wp, wp, sz, u32, u32, u32, i, i, p, p, sz, p, p]
    L.pt_selftest_rect_plan.argtypes = [wp, u32, u32, wp, sz, p, ctypes.POINTER(ctypes.c_uint64)]
    vp = ctypes.POINTER(View)
    L.pt_render_views.argtypes = [p, vp, sz, u32, u32, u32, u32, i, i, p, p]
    L.pt_render_views_async.argtypes = [p, vp, sz, u32, u32, u32, u32, i, i, p, sz, p, p]
    L.pt_selftest_view_plan.argtypes = [vp, sz, u32, u32, p, ctypes.POINTER(ctypes.c_uint64)]
    for fn in ("pt_render_views", "pt_render_views_async", "pt_selftest_view_plan"):
        getattr(L, fn).restype = i
    L.pt_noise_tiles_async.argtypes = [p, p, p, u32, u32, sz, u32, u32, p, dbl, dbl, p, p]
    L.pt_noise_tiles.argtypes = [p, p, p, u32, u32, u32, u32, p, dbl, dbl, p]
    L.pt_tile_mean_async.argtypes = [p, p, u32, u32, sz, u32, u32, p, p, p]
    L.pt_render_adaptive.argtypes = [p, p, wp, ctypes.POINTER(Adaptive), u32, i, i, p, p, p, p, p, p, ctypes.POINTER(u32)]
    L.pt_selftest_tile_rects.argtypes = [p, u32, u32, p, sz, ctypes.POINTER(sz)]
    dpp = ctypes.POINTER(DenoiseParams)
    L.pt_render_features.argtypes = [p, p, wp, u32, u32, u32, p, p, p]
    L.pt_render_features_async.argtypes = [p, p, wp, u32, u32, u32, p, p, sz, p, p]
    L.pt_query_hits.argtypes = [p, p, sz, p, p]
    L.pt_query_hits_async.argtypes = [p, p, sz, p, p, p]
    L.pt_query_occluded.argtypes = [p, p, sz, p, p]
    L.pt_query_occluded_async.argtypes = [p, p, sz, p, p, p]
    L.pt_camera_rays.argtypes = [p, p, wp, u32, p]
    L.pt_camera_rays_async.argtypes = [p, p, wp, u32, p, p]
    L.pt_query_radiance.argtypes = [p, p, p, sz, ctypes.POINTER(RadianceParams), p, p]
    L.pt_query_radiance_async.argtypes = [p, p, p, sz, ctypes.POINTER(RadianceParams), p, p, p]
    L.pt_camera_seeds.argtypes = [p, p, wp, u32, p]
    L.pt_camera_seeds_async.argtypes = [p, p, wp, u32, p, p]
    for fn in ("pt_query_radiance", "pt_query_radiance_async", "pt_camera_seeds", "pt_camera_seeds_async"):
        getattr(L, fn).restype = i
    L.pt_gather.argtypes = [p, p, sz, ctypes.POINTER(GatherParams), p, p]
    L.pt_gather_async.argtypes = [p, p, sz, ctypes.POINTER(GatherParams), p, p, p]
    L.pt_gather_rays.argtypes = [p, p, sz, u32, u32, p, p]
    L.pt_gather_rays_async.argtypes = [p, p, sz, u32, u32, p, p, p]
    for fn in ("pt_gather", "pt_gather_async", "pt_gather_rays", "pt_gather_rays_async"):
        getattr(L, fn).restype = i
    L.pt_denoise_defaults.argtypes = [dpp]
    L.pt_denoise_defaults.restype = None
    L.pt_denoise.argtypes = [p, p, p, u32, u32, u32, u32, p, p, p, u32, dpp, p, p]
    L.pt_denoise_async.argtypes = [p, p, p, u32, u32, sz, u32, u32, p, p, p, u32, dpp, p, p, p]
    L.pt_render_denoised_image.argtypes = [p, p, u32, u32, u32, i, i, u32, dpp, p, p]
    for fn in ("pt_render_features", "pt_render_features_async", "pt_denoise", "pt_denoise_async", "pt_render_denoised_image"):
        getattr(L, fn).restype = i
    tpp = ctypes.POINTER(TemporalParams)
    L.pt_temporal_defaults.argtypes = [tpp]
    L.pt_temporal_defaults.restype = None
    L.pt_reproject_async.argtypes = [p, p, p, u32, p, p, p, p, p, p, p, u32, u32, sz, tpp, p, p, p, p, p, p]
    L.pt_reproject.argtypes = [p, p, p, u32, p, p, p, p, p, p, p, u32, u32, tpp, p, p, p, p, p]
    L.pt_denoise_mean_async.argtypes = [p, p, p, u32, u32, sz, p, p, u32, dpp, p, p, p]
    L.pt_denoise_mean.argtypes = [p, p, p, u32, u32, p, p, u32, dpp, p, p]
    L.pt_history_create.argtypes = [p, u32, u32, ctypes.POINTER(p)]
    L.pt_history_reset.argtypes = [p]
    L.pt_history_destroy.argtypes = [p]
    L.pt_history_destroy.restype = None
    L.pt_history_step.argtypes = [p, p, u32, u32, u32, i, i, u32, tpp, dpp, p, p, p, p, p]
    for fn in ("pt_reproject_async", "pt_reproject", "pt_denoise_mean_async", "pt_denoise_mean", "pt_history_create",
               "pt_history_reset", "pt_history_step"):
        getattr(L, fn).restype = i
    L.pt_tonemap.argtypes = [p, sz, u32, p]
    L.pt_selftest_math.argtypes = [i, i, p, p, p, sz]
    L.pt_profile_enable.argtypes = [p, i]
    L.pt_profile_select.argtypes = [p, ctypes.c_char_p]
    L.pt_selftest_rcp.argtypes = [i, i, u32, u32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(u32)]
    L.pt_bvh_build.argtypes = [p, sz, p, sz, p, sz, ctypes.POINTER(sz)]
    L.pt_bvh_build_sah.argtypes = [p, sz, p, sz, p, sz, ctypes.POINTER(sz)]
    L.pt_bvh_build_sah2.argtypes = [p, sz, p, sz, p, sz, p, sz, ctypes.POINTER(sz)]
    bpp = ctypes.POINTER(BuildParams)
    L.pt_build_defaults.argtypes = [bpp]
    L.pt_bvh_build_lbvh.argtypes = [p, sz, bpp, p, sz, ctypes.POINTER(sz)]
    L.pt_scene_create_mesh.argtypes = [p, sz, bpp, i, ctypes.POINTER(p)]
    L.pt_scene_export_bvh.argtypes = [p, p, sz, ctypes.POINTER(sz)]
    for fn in ("pt_build_defaults", "pt_bvh_build_lbvh", "pt_scene_create_mesh", "pt_scene_export_bvh"):
        getattr(L, fn).restype = i
    L.pt_tonemap_async.argtypes = [p, p, sz, u32, p, p]
    L.pt_readback_async.argtypes = [p, p, sz, p, p]
    L.pt_render_image.argtypes = [p, p, u32, u32, u32, i, i, p, p]
    L.pt_profile_read.argtypes = [p, ctypes.POINTER(KernelTime), i, ctypes.POINTER(i)]
    L.pt_scene_set_vertex_normals.argtypes = [p, i]
    L.pt_scene_set_camera.argtypes = [p, ctypes.POINTER(Camera)]
    L.pt_scene_get_camera.argtypes = [p, ctypes.POINTER(Camera)]
    L.pt_scene_set_camera.restype = L.pt_scene_get_camera.restype = i
    L.pt_scene_check.argtypes = [p]
    L.pt_render_multi.argtypes = [ctypes.POINTER(p), i, p, u32, u32, u32, i, i, p, p]
    L.pt_set_hw_queues.argtypes = [i]
    L.pt_selftest_valu.argtypes = [i, i, i, i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
    L.pt_set_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.pt_get_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p, sz]
    L.pt_reset_options.argtypes = []
    L.pt_reset_options.restype = None
    i32p = ctypes.POINTER(ctypes.c_int32)
    L.pt_scene_leaf_bvh.argtypes = [p, i, i32p, i32p, i32p]
    L.pt_selftest_leaf.argtypes = [p, i, i, u32, u32, p]
    L.pt_selftest_lights.argtypes = [p, p, p, sz, p]
    L.pt_selftest_view_half_h.argtypes = [p, sz, p]
    for fn in ("pt_selftest_lights", "pt_selftest_view_half_h", "pt_render_moments", "pt_render_moments_async", "pt_noise_tiles_async", "pt_noise_tiles", "pt_tile_mean_async",
               "pt_render_adaptive", "pt_selftest_tile_rects", "pt_render_window", "pt_render_window_async", "pt_frame_window", "pt_scene_leaf_bvh", "pt_selftest_leaf", "pt_selftest_valu", "pt_set_option", "pt_get_option", "pt_release_communicators", "pt_scene_check", "pt_set_hw_queues", "pt_render_multi", "pt_bvh_build_sah", "pt_bvh_build_sah2", "pt_device_count", "pt_scene_create", "pt_scene_get_info", "pt_render", "pt_render_async", "pt_frame",
               "pt_frame_async", "pt_tonemap", "pt_selftest_math", "pt_profile_enable", "pt_profile_select", "pt_profile_read", "pt_selftest_rcp", "pt_bvh_build", "pt_tonemap_async", "pt_readback_async", "pt_render_image",
               "pt_scene_set_vertex_normals"):
        getattr(L, fn).restype = i
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise PtError(rc, load_library().pt_last_error().decode(errors="replace"))


def abi_version() -> int:
    return int(load_library().pt_abi_version())


def build_id() -> str:
    return load_library().pt_build_id().decode()


def _opt_name(name: str) -> str:
    """Option keys: the C names ("kernel", "trav", ...); the old environment spellings
    ("PT_KERNEL") are accepted and mapped."""
    return name[3:].lower() if name.startswith("PT_") else name


def set_option(name: str, value) -> None:
    """pt_set_option: process-wide kernel-selection switch (value None = default)."""
    v = None if value is None else str(value).encode()
    _check(load_library().pt_set_option(_opt_name(name).encode(), v))


def get_option(name: str) -> str:
    buf = ctypes.create_string_buffer(64)
    _check(load_library().pt_get_option(_opt_name(name).encode(), buf, 64))
    return buf.value.decode()


def reset_options() -> None:
    load_library().pt_reset_options()


def last_bf_width() -> int:
    """pt_last_bf_width: set width of the stackless replay in the fused step kernel launched last in
    this process — 32 (the narrow instance: scenes of <= 32 entries and nodes, option bf_narrow), 64,
    or 0 (none yet, the counting instances, the stack walk)."""
    f = load_library().pt_last_bf_width
    f.restype = ctypes.c_int
    return int(f())


def last_step_addr() -> int:
    """pt_last_step_addr: offset width of the queue addressing in the fused step kernel launched last in
    this process — 32 (the default while a part's queue arrays stay below 4 GiB), 64 (larger parts,
    option step_addr64), or 0 (none yet)."""
    f = load_library().pt_last_step_addr
    f.restype = ctypes.c_int
    return int(f())


class options:
    """Context manager: `with pt_amd.options(kernel="wavefront", trav="lean16"): ...` sets the
    options for the block and restores the previous values after it."""

    def __init__(self, mapping=None, **kv):
        self.kv = {_opt_name(k): v for k, v in {**(mapping or {}), **kv}.items()}
        self.saved = {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.saved[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *a):
        for k, v in self.saved.items():
            set_option(k, v or None)


def release_communicators() -> None:
    """pt_release_communicators: destroy the RCCL communicators pt_render_multi cached."""
    _check(load_library().pt_release_communicators())


def set_hw_queues(n: int = 8):
    """Explicit opt-in (pt_set_hw_queues): ask HIP for n hardware queues per process.  Only
    effective before the HIP runtime starts in this process (before torch touches the GPU);
    the library itself never changes the environment."""
    os.environ["GPU_MAX_HW_QUEUES"] = str(int(n))


def device_count() -> int:
    n = ctypes.c_int(0)
    _check(load_library().pt_device_count(ctypes.byref(n)))
    return n.value


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


class Scene:
    """One `SceneObjectPacked` resident on one GPU (program-raymarch.ts:109-131)."""

    def __init__(self, triangle_data, bvh_data, device: int = 0):
        self._lib = load_library()
        self.triangle_data = _f32(triangle_data)
        self.bvh_data = _f32(bvh_data)
        self.device = device
        h = ctypes.c_void_p()
        _check(self._lib.pt_scene_create(_ptr(self.triangle_data), self.triangle_data.size, _ptr(self.bvh_data),
                                         self.bvh_data.size, device, ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_mesh(cls, triangle_data, max_leaf: int = 4, isolate_emitters: bool = True, device: int = 0,
                  profile: bool = False) -> "Scene":
        """pt_scene_create_mesh: the scene from triangle_data alone — its tree (the LBVH of include/pt_hip.h)
        and device records are built on the GPU.  A traversal scene (no mailbox, leaf chunks, leaf pass or
        remainders); export_bvh() returns its tree in the reference's packed layout.  profile: the build's kernels are
        timed (profile_read() gives the time per stage, "k_build_sort", ...) and the timing stays enabled."""
        self = cls.__new__(cls)
        self._lib = load_library()
        self.triangle_data = _f32(triangle_data)
        self.bvh_data = None
        self.device = device
        prm = _build_params(max_leaf, isolate_emitters, profile)
        h = ctypes.c_void_p()
        _check(self._lib.pt_scene_create_mesh(_ptr(self.triangle_data), self.triangle_data.size, ctypes.byref(prm), device,
                                              ctypes.byref(h)))
        self._h = h
        return self

    def export_bvh(self) -> np.ndarray:
        """pt_scene_export_bvh: the packed bvh_data of a scene made by from_mesh — what bvh_build_lbvh returns
        for the same triangle_data and parameters."""
        n = ctypes.c_size_t(0)
        _check(self._lib.pt_scene_export_bvh(self._h, None, 0, ctypes.byref(n)))
        out = np.empty(n.value, np.float32)
        _check(self._lib.pt_scene_export_bvh(self._h, _ptr(out), out.size, ctypes.byref(n)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_vertex_normals(self, enable: bool = True):
        """Vertex-normal shading (pt_scene_set_vertex_normals; off = the reference's behaviour)."""
        _check(self._lib.pt_scene_set_vertex_normals(self._h, 1 if enable else 0))

    def set_camera(self, model="pinhole", lens_radius: float = 0.0, focus_distance: float = 1.0):
        """pt_scene_set_camera: the camera model of later calls on the scene — "pinhole" (the reference's,
        the default), "thin_lens" (lens_radius, focus_distance), "ortho" (focus_distance) or "equirect";
        a model's number (CAMERA_MODELS' index) is taken as it is."""
        m = CAMERA_MODELS.index(model) if isinstance(model, str) and model in CAMERA_MODELS else model
        if isinstance(m, str):
            raise ValueError(f"unknown camera model {model!r} (one of {CAMERA_MODELS})")
        cam = Camera(int(m), float(lens_radius), float(focus_distance), 0)
        _check(self._lib.pt_scene_set_camera(self._h, ctypes.byref(cam)))

    @property
    def camera(self) -> dict:
        """pt_scene_get_camera: {"model", "lens_radius", "focus_distance"} as set."""
        cam = Camera()
        _check(self._lib.pt_scene_get_camera(self._h, ctypes.byref(cam)))
        name = CAMERA_MODELS[cam.model] if cam.model < len(CAMERA_MODELS) else cam.model
        return {"model": name, "lens_radius": cam.lens_radius, "focus_distance": cam.focus_distance}

    @property
    def info(self) -> dict:
        inf = SceneInfo()
        _check(self._lib.pt_scene_get_info(self._h, ctypes.byref(inf)))
        return inf.as_dict()

    def leaf_bvhs(self) -> list:
        """pt_scene_leaf_bvh: (first record, entries, nodes) of every leaf BVH of the scene."""
        out, k = [], 0
        while True:
            a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
            if self._lib.pt_scene_leaf_bvh(self._h, k, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) != 0:
                return out
            out.append((a.value, b.value, c.value))
            k += 1

    def selftest_leaf(self, leaf: int, mode: int, seed: int, nrays: int) -> np.ndarray:
        """pt_selftest_leaf: [nrays, 6] int32 — the sequential loop's (position or -1, t bits), the
        walk's, the walk's entry tests and nodes (mode + 4: the shared multi-ray walk, no counts)."""
        out = np.zeros((nrays, 6), np.int32)
        _check(self._lib.pt_selftest_leaf(self._h, leaf, mode, seed, nrays, _ptr(out)))
        return out

    def selftest_lights(self, seeds, points):
        """pt_selftest_lights: the device's sample_area_lights for seeds [n] (uint32) and points [n, 3]:
        (directions [n, 3] float32, slots k [n] int32; k == Ntri is the table's clamped last entry)."""
        seeds = np.ascontiguousarray(seeds, np.uint32)
        points = _f32(points)
        if seeds.ndim != 1 or points.shape != (seeds.size, 3):
            raise ValueError("seeds must be [n] and points [n, 3]")
        out = np.zeros((seeds.size, 4), np.float32)
        _check(self._lib.pt_selftest_lights(self._h, _ptr(seeds), _ptr(points), seeds.size, _ptr(out)))
        return out[:, :3].copy(), out[:, 3].copy().view(np.int32)

    def render(self, meta, frame0: int, nframes: int, stride: int = 1, max_depth: int = -1, mode: int = MODE_AUTO,
               accum: np.ndarray | None = None, counters: bool = False, window=None):
        """Host-buffer render (blocking). Returns accum [H, W, 3] (and counters if requested).
        window=(x0, y0, w, h): only that rectangle of the image (pt_render_window) — accum is
        [h, w, 3] and holds the bits of accum_full[y0:y0+h, x0:x0+w] of the whole image's render."""
        meta = _f32(meta)
        win = _window(window)
        W, H = _extent(meta, win)
        if accum is None:
            accum = np.zeros((H, W, 3), np.float32)
        if accum.dtype != np.float32 or not accum.flags.c_contiguous or accum.size != W * H * 3:
            raise ValueError("accum must be a contiguous float32 array of H*W*3 elements (the window's h*w*3)")
        c = Counters()
        cp = ctypes.byref(c) if counters else None
        if win is None:
            _check(self._lib.pt_render(self._h, _ptr(meta), frame0, nframes, stride, max_depth, mode, _ptr(accum), cp))
        else:
            _check(self._lib.pt_render_window(self._h, _ptr(meta), ctypes.byref(win), frame0, nframes, stride,
                                              max_depth, mode, _ptr(accum), cp))
        return (accum, c.as_dict()) if counters else accum

    def render_async(self, meta, frame0: int, nframes: int, stride: int, max_depth: int, mode: int, d_accum_ptr: int,
                     stream_ptr: int = 0, d_counters_ptr: int = 0, window=None, row_pitch=None):
        """Device render into a caller-owned device buffer (e.g. a torch.cuda tensor's data_ptr()).
        window=(x0, y0, w, h): only that rectangle (pt_render_window_async); d_accum_ptr then
        addresses the window's FIRST pixel and row_pitch is the distance between its rows in pixels
        (default w: a dense [h, w, 3] buffer; the image's W with d_accum_ptr = image + 12 * (y0 * W
        + x0) bytes renders the window in place inside a full [H, W, 3] image)."""
        meta = _f32(meta)
        win = _window(window)
        if win is None and row_pitch is None:
            _check(self._lib.pt_render_async(self._h, _ptr(meta), frame0, nframes, stride, max_depth, mode,
                                             ctypes.c_void_p(d_accum_ptr), ctypes.c_void_p(d_counters_ptr or None),
                                             ctypes.c_void_p(stream_ptr or None)))
            return
        pitch = _extent(meta, win)[0] if row_pitch is None else _uint(row_pitch, "row_pitch")
        _check(self._lib.pt_render_window_async(self._h, _ptr(meta), ctypes.byref(win) if win is not None else None,
                                                frame0, nframes, stride, max_depth, mode, ctypes.c_void_p(d_accum_ptr),
                                                pitch, ctypes.c_void_p(d_counters_ptr or None),
                                                ctypes.c_void_p(stream_ptr or None)))

    def render_window_async(self, meta, window, frame0: int, nframes: int, stride: int, max_depth: int, mode: int,
                            d_accum_ptr: int, row_pitch=None, stream_ptr: int = 0, d_counters_ptr: int = 0):
        """pt_render_window_async under its own name: render_async with a window and a row pitch."""
        self.render_async(meta, frame0, nframes, stride, max_depth, mode, d_accum_ptr, stream_ptr, d_counters_ptr,
                          window=window, row_pitch=row_pitch)

    def render_moments(self, meta, frame0: int, nframes: int, stride: int = 1, max_depth: int = -1,
                       mode: int = MODE_AUTO, accum: np.ndarray | None = None, m2: np.ndarray | None = None,
                       counters: bool = False, window=None):
        """render that also accumulates the second moments (pt_render_moments): m2 += clamp(L)^2 per
        frame, f32, in/out like accum and of its shape.  Returns (accum, m2) (and counters if
        requested); accum holds the bits render gives from the same start."""
        meta = _f32(meta)
        win = _window(window)
        W, H = _extent(meta, win)
        bufs = []
        for a, what in ((accum, "accum"), (m2, "m2")):
            if a is None:
                a = np.zeros((H, W, 3), np.float32)
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous or a.size != W * H * 3:
                raise ValueError(f"{what} must be a contiguous float32 array of H*W*3 elements (the window's h*w*3)")
            bufs.append(a)
        c = Counters()
        _check(self._lib.pt_render_moments(self._h, _ptr(meta), ctypes.byref(win) if win is not None else None, frame0,
                                           nframes, stride, max_depth, mode, _ptr(bufs[0]), _ptr(bufs[1]),
                                           ctypes.byref(c) if counters else None))
        return (bufs[0], bufs[1], c.as_dict()) if counters else (bufs[0], bufs[1])

    def render_moments_async(self, meta, frame0: int, nframes: int, stride: int, max_depth: int, mode: int,
                             d_accum_ptr: int, d_m2_ptr: int, stream_ptr: int = 0, d_counters_ptr: int = 0, window=None,
                             row_pitch=None):
        """render_async with the second moments (pt_render_moments_async): d_m2_ptr addresses a device
        f32 buffer laid out like d_accum_ptr's (the window's first pixel, the same row_pitch)."""
        meta = _f32(meta)
        win = _window(window)
        pitch = _extent(meta, win)[0] if row_pitch is None else _uint(row_pitch, "row_pitch")
        _check(self._lib.pt_render_moments_async(self._h, _ptr(meta), ctypes.byref(win) if win is not None else None,
                                                 frame0, nframes, stride, max_depth, mode, ctypes.c_void_p(d_accum_ptr),
                                                 ctypes.c_void_p(d_m2_ptr or None), pitch,
                                                 ctypes.c_void_p(d_counters_ptr or None),
                                                 ctypes.c_void_p(stream_ptr or None)))

    def render_rects(self, meta, rects, frame0: int, nframes: int, stride: int = 1, max_depth: int = -1,
                     mode: int = MODE_AUTO, accum: np.ndarray | None = None, m2: np.ndarray | None = None,
                     counters: bool = False, frame=None):
        """pt_render_rects: the pixels of the (x0, y0, w, h) rectangles of rects (image coordinates,
        disjoint, inside frame) in ONE pass through the pipeline.  accum (and m2, when given: the second
        moments too) are [h, w, 3] over frame=(x0, y0, w, h) (None: the whole image), in/out; only the
        rectangles' pixels change, each to the bits Scene.render(window=...) gives it.  Returns accum,
        then m2 if given, then the counters if requested (one value: accum alone)."""
        meta = _f32(meta)
        fr = _window(frame)
        arr, n = _rects(rects)
        W, H = _extent(meta, fr)
        if accum is None:
            accum = np.zeros((H, W, 3), np.float32)
        for a, what in ((accum, "accum"), (m2, "m2")):
            if a is not None and (not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous or
                                  a.size != W * H * 3):
                raise ValueError(f"{what} must be a contiguous float32 array of H*W*3 elements (the frame's h*w*3)")
        c = Counters()
        _check(self._lib.pt_render_rects(self._h, _ptr(meta), ctypes.byref(fr) if fr is not None else None, arr, n, frame0,
                                         nframes, stride, max_depth, mode, _ptr(accum), _ptr(m2) if m2 is not None else None,
                                         ctypes.byref(c) if counters else None))
        out = (accum,) + ((m2,) if m2 is not None else ()) + ((c.as_dict(),) if counters else ())
        return out[0] if len(out) == 1 else out

    def render_rects_async(self, meta, rects, frame0: int, nframes: int, stride: int, max_depth: int, mode: int,
                           d_accum_ptr: int, d_m2_ptr: int = 0, row_pitch=None, stream_ptr: int = 0,
                           d_counters_ptr: int = 0, frame=None):
        """pt_render_rects_async: d_accum_ptr (and d_m2_ptr, 0: no moments) address the FIRST pixel of
        frame (None: the image) in device buffers whose rows are row_pitch pixels apart (default: the
        frame's width); nothing outside the rectangles is read or written."""
        meta = _f32(meta)
        fr = _window(frame)
        arr, n = _rects(rects)
        pitch = _extent(meta, fr)[0] if row_pitch is None else _uint(row_pitch, "row_pitch")
        _check(self._lib.pt_render_rects_async(self._h, _ptr(meta), ctypes.byref(fr) if fr is not None else None, arr, n,
                                               frame0, nframes, stride, max_depth, mode, ctypes.c_void_p(d_accum_ptr),
                                               ctypes.c_void_p(d_m2_ptr or None), pitch,
                                               ctypes.c_void_p(d_counters_ptr or None), ctypes.c_void_p(stream_ptr or None)))

    def render_views(self, views, nframes: int, stride: int = 1, max_depth: int = -1, mode: int = MODE_AUTO, atlas=None,
                     accum: np.ndarray | None = None, counters: bool = False):
        """pt_render_views: a list of views — dicts {meta, window=None, camera=None, dst=None, frame0=0}; camera
        as set_camera's arguments (model, lens_radius, focus_distance) — of this scene in ONE pass through the
        pipeline.  accum is the atlas [atlas_h, atlas_w, 3], in/out; view v's window lands at dst=(x, y) and
        holds the bits Scene.render(meta, frame0, nframes, stride, max_depth, window=window) gives under
        set_camera(*camera); nothing else of accum changes.  With atlas=None and no dst the views are packed
        by view_atlas.  Returns accum (and the counters, summed over the views, if requested)."""
        arr, n, (aw, ah) = _views(views, atlas)
        if accum is None:
            accum = np.zeros((ah, aw, 3), np.float32)
        if not isinstance(accum, np.ndarray) or accum.dtype != np.float32 or not accum.flags.c_contiguous or \
                accum.size != aw * ah * 3:
            raise ValueError("accum must be a contiguous float32 array of atlas_h*atlas_w*3 elements")
        c = Counters()
        _check(self._lib.pt_render_views(self._h, arr, n, aw, ah, _uint(nframes, "nframes"), _uint(stride, "stride"),
                                         max_depth, mode, _ptr(accum), ctypes.byref(c) if counters else None))
        return (accum, c.as_dict()) if counters else accum

    def render_views_async(self, views, nframes: int, stride: int, max_depth: int, mode: int, d_accum_ptr: int, atlas=None,
                           row_pitch=None, stream_ptr: int = 0, d_counters_ptr: int = 0):
        """pt_render_views_async: d_accum_ptr addresses the atlas's FIRST pixel in a device buffer whose rows
        are row_pitch pixels apart (default: the atlas's width); nothing outside the views' destination
        rectangles is read or written.  Returns the atlas's (w, h)."""
        arr, n, (aw, ah) = _views(views, atlas)
        pitch = aw if row_pitch is None else _uint(row_pitch, "row_pitch")
        _check(self._lib.pt_render_views_async(self._h, arr, n, aw, ah, _uint(nframes, "nframes"), _uint(stride, "stride"),
                                               max_depth, mode, ctypes.c_void_p(d_accum_ptr), pitch,
                                               ctypes.c_void_p(d_counters_ptr or None), ctypes.c_void_p(stream_ptr or None)))
        return aw, ah

    def noise_tiles(self, accum, m2, tile, frames, tol: float, floor: float) -> np.ndarray:
        """pt_noise_tiles: the noise verdict of every tile of tile=(tile_w, tile_h) pixels over the host
        accumulators accum and m2 [h, w, 3]; frames [TY, TX] are the tiles' sample counts.  Returns a
        [TY, TX] array of TILE_NOISE_DTYPE (noisy, pixels, max_err)."""
        acc, sq = _f32(accum), _f32(m2)
        if acc.ndim != 3 or acc.shape[2] != 3 or sq.shape != acc.shape:
            raise PtError(-1, f"accum and m2 must both be [h, w, 3], not {acc.shape} and {sq.shape}")
        h, w = acc.shape[:2]
        tw, th = _tile(tile)
        tx, ty = -(-w // tw), -(-h // th)
        fr = np.ascontiguousarray(frames, dtype=np.uint32)
        if fr.size != tx * ty:
            raise PtError(-1, f"frames must hold one count per tile ({ty} x {tx}), not {fr.shape}")
        out = np.zeros((ty, tx), TILE_NOISE_DTYPE)
        _check(self._lib.pt_noise_tiles(self._h, _ptr(acc), _ptr(sq), w, h, tw, th, _ptr(fr), _real(tol, "tol"),
                                        _real(floor, "floor"), _ptr(out)))
        return out

    def noise_tiles_async(self, d_accum_ptr: int, d_m2_ptr: int, w: int, h: int, tile, d_frames_ptr: int, tol: float,
                          floor: float, d_out_ptr: int, row_pitch=None, stream_ptr: int = 0):
        """pt_noise_tiles_async between caller-owned device buffers: accumulators of w x h pixels, rows
        row_pitch pixels apart (default w), u32 frames and 16-byte verdicts per tile."""
        tw, th = _tile(tile)
        w, h = _uint(w, "w", 1), _uint(h, "h", 1)
        pitch = w if row_pitch is None else _uint(row_pitch, "row_pitch")
        _check(self._lib.pt_noise_tiles_async(self._h, ctypes.c_void_p(d_accum_ptr or None), ctypes.c_void_p(d_m2_ptr or None),
                                              w, h, pitch, tw, th, ctypes.c_void_p(d_frames_ptr or None), _real(tol, "tol"),
                                              _real(floor, "floor"), ctypes.c_void_p(d_out_ptr or None),
                                              ctypes.c_void_p(stream_ptr or None)))

    def tile_mean_async(self, d_accum_ptr: int, w: int, h: int, tile, d_frames_ptr: int, d_mean_ptr: int, row_pitch=None,
                        stream_ptr: int = 0):
        """pt_tile_mean_async: mean = accum / f32(frames of the pixel's tile) (0 where that is 0), between
        device buffers of the same layout."""
        tw, th = _tile(tile)
        w, h = _uint(w, "w", 1), _uint(h, "h", 1)
        pitch = w if row_pitch is None else _uint(row_pitch, "row_pitch")
        _check(self._lib.pt_tile_mean_async(self._h, ctypes.c_void_p(d_accum_ptr or None), w, h, pitch, tw, th,
                                            ctypes.c_void_p(d_frames_ptr or None), ctypes.c_void_p(d_mean_ptr or None),
                                            ctypes.c_void_p(stream_ptr or None)))

    def render_adaptive(self, meta, frame0: int = 0, max_depth: int = -1, mode: int = MODE_AUTO, window=None,
                        tile=(64, 64), min_frames: int = 16, step_frames: int = 16, max_frames: int = 256,
                        tol: float = 0.05, floor: float = 0.05, noisy_fraction: float = 0.01, counters: bool = False) -> dict:
        """pt_render_adaptive: min_frames frames everywhere, then step_frames more per pass on the tiles
        where more than noisy_fraction of the pixels still have a relative standard error above tol,
        up to max_frames per tile.  Returns {"accum", "m2": [h, w, 3] sums over each tile's frames,
        "tile_frames": [TY, TX] u32, "tile_noise": [TY, TX] TILE_NOISE_DTYPE, "rgba": [h, w, 4] u8 of
        the per-tile mean, "passes"} and "counters" if requested."""
        meta = _f32(meta)
        win = _window(window)
        ad = _adaptive(tile, min_frames, step_frames, max_frames, tol, floor, noisy_fraction, frame0)
        W, H = _extent(meta, win)
        tx, ty = -(-W // ad.tile_w), -(-H // ad.tile_h)
        out = {"accum": np.zeros((H, W, 3), np.float32), "m2": np.zeros((H, W, 3), np.float32),
               "tile_frames": np.zeros((ty, tx), np.uint32), "tile_noise": np.zeros((ty, tx), TILE_NOISE_DTYPE),
               "rgba": np.zeros((H, W, 4), np.uint8)}
        c = Counters()
        npass = ctypes.c_uint32(0)
        _check(self._lib.pt_render_adaptive(self._h, _ptr(meta), ctypes.byref(win) if win is not None else None,
                                            ctypes.byref(ad), frame0, max_depth, mode, _ptr(out["accum"]), _ptr(out["m2"]),
                                            _ptr(out["tile_frames"]), _ptr(out["tile_noise"]), _ptr(out["rgba"]),
                                            ctypes.byref(c) if counters else None, ctypes.byref(npass)))
        out["passes"] = int(npass.value)
        if counters:
            out["counters"] = c.as_dict()
        return out

    def render_features(self, meta, frame0: int, nframes: int, stride: int = 1, geo: np.ndarray | None = None,
                        alb: np.ndarray | None = None, counters: bool = False, window=None):
        """pt_render_features: the guide buffers of the first hit, summed over the frames frame0 +
        i * stride: geo [h, w, 4] += (normal, hit distance), alb [h, w, 4] += (albedo, 1) per hit (so
        alb[..., 3] counts the hits), in/out like accum.  Returns (geo, alb) (and counters if requested).

        With the adaptive driver (tile frame counts differ, the guides are uniform):

            r = scene.render_adaptive(meta, tile=(64, 64), min_frames=16, max_frames=256)
            geo, alb = scene.render_features(meta, 0, 4)
            img, var = scene.denoise(r["accum"], r["m2"], geo, alb, feature_frames=4, tile=(64, 64),
                                     frames=r["tile_frames"])
        """
        meta = _f32(meta)
        win = _window(window)
        W, H = _extent(meta, win)
        bufs = []
        for a, what in ((geo, "geo"), (alb, "alb")):
            if a is None:
                a = np.zeros((H, W, 4), np.float32)
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous or a.size != W * H * 4:
                raise ValueError(f"{what} must be a contiguous float32 array of H*W*4 elements (the window's h*w*4)")
            bufs.append(a)
        c = Counters()
        _check(self._lib.pt_render_features(self._h, _ptr(meta), ctypes.byref(win) if win is not None else None, frame0,
                                            nframes, stride, _ptr(bufs[0]), _ptr(bufs[1]),
                                            ctypes.byref(c) if counters else None))
        return (bufs[0], bufs[1], c.as_dict()) if counters else (bufs[0], bufs[1])

    def render_features_async(self, meta, frame0: int, nframes: int, stride: int, d_geo_ptr: int, d_alb_ptr: int,
                              stream_ptr: int = 0, d_counters_ptr: int = 0, window=None, row_pitch=None):
        """pt_render_features_async: d_geo_ptr / d_alb_ptr address the window's FIRST pixel in device f32
        buffers of four floats per pixel (16-byte aligned), rows row_pitch pixels apart (default: the
        window's width)."""
        meta = _f32(meta)
        win = _window(window)
        pitch = _extent(meta, win)[0] if row_pitch is None else _uint(row_pitch, "row_pitch")
        _check(self._lib.pt_render_features_async(self._h, _ptr(meta), ctypes.byref(win) if win is not None else None,
                                                  frame0, nframes, stride, ctypes.c_void_p(d_geo_ptr or None),
                                                  ctypes.c_void_p(d_alb_ptr or None), pitch,
                                                  ctypes.c_void_p(d_counters_ptr or None), ctypes.c_void_p(stream_ptr or None)))

    def query_hits(self, rays, counters: bool = False):
        """pt_query_hits: the closest hit of every ray (rays: [n, 8] f32 — o, tmax, d, reserved — or
        RAY_DTYPE records; d is not normalised and t is in its units).  Returns [n, 8] f32 (p, t, n,
        material as int32 bits: `.view(pt_amd.HIT_DTYPE)` names the fields; a miss is t = -1,
        material = -1), and the counters if requested."""
        r = _rays(rays)
        out = np.zeros((r.shape[0], 8), np.float32)
        c = Counters()
        _check(self._lib.pt_query_hits(self._h, _ptr(r), r.shape[0], _ptr(out), ctypes.byref(c) if counters else None))
        return (out, c.as_dict()) if counters else out

    def query_occluded(self, rays, counters: bool = False):
        """pt_query_occluded: uint8 [n], 1 where the ray's closest hit lies below its tmax (the segment
        is blocked), computed with early exit; and the counters if requested."""
        r = _rays(rays)
        out = np.zeros(r.shape[0], np.uint8)
        c = Counters()
        _check(self._lib.pt_query_occluded(self._h, _ptr(r), r.shape[0], _ptr(out), ctypes.byref(c) if counters else None))
        return (out, c.as_dict()) if counters else out

    def camera_rays(self, meta, frame: int, window=None) -> np.ndarray:
        """pt_camera_rays: [h, w, 8] f32, the rays the render traces for the window's pixels in `frame`
        (tmax = +inf), ready for query_hits."""
        meta = _f32(meta)
        win = _window(window)
        W, H = _extent(meta, win)
        out = np.zeros((H, W, 8), np.float32)
        _check(self._lib.pt_camera_rays(self._h, _ptr(meta), ctypes.byref(win) if win is not None else None,
                                        _uint(frame, "frame"), _ptr(out)))
        return out

    def query_hits_async(self, d_rays_ptr: int, n: int, d_hits_ptr: int, stream_ptr: int = 0, d_counters_ptr: int = 0):
        """pt_query_hits_async: n pt_ray records at d_rays_ptr -> n pt_hit records at d_hits_ptr (device
        memory, both 16-byte aligned), asynchronous on the stream."""
        _check(self._lib.pt_query_hits_async(self._h, ctypes.c_void_p(d_rays_ptr or None), n,
                                             ctypes.c_void_p(d_hits_ptr or None), ctypes.c_void_p(d_counters_ptr or None),
                                             ctypes.c_void_p(stream_ptr or None)))

    def query_occluded_async(self, d_rays_ptr: int, n: int, d_occluded_ptr: int, stream_ptr: int = 0,
                             d_counters_ptr: int = 0):
        """pt_query_occluded_async: n pt_ray records -> n bytes at d_occluded_ptr."""
        _check(self._lib.pt_query_occluded_async(self._h, ctypes.c_void_p(d_rays_ptr or None), n,
                                                 ctypes.c_void_p(d_occluded_ptr or None),
                                                 ctypes.c_void_p(d_counters_ptr or None), ctypes.c_void_p(stream_ptr or None)))

    def camera_rays_async(self, meta, frame: int, d_rays_ptr: int, stream_ptr: int = 0, window=None):
        """pt_camera_rays_async: the window's w * h pt_ray records to d_rays_ptr (16-byte aligned)."""
        meta = _f32(meta)
        win = _window(window)
        _check(self._lib.pt_camera_rays_async(self._h, _ptr(meta), ctypes.byref(win) if win is not None else None,
                                              _uint(frame, "frame"), ctypes.c_void_p(d_rays_ptr or None),
                                              ctypes.c_void_p(stream_ptr or None)))

    def query_radiance(self, rays, seeds, nsamples: int = 1, max_depth: int = 8, rr: float = 0.9, direct_only: bool = False,
                       out=None, counters: bool = False):
        """pt_query_radiance: nsamples full paths from every ray (rays: [n, 8] f32 as for query_hits, unit
        directions — see unit_rays; seeds: [n] uint32, the seed of sample 0), clamped and added per ray.
        Returns [n, 3] f32: the sums, added to `out` ([n, 3] f32, left untouched) if given; and the
        counters if requested.  A ray whose direction is not admitted (|d|^2 further than 2^-18 from 1)
        is not traced and adds nothing."""
        r = _rays(rays)
        sd = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        n = r.shape[0]
        if sd.shape[0] != n:
            raise PtError(-1, f"seeds must hold one uint32 per ray ({n}), not {sd.shape[0]}")
        if out is None:
            acc = np.zeros((n, 3), np.float32)
        else:
            acc = np.array(out, np.float32, copy=True, order="C")
            if acc.shape != (n, 3):
                raise PtError(-1, f"out must be [n, 3] f32 with n = {n}, not {acc.shape}")
        prm = RadianceParams(float(rr), 1 if direct_only else 0, int(max_depth), _uint(nsamples, "nsamples"))
        c = Counters()
        _check(self._lib.pt_query_radiance(self._h, _ptr(r), _ptr(sd), n, ctypes.byref(prm), _ptr(acc),
                                           ctypes.byref(c) if counters else None))
        return (acc, c.as_dict()) if counters else acc

    def query_radiance_async(self, d_rays_ptr: int, d_seeds_ptr: int, n: int, d_accum_ptr: int, nsamples: int = 1,
                             max_depth: int = 8, rr: float = 0.9, direct_only: bool = False, stream_ptr: int = 0,
                             d_counters_ptr: int = 0):
        """pt_query_radiance_async: n pt_ray records (16-byte aligned), n uint32 seeds and the [n, 3] f32
        accumulator (in/out) in device memory, asynchronous on the stream."""
        prm = RadianceParams(float(rr), 1 if direct_only else 0, int(max_depth), _uint(nsamples, "nsamples"))
        _check(self._lib.pt_query_radiance_async(self._h, ctypes.c_void_p(d_rays_ptr or None),
                                                 ctypes.c_void_p(d_seeds_ptr or None), n, ctypes.byref(prm),
                                                 ctypes.c_void_p(d_accum_ptr or None),
                                                 ctypes.c_void_p(d_counters_ptr or None), ctypes.c_void_p(stream_ptr or None)))

    def gather(self, points, normals, seeds, nsamples: int, sample0: int = 0, mode="cosine", max_depth: int = 8,
               rr: float = 0.9, direct_only: bool = False, out=None, counters: bool = False):
        """pt_gather: samples sample0 .. sample0 + nsamples - 1 of every point (points, normals [n, 3] f32,
        seeds [n] uint32; normals may be None for "sh9"), their directions drawn on the device.  Returns
        the sums — [n, 3] f32 for "cosine" (irradiance = pi / N times it), [n, 27] for "sh9" (coefficient
        k of channel c at 9 c + k; scale by 4 pi / N) — added to `out` (left untouched) if given; and the
        counters if requested.  A point or sample that is not admitted adds nothing."""
        m = _gather_mode(mode)
        pts = gather_points(points, normals, seeds)
        n, w = pts.shape[0], 27 if m == 1 else 3
        if out is None:
            acc = np.zeros((n, w), np.float32)
        else:
            acc = np.array(out, np.float32, copy=True, order="C")
            if acc.shape != (n, w):
                raise PtError(-1, f"out must be [n, {w}] f32 with n = {n}, not {acc.shape}")
        prm = GatherParams(float(rr), 1 if direct_only else 0, int(max_depth), _uint(sample0, "sample0"),
                           _uint(nsamples, "nsamples"), m)
        c = Counters()
        _check(self._lib.pt_gather(self._h, _ptr(pts), n, ctypes.byref(prm), _ptr(acc), ctypes.byref(c) if counters else None))
        return (acc, c.as_dict()) if counters else acc

    def gather_async(self, d_points_ptr: int, n: int, d_accum_ptr: int, nsamples: int, sample0: int = 0, mode="cosine",
                     max_depth: int = 8, rr: float = 0.9, direct_only: bool = False, stream_ptr: int = 0,
                     d_counters_ptr: int = 0):
        """pt_gather_async: n pt_gather_point records (gather_points; 16-byte aligned) and the [n, 3] or
        [n, 27] f32 accumulator (in/out) in device memory, asynchronous on the stream."""
        prm = GatherParams(float(rr), 1 if direct_only else 0, int(max_depth), _uint(sample0, "sample0"),
                           _uint(nsamples, "nsamples"), _gather_mode(mode))
        _check(self._lib.pt_gather_async(self._h, ctypes.c_void_p(d_points_ptr or None), n, ctypes.byref(prm),
                                         ctypes.c_void_p(d_accum_ptr or None), ctypes.c_void_p(d_counters_ptr or None),
                                         ctypes.c_void_p(stream_ptr or None)))

    def gather_rays(self, points, normals, seeds, sample: int = 0, mode="cosine"):
        """pt_gather_rays: (rays [n, 8] f32, seeds [n] uint32) of sample `sample` of every point — the inputs
        with which query_radiance(nsamples=1) repeats that sample of a "cosine" gather.  A point or sample
        that is not admitted gets a zero direction and seed 0."""
        pts = gather_points(points, normals, seeds)
        n = pts.shape[0]
        rays, sd = np.zeros((n, 8), np.float32), np.zeros(n, np.uint32)
        _check(self._lib.pt_gather_rays(self._h, _ptr(pts), n, _gather_mode(mode), _uint(sample, "sample"), _ptr(rays), _ptr(sd)))
        return rays, sd

    def gather_rays_async(self, d_points_ptr: int, n: int, sample: int, d_rays_ptr: int, d_seeds_ptr: int, mode="cosine",
                          stream_ptr: int = 0):
        """pt_gather_rays_async: device pointers (points and rays 16-byte, seeds 4-byte aligned)."""
        _check(self._lib.pt_gather_rays_async(self._h, ctypes.c_void_p(d_points_ptr or None), n, _gather_mode(mode),
                                              _uint(sample, "sample"), ctypes.c_void_p(d_rays_ptr or None),
                                              ctypes.c_void_p(d_seeds_ptr or None), ctypes.c_void_p(stream_ptr or None)))

    def camera_seeds(self, meta, window=None, frame: int = 0) -> np.ndarray:
        """pt_camera_seeds: [h, w] uint32, the seed the render hands to radiance() for the window's pixels
        in `frame` — with camera_rays, the inputs with which query_radiance(nsamples=1) repeats that frame."""
        meta = _f32(meta)
        win = _window(window)
        W, H = _extent(meta, win)
        out = np.zeros((H, W), np.uint32)
        _check(self._lib.pt_camera_seeds(self._h, _ptr(meta), ctypes.byref(win) if win is not None else None,
                                         _uint(frame, "frame"), _ptr(out)))
        return out

    def camera_seeds_async(self, meta, frame: int, d_seeds_ptr: int, stream_ptr: int = 0, window=None):
        """pt_camera_seeds_async: the window's w * h uint32 seeds to d_seeds_ptr (4-byte aligned)."""
        meta = _f32(meta)
        win = _window(window)
        _check(self._lib.pt_camera_seeds_async(self._h, _ptr(meta), ctypes.byref(win) if win is not None else None,
                                               _uint(frame, "frame"), ctypes.c_void_p(d_seeds_ptr or None),
                                               ctypes.c_void_p(stream_ptr or None)))

    def denoise(self, accum, m2, geo, alb, feature_frames: int, frames, tile=None, params=None):
        """pt_denoise: the variance-guided a-trous filter over the host accumulators accum, m2 [h, w, 3]
        and the guide buffers geo, alb [h, w, 4] (render_features over feature_frames frames).  frames:
        the sample count of a uniform render, or with tile=(tile_w, tile_h) the [TY, TX] counts per tile
        (render_adaptive's tile_frames).  params: None (denoise_defaults()), a DenoiseParams or a
        mapping of its fields.  Returns (image [h, w, 3] f32: the filtered mean, variance [h, w])."""
        acc, sq, ge, al = _f32(accum), _f32(m2), _f32(geo), _f32(alb)
        if acc.ndim != 3 or acc.shape[2] != 3 or sq.shape != acc.shape:
            raise PtError(-1, f"accum and m2 must both be [h, w, 3], not {acc.shape} and {sq.shape}")
        h, w = acc.shape[:2]
        if ge.shape != (h, w, 4) or al.shape != (h, w, 4):
            raise PtError(-1, f"geo and alb must both be [{h}, {w}, 4], not {ge.shape} and {al.shape}")
        tw, th = (w, h) if tile is None else _tile(tile)
        tx, ty = -(-w // tw), -(-h // th)
        fr = np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1)
        if fr.size != tx * ty:
            raise PtError(-1, f"frames must hold one count per tile ({ty} x {tx}), not {fr.size} values")
        prm = _denoise_params(params)
        out, var = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
        _check(self._lib.pt_denoise(self._h, _ptr(acc), _ptr(sq), w, h, tw, th, _ptr(fr), _ptr(ge), _ptr(al),
                                    _uint(feature_frames, "feature_frames", 1), ctypes.byref(prm) if prm is not None else None,
                                    _ptr(out), _ptr(var)))
        return out, var

    def denoise_async(self, d_accum_ptr: int, d_m2_ptr: int, w: int, h: int, tile, d_frames_ptr: int, d_geo_ptr: int,
                      d_alb_ptr: int, feature_frames: int, d_out_ptr: int, d_var_out_ptr: int = 0, params=None,
                      row_pitch=None, stream_ptr: int = 0):
        """pt_denoise_async between caller-owned device buffers, all with rows row_pitch pixels apart
        (default w): accumulators [h, w, 3], guides [h, w, 4], u32 frames per tile of tile=(tile_w,
        tile_h), out [h, w, 3] and (0: none) var_out [h, w]."""
        tw, th = _tile(tile)
        w, h = _uint(w, "w", 1), _uint(h, "h", 1)
        pitch = w if row_pitch is None else _uint(row_pitch, "row_pitch")
        prm = _denoise_params(params)
        v = ctypes.c_void_p
        _check(self._lib.pt_denoise_async(self._h, v(d_accum_ptr or None), v(d_m2_ptr or None), w, h, pitch, tw, th,
                                          v(d_frames_ptr or None), v(d_geo_ptr or None), v(d_alb_ptr or None),
                                          _uint(feature_frames, "feature_frames", 1),
                                          ctypes.byref(prm) if prm is not None else None, v(d_out_ptr or None),
                                          v(d_var_out_ptr or None), v(stream_ptr or None)))

    def denoise_mean(self, c, var, geo, alb, feature_frames: int, params=None):
        """pt_denoise_mean: the denoiser for a caller that has the mean c [h, w, 3] and the variance of the
        mean var [h, w] (reproject's out and var); geo, alb, feature_frames and params as for denoise.
        Returns (image [h, w, 3], variance [h, w])."""
        cc, vv, ge, al = _f32(c), _f32(var), _f32(geo), _f32(alb)
        if cc.ndim != 3 or cc.shape[2] != 3:
            raise PtError(-1, f"c must be [h, w, 3], not {cc.shape}")
        h, w = cc.shape[:2]
        if vv.shape != (h, w):
            raise PtError(-1, f"var must be [{h}, {w}], not {vv.shape}")
        if ge.shape != (h, w, 4) or al.shape != (h, w, 4):
            raise PtError(-1, f"geo and alb must both be [{h}, {w}, 4], not {ge.shape} and {al.shape}")
        prm = _denoise_params(params)
        out, vout = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
        _check(self._lib.pt_denoise_mean(self._h, _ptr(cc), _ptr(vv), w, h, _ptr(ge), _ptr(al),
                                         _uint(feature_frames, "feature_frames", 1),
                                         ctypes.byref(prm) if prm is not None else None, _ptr(out), _ptr(vout)))
        return out, vout

    def denoise_mean_async(self, d_c_ptr: int, d_var_ptr: int, w: int, h: int, d_geo_ptr: int, d_alb_ptr: int,
                           feature_frames: int, d_out_ptr: int, d_var_out_ptr: int = 0, params=None, row_pitch=None,
                           stream_ptr: int = 0):
        """pt_denoise_mean_async between caller-owned device buffers, all with rows row_pitch pixels apart
        (default w): c [h, w, 3], var [h, w], guides [h, w, 4], out [h, w, 3] and (0: none) var_out [h, w]."""
        w, h = _uint(w, "w", 1), _uint(h, "h", 1)
        pitch = w if row_pitch is None else _uint(row_pitch, "row_pitch")
        prm = _denoise_params(params)
        v = ctypes.c_void_p
        _check(self._lib.pt_denoise_mean_async(self._h, v(d_c_ptr or None), v(d_var_ptr or None), w, h, pitch,
                                               v(d_geo_ptr or None), v(d_alb_ptr or None),
                                               _uint(feature_frames, "feature_frames", 1),
                                               ctypes.byref(prm) if prm is not None else None, v(d_out_ptr or None),
                                               v(d_var_out_ptr or None), v(stream_ptr or None)))

    def reproject(self, accum, m2, n: int, geo, alb, meta, prev=None, params=None):
        """pt_reproject: one step of temporal accumulation on host buffers.  accum, m2 [h, w, 3]: the sums of
        an n-frame moments render from zero; geo, alb [h, w, 4]: render_features' sums; meta: the step's
        camera.  prev: None (a first step) or the previous step's result (its "meta", "hist", "mom",
        "gbuf").  params: None (temporal_defaults()), a TemporalParams or a mapping of its fields.
        Returns {"meta", "hist", "mom", "gbuf" [h, w, 4], "out" [h, w, 3], "var" [h, w]}."""
        acc, sq, ge, al, meta = _f32(accum), _f32(m2), _f32(geo), _f32(alb), _f32(meta)
        if acc.ndim != 3 or acc.shape[2] != 3 or sq.shape != acc.shape:
            raise PtError(-1, f"accum and m2 must both be [h, w, 3], not {acc.shape} and {sq.shape}")
        h, w = acc.shape[:2]
        if ge.shape != (h, w, 4) or al.shape != (h, w, 4):
            raise PtError(-1, f"geo and alb must both be [{h}, {w}, 4], not {ge.shape} and {al.shape}")
        if meta.shape != (48,):
            raise PtError(-1, "meta must hold 48 floats")
        pm = ph = pq = pg = None
        if prev is not None:
            pm, ph, pq, pg = (_f32(prev[k]) for k in ("meta", "hist", "mom", "gbuf"))
            if pm.shape != (48,) or any(a.shape != (h, w, 4) for a in (ph, pq, pg)):
                raise PtError(-1, f"prev: meta must hold 48 floats and hist, mom, gbuf be [{h}, {w}, 4]")
        prm = _temporal_params(params)
        r = {"meta": meta.copy(), "hist": np.zeros((h, w, 4), np.float32), "mom": np.zeros((h, w, 4), np.float32),
             "gbuf": np.zeros((h, w, 4), np.float32), "out": np.zeros((h, w, 3), np.float32),
             "var": np.zeros((h, w), np.float32)}
        q = lambda a: _ptr(a) if a is not None else None
        _check(self._lib.pt_reproject(self._h, _ptr(acc), _ptr(sq), _uint(n, "n", 1), _ptr(ge), _ptr(al), _ptr(meta), q(pm),
                                      q(ph), q(pq), q(pg), w, h, ctypes.byref(prm) if prm is not None else None,
                                      _ptr(r["hist"]), _ptr(r["mom"]), _ptr(r["gbuf"]), _ptr(r["out"]), _ptr(r["var"])))
        return r

    def reproject_async(self, d_accum_ptr: int, d_m2_ptr: int, n: int, d_geo_ptr: int, d_alb_ptr: int, meta, w: int, h: int,
                        d_hist_ptr: int, d_mom_ptr: int, d_gbuf_ptr: int, meta_prev=None, d_hist_prev_ptr: int = 0,
                        d_mom_prev_ptr: int = 0, d_gbuf_prev_ptr: int = 0, d_out_ptr: int = 0, d_var_ptr: int = 0,
                        params=None, row_pitch=None, stream_ptr: int = 0):
        """pt_reproject_async between caller-owned device buffers, all with rows row_pitch pixels apart
        (default w).  meta_prev None and the three previous planes 0: a first step."""
        meta = _f32(meta)
        mp = None if meta_prev is None else _f32(meta_prev)
        w, h = _uint(w, "w", 1), _uint(h, "h", 1)
        pitch = w if row_pitch is None else _uint(row_pitch, "row_pitch")
        prm = _temporal_params(params)
        v = ctypes.c_void_p
        _check(self._lib.pt_reproject_async(self._h, v(d_accum_ptr or None), v(d_m2_ptr or None), _uint(n, "n", 1),
                                            v(d_geo_ptr or None), v(d_alb_ptr or None), _ptr(meta),
                                            _ptr(mp) if mp is not None else None, v(d_hist_prev_ptr or None),
                                            v(d_mom_prev_ptr or None), v(d_gbuf_prev_ptr or None), w, h, pitch,
                                            ctypes.byref(prm) if prm is not None else None, v(d_hist_ptr or None),
                                            v(d_mom_ptr or None), v(d_gbuf_ptr or None), v(d_out_ptr or None),
                                            v(d_var_ptr or None), v(stream_ptr or None)))

    def render_denoised(self, meta, frame0: int, nframes: int, stride: int = 1, max_depth: int = -1, mode: int = MODE_AUTO,
                        feature_frames: int = 4, params=None, counters: bool = False):
        """pt_render_denoised_image: an nframes (>= 2) moments render, the guides of the first
        feature_frames frames, the denoiser and the device tone map in one call: RGBA u8 [H, W, 4]."""
        meta = _f32(meta)
        W, H = int(meta[0]), int(meta[1])
        prm = _denoise_params(params)
        out = np.zeros((H, W, 4), np.uint8)
        c = Counters()
        _check(self._lib.pt_render_denoised_image(self._h, _ptr(meta), frame0, _uint(nframes, "nframes", 2), stride, max_depth,
                                                  mode, _uint(feature_frames, "feature_frames", 1),
                                                  ctypes.byref(prm) if prm is not None else None, _ptr(out),
                                                  ctypes.byref(c) if counters else None))
        return (out, c.as_dict()) if counters else out

    def render_image(self, meta, frame0: int, nframes: int, stride: int = 1, max_depth: int = -1,
                     mode: int = MODE_AUTO, counters: bool = False):
        """programEntry's displayed image in one call: RGBA u8 [H, W, 4] (device tone map)."""
        meta = _f32(meta)
        W, H = int(meta[0]), int(meta[1])
        out = np.zeros((H, W, 4), np.uint8)
        c = Counters()
        _check(self._lib.pt_render_image(self._h, _ptr(meta), frame0, nframes, stride, max_depth, mode, _ptr(out),
                                         ctypes.byref(c) if counters else None))
        return (out, c.as_dict()) if counters else out

    def readback_async(self, d_src_ptr: int, n: int, h_dst_ptr: int, stream_ptr: int = 0):
        """n floats from device memory to pinned host memory on `stream` (pt_readback_async)."""
        _check(self._lib.pt_readback_async(self._h, ctypes.c_void_p(d_src_ptr), n, ctypes.c_void_p(h_dst_ptr),
                                           ctypes.c_void_p(stream_ptr or None)))

    def tonemap_async(self, d_accum_ptr: int, npix: int, sample_runs: int, d_rgba_ptr: int, stream_ptr: int = 0):
        """Device tone map between caller-owned device buffers (e.g. torch tensors)."""
        _check(self._lib.pt_tonemap_async(self._h, ctypes.c_void_p(d_accum_ptr), npix, sample_runs,
                                          ctypes.c_void_p(d_rgba_ptr), ctypes.c_void_p(stream_ptr or None)))

    def check(self):
        """Wait for this scene's renders and raise if one failed on the device (pt_scene_check:
        a wavefront traversal wave that gave up at its watchdog limit)."""
        _check(self._lib.pt_scene_check(self._h))

    def profile_enable(self, enable: bool = True):
        """Bracket every kernel launch of this scene with HIP events (discards earlier records)."""
        _check(self._lib.pt_profile_enable(self._h, 1 if enable else 0))

    def profile_select(self, kernel: str | None = None):
        """Record only `kernel` ("k_wf_trace", "k_regen", ...); None = every kernel."""
        _check(self._lib.pt_profile_select(self._h, kernel.encode() if kernel else None))

    def profile_read(self) -> dict:
        """{kernel name: {"launches", "total_ms", "avg_ms", "min_ms", "max_ms", "busy_ms"}} since
        profile_enable(); busy_ms = union of the launches' intervals (parts on several streams overlap)."""
        buf = (KernelTime * 16)()
        n = ctypes.c_int(0)
        _check(self._lib.pt_profile_read(self._h, buf, 16, ctypes.byref(n)))
        out = {}
        for k in buf[: n.value]:
            out[k.name.decode()] = {"launches": int(k.launches), "total_ms": k.total_ms,
                                    "avg_ms": k.total_ms / max(1, k.launches), "min_ms": k.min_ms, "max_ms": k.max_ms,
                                    "busy_ms": k.busy_ms}
        return out

    def frame(self, meta, t: int, max_depth: int = -1, window=None) -> np.ndarray:
        """One reference dispatch: raw radiance [H, W, 3] for RNG salt t.  window=(x0, y0, w, h):
        that rectangle only, [h, w, 3], the same bits (pt_frame_window)."""
        meta = _f32(meta)
        win = _window(window)
        W, H = _extent(meta, win)
        out = np.zeros((H, W, 3), np.float32)
        if win is None:
            _check(self._lib.pt_frame(self._h, _ptr(meta), t, max_depth, _ptr(out)))
        else:
            _check(self._lib.pt_frame_window(self._h, _ptr(meta), ctypes.byref(win), t, max_depth, _ptr(out)))
        return out


def render_multi(scenes, meta, frame0: int, nframes: int, stride: int = 1, max_depth: int = -1,
                 mode: int = MODE_AUTO, accum: np.ndarray | None = None, counters: bool = False):
    """pt_render_multi: one image over several Scenes (one per device, repeats allowed), frames dealt
    round-robin, partial accumulators reduced onto scenes[0]'s device (RCCL, or PT_REDUCE=ordered)."""
    meta = _f32(meta)
    W, H = int(meta[0]), int(meta[1])
    if accum is None:
        accum = np.zeros((H, W, 3), np.float32)
    if accum.dtype != np.float32 or not accum.flags.c_contiguous or accum.size != W * H * 3:
        raise ValueError("accum must be a contiguous float32 array of H*W*3 elements")
    handles = (ctypes.c_void_p * len(scenes))(*[s._h.value for s in scenes])
    c = Counters()
    _check(load_library().pt_render_multi(handles, len(scenes), _ptr(meta), frame0, nframes, stride, max_depth, mode,
                                          _ptr(accum), ctypes.byref(c) if counters else None))
    return (accum, c.as_dict()) if counters else accum


def render_tiled(scene, meta, frame0: int, nframes: int, stride: int = 1, max_depth: int = -1,
                 mode: int = MODE_AUTO, tile=(256, 256), counters: bool = False):
    """The whole image rendered tile by tile: one Scene.render(window=...) per tile of tile=(tw, th)
    pixels (the right and bottom tiles are as small as the image leaves them), pasted into a full
    [H, W, 3] accumulator — the same bits as Scene.render of the whole image.  counters: summed over
    the tiles (samples and the query counts equal the whole image's; the traversal counts depend on
    which rays share a batch)."""
    meta = _f32(meta)
    try:
        tw, th = tile
    except (TypeError, ValueError):
        raise PtError(-1, f"tile must be (tw, th), not {tile!r}") from None
    tw, th = _uint(tw, "tile width", 1), _uint(th, "tile height", 1)
    W, H = int(meta[0]), int(meta[1])
    accum = np.zeros((H, W, 3), np.float32)
    total = Counters()
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            w, h = min(tw, W - x0), min(th, H - y0)
            r = scene.render(meta, frame0, nframes, stride, max_depth, mode, counters=counters, window=(x0, y0, w, h))
            if counters:
                r, c = r
                for n, _ in Counters._fields_:
                    setattr(total, n, getattr(total, n) + c[n])
            accum[y0:y0 + h, x0:x0 + w] = r
    return (accum, total.as_dict()) if counters else accum


def tile_rects(active) -> np.ndarray:
    """pt_selftest_tile_rects (host only): the rectangles [n, 4] u32 (tx0, ty0, width, height, in tiles)
    pt_render_adaptive renders for the [TY, TX] mask of active tiles."""
    a = np.ascontiguousarray(np.asarray(active) != 0, dtype=np.uint8)
    if a.ndim != 2 or a.size == 0:
        raise PtError(-1, f"active must be a non-empty [TY, TX] mask, not shape {a.shape}")
    ty, tx = a.shape
    out = np.zeros((max(1, int(a.sum())), 4), np.uint32)
    n = ctypes.c_size_t(0)
    _check(load_library().pt_selftest_tile_rects(_ptr(a), tx, ty, _ptr(out), out.shape[0], ctypes.byref(n)))
    return out[: n.value]


def rect_plan(rects, W: int, H: int, frame=None):
    """pt_selftest_rect_plan (host only): a rectangle list checked as pt_render_rects checks it, for a
    W x H image and frame=(x0, y0, w, h) (None: the image).  Returns (first, npix): every rectangle's
    first slot [n] u64 — the prefix sums of w * h in list order — and the list's pixels per frame."""
    fr = _window(frame)
    arr, n = _rects(rects)
    first = np.zeros(max(1, n), np.uint64)
    npix = ctypes.c_uint64(0)
    _check(load_library().pt_selftest_rect_plan(ctypes.byref(fr) if fr is not None else None, _uint(W, "W"), _uint(H, "H"),
                                                arr, n, _ptr(first), ctypes.byref(npix)))
    return first[:n], int(npix.value)


def view_plan(views, atlas=None):
    """pt_selftest_view_plan (host only): a view list checked as a one-frame pt_render_views checks it.
    Returns (first, npix): every view's first slot (uint64, list order) and the paths per frame."""
    arr, n, (aw, ah) = _views(views, atlas)
    first = np.zeros(n, np.uint64)
    npix = ctypes.c_uint64(0)
    _check(load_library().pt_selftest_view_plan(arr, n, aw, ah, _ptr(first), ctypes.byref(npix)))
    return first, int(npix.value)


class History:
    """pt_history: the temporal state of one camera path on the device (two sets of the hist, mom and gbuf
    planes of a w x h image and the previous step's camera), counted in the scene's device_bytes.  Close it
    before its scene; a step after the scene is gone raises PtError."""

    def __init__(self, scene: Scene, w: int, h: int):
        self._lib = scene._lib
        self.w, self.h = _uint(w, "w", 1), _uint(h, "h", 1)
        hd = ctypes.c_void_p()
        _check(self._lib.pt_history_create(scene._h, self.w, self.h, ctypes.byref(hd)))
        self._h = hd

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pt_history_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        """pt_history_reset: the next step is a first step."""
        _check(self._lib.pt_history_reset(self._h))

    def step(self, meta, frame0: int, nframes: int, stride: int = 1, max_depth: int = -1, mode: int = MODE_AUTO,
             feature_frames: int = 4, params=None, denoise=None, counters: bool = False) -> dict:
        """pt_history_step: an nframes moments render of meta's image, the guides of the first feature_frames
        frames, the reprojection against the previous step (params: as for Scene.reproject), optionally the
        denoiser (denoise: None = unfiltered, True = denoise_defaults(), or as Scene.denoise's params) and
        the tone map.  Returns {"mean" [h, w, 3], "var" [h, w], "rgba" [h, w, 4] u8, "history_len" [h, w]}
        (and "counters")."""
        meta = _f32(meta)
        if meta.shape != (48,):
            raise PtError(-1, "meta must hold 48 floats")
        tp = _temporal_params(params)
        dp = denoise_defaults() if denoise is True else _denoise_params(denoise)
        h, w = self.h, self.w
        r = {"mean": np.zeros((h, w, 3), np.float32), "var": np.zeros((h, w), np.float32),
             "rgba": np.zeros((h, w, 4), np.uint8), "history_len": np.zeros((h, w), np.float32)}
        c = Counters()
        _check(self._lib.pt_history_step(self._h, _ptr(meta), _uint(frame0, "frame0"), _uint(nframes, "nframes", 1),
                                         _uint(stride, "stride"), max_depth, mode, _uint(feature_frames, "feature_frames", 1),
                                         ctypes.byref(tp) if tp is not None else None,
                                         ctypes.byref(dp) if dp is not None else None, _ptr(r["mean"]), _ptr(r["var"]),
                                         _ptr(r["rgba"]), _ptr(r["history_len"]), ctypes.byref(c) if counters else None))
        if counters:
            r["counters"] = c.as_dict()
        return r


def tonemap(accum, sample_runs: int) -> np.ndarray:
    """program-raymarch.ts:295-316 display transform -> RGBA u8 [..., 4]."""
    acc = _f32(accum)
    npix = acc.size // 3
    out = np.zeros(npix * 4, np.uint8)
    _check(load_library().pt_tonemap(_ptr(acc), npix, sample_runs, _ptr(out)))
    return out.reshape(acc.shape[:-1] + (4,)) if acc.ndim >= 2 else out


def selftest_math(fn: str, a, b=None, device: int = 0) -> np.ndarray:
    a = _f32(a).reshape(-1)
    b = _f32(np.zeros_like(a) if b is None else b).reshape(-1)
    out = np.zeros_like(a)
    _check(load_library().pt_selftest_math(device, MATH_FNS.index(fn), _ptr(a), _ptr(b), _ptr(out), a.size))
    return out


def selftest_rcp(steps: int = -1, lo_bits: int = 0x00800000, hi_bits: int = 0x7E000000, device: int = 0):
    """(mismatches, failing input bits) of the core's reciprocal vs IEEE 1/x for every float whose
    magnitude bits lie in [lo_bits, hi_bits] (default 2^-126..2^125), both signs."""
    L = load_library()
    m = ctypes.c_uint64(0)
    b = ctypes.c_uint32(0)
    _check(L.pt_selftest_rcp(device, steps, lo_bits, hi_bits, ctypes.byref(m), ctypes.byref(b)))
    return int(m.value), int(b.value)


def selftest_view_half_h(metas) -> np.ndarray:
    """pt_selftest_view_half_h: the host's view_half_h for meta blocks [n, 48] (needs no GPU)."""
    metas = _f32(metas).reshape(-1, 48)
    out = np.zeros(len(metas), np.float32)
    _check(load_library().pt_selftest_view_half_h(_ptr(metas), len(metas), _ptr(out)))
    return out


def selftest_valu(iters: int = 20000, reps: int = 5, packed: int = 0, device: int = 0):
    """pt_selftest_valu: (ms of the timed launches, FMA wave-instructions they issued; packed 1:
    v_pk_fma_f32, 2: packed and plain chains interleaved)."""
    ms = ctypes.c_double(0.0)
    n = ctypes.c_uint64(0)
    _check(load_library().pt_selftest_valu(device, iters, reps, int(packed), ctypes.byref(ms), ctypes.byref(n)))
    return float(ms.value), int(n.value)


def bvh_build_lbvh(triangle_data, max_leaf: int = 4, isolate_emitters: bool = True) -> np.ndarray:
    """pt_bvh_build_lbvh: the LBVH of include/pt_hip.h over the records of a packed triangle_data, built on
    the host (no GPU) -> packed bvh_data (f32).  Scene.from_mesh builds the same tree on the device."""
    L = load_library()
    t = _f32(triangle_data)
    prm = _build_params(max_leaf, isolate_emitters)
    n = ctypes.c_size_t(0)
    _check(L.pt_bvh_build_lbvh(_ptr(t), t.size, ctypes.byref(prm), None, 0, ctypes.byref(n)))
    out = np.empty(n.value, np.float32)
    _check(L.pt_bvh_build_lbvh(_ptr(t), t.size, ctypes.byref(prm), _ptr(out), out.size, ctypes.byref(n)))
    return out


def bvh_build(vertices, tris, sah: bool = False, isolate=None) -> np.ndarray:
    """Native BVH build + pack (host only, no GPU): vertices f64 [n, 3] (post-CTM), tris
    int32 [m, 4] = (i0, i1, i2, material) with 1-based vertex indices -> packed bvh_data (f32).
    sah=True: the fast binned-SAH tree (pt_bvh_build_sah), same layout, not the reference's tree;
    isolate: per material id a flag (the emitters) — their triangles go under the root's left child
    (pt_bvh_build_sah2)."""
    L = load_library()
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1)
    if sah and isolate is not None:
        iso = np.ascontiguousarray(isolate, dtype=np.uint8).reshape(-1)

        def fn(vp, nv, tp, nt, op, cap, nref):
            return L.pt_bvh_build_sah2(vp, nv, tp, nt, _ptr(iso), iso.size, op, cap, nref)
    else:
        fn = L.pt_bvh_build_sah if sah else L.pt_bvh_build
    n = ctypes.c_size_t(0)
    _check(fn(_ptr(v), v.size // 3, _ptr(t), t.size // 4, None, 0, ctypes.byref(n)))
    out = np.empty(n.value, np.float32)
    _check(fn(_ptr(v), v.size // 3, _ptr(t), t.size // 4, _ptr(out), out.size, ctypes.byref(n)))
    return out
