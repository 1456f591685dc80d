"""numpy references of the guide buffers and the denoiser (include/pt_hip.h: pt_render_features,
pt_denoise, pt_render_denoised_image), shared by test_denoise_cpu.py, test_gpu_features.py,
test_gpu_denoise.py and test_gpu_node_denoise.py.

The camera ray is restated from the oracle's pixel_sample (oracle/pt_oracle.c) with the oracle's own
hashes and view_half_h, C fmaf from libm and numpy's correctly rounded f32 sqrt and division; the hit
is oracle.intersect's.  The filter restates the header operation by operation: f32, every operation
rounded once, no FMA, the variance in double, exp2 the oracle's pinned one.  The library's results are
compared with these bit for bit."""
import ctypes

import numpy as np

import oracle

F = np.float32
DEFAULTS = dict(iters=4, sigma_n=0.5, sigma_a=0.3, sigma_z=0.1, sigma_l=4.0)
_M32 = 0xFFFFFFFF

_libm = ctypes.CDLL("libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def fmaf(a, b, c):
    return F(_libm.fmaf(float(a), float(b), float(c)))


def camera_ray(meta, x, y, t):
    """(origin[4], direction[4]) of pixel (x, y) for salt t: pixel_sample up to the ray."""
    meta = np.ascontiguousarray(meta, F)
    W, H, focal = meta[0], meta[1], meta[2]
    cam, inv_w, inv_h, aspect, M = meta[4:8], meta[8], meta[9], meta[10], meta[28:44]
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
    pp = (vhw * norm_x, vhh * norm_y, -focal, F(1.0))
    pw = [fmaf(M[12 + k], pp[3], fmaf(M[8 + k], pp[2], fmaf(M[4 + k], pp[1], M[k] * pp[0]))) for k in range(4)]
    d = [pw[k] - cam[k] for k in range(4)]
    ln = np.sqrt(fmaf(d[3], d[3], fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]))))
    return np.array(cam, F), np.array([v / ln for v in d], F)


def albedo(tri, mat_id):
    """Ke where (Ke.r + Ke.g) + Ke.b > 0, else Kd + Ks; also whether the material emits."""
    m = int(tri[4]) + 15 * int(mat_id)
    kd, ks, ke = tri[m + 6:m + 9], tri[m + 9:m + 12], tri[m + 12:m + 15]
    emits = bool((ke[0] + ke[1]) + ke[2] > 0)
    return (ke.copy() if emits else kd + ks), emits


class FirstHits:
    """The first hit of (pixel, frame) of one scene and camera, memoised: (normal[3], t, albedo[3],
    emits, counters) or None for a miss (with its counters).  Honours oracle.set_vertex_normals as set
    when a hit is first asked for: keep one object per mode."""

    def __init__(self, tri, bvh, meta):
        self.tri, self.bvh, self.meta = (np.ascontiguousarray(a, F) for a in (tri, bvh, meta))
        self._memo = {}

    def hit(self, x, y, k):
        key = (x, y, k)
        if key not in self._memo:
            t = int(F(k)) & _M32  # the salt u32(f32(k))
            o, d = camera_ray(self.meta, x, y, t)
            ok, out, cnt = oracle.intersect(self.tri, self.bvh, o, d)
            if ok:
                a, emits = albedo(self.tri, out[7])
                self._memo[key] = (out[3:6].copy(), F(out[6]), a, emits, cnt)
            else:
                self._memo[key] = (None, None, None, False, cnt)
        return self._memo[key]

    def features(self, win, frame0, nframes, stride, geo=None, alb=None):
        """pt_render_features of window win = (x0, y0, w, h): (geo, alb [h, w, 4], counters)."""
        x0, y0, w, h = win
        geo = np.zeros((h, w, 4), F) if geo is None else np.array(geo, F)
        alb = np.zeros((h, w, 4), F) if alb is None else np.array(alb, F)
        cnt = dict(samples=0, ext_queries=0, shadow_queries=0, nodes=0, tri_tests=0, box_tests=0)
        for j in range(h):
            for i in range(w):
                for f in range(nframes):
                    n, t, a, _, c = self.hit(x0 + i, y0 + j, frame0 + f * stride)
                    cnt["samples"] += 1
                    cnt["ext_queries"] += 1
                    for key in ("nodes", "tri_tests", "box_tests"):
                        cnt[key] += c[key]
                    if n is None:
                        continue
                    geo[j, i, :3] = geo[j, i, :3] + n
                    geo[j, i, 3] = geo[j, i, 3] + t
                    alb[j, i, :3] = alb[j, i, :3] + a
                    alb[j, i, 3] = alb[j, i, 3] + F(1.0)
        return geo, alb, cnt


_FIRST_HITS = {}


def first_hits(scene, packed, w, h, vertex_normals=False):
    """The FirstHits of a packed scene (conftest.Packed) at w x h, one per (scene, size, normal mode)
    for the whole session.  vertex_normals: the caller switches the oracle (oracle.set_vertex_normals)
    around every use of the object."""
    key = (scene, w, h, bool(vertex_normals))
    if key not in _FIRST_HITS:
        _FIRST_HITS[key] = FirstHits(packed.triangle_data, packed.bvh_data, packed.meta_for(w, h))
    return _FIRST_HITS[key]


def exp2(x):
    """The pinned exp2 of every element (each distinct value evaluated once)."""
    u, inv = np.unique(np.asarray(x, F).ravel(), return_inverse=True)
    return oracle.math_fn("exp2", u)[inv].reshape(np.shape(x))


def frames_of_pixels(frames, w, h, tile):
    tw, th = tile
    f = np.asarray(frames, np.uint32).reshape(-(-h // th), -(-w // tw))
    return np.repeat(np.repeat(f, th, axis=0), tw, axis=1)[:h, :w]


def prepare(acc, m2, n, geo, alb, feature_frames):
    """c [h, w, 3], var [h, w], N [h, w, 3], Z [h, w], A [h, w, 3]; n: [h, w] frames per pixel."""
    acc, m2, geo, alb = (np.asarray(a, F) for a in (acc, m2, geo, alb))
    n = np.asarray(n, np.uint32)
    with np.errstate(all="ignore"):
        c = np.where(n[..., None] > 0, acc / n.astype(F)[..., None], F(0)).astype(F)
        S, Q, nd = acc.astype(np.float64), m2.astype(np.float64), n.astype(np.float64)
        d = Q - (S * S) / nd[..., None]
        v = np.where(d > 0, d, 0.0)
        V = (v[..., 0] + v[..., 1]) + v[..., 2]
        var = np.where(n >= 2, (V / (nd * (nd - 1))).astype(F), F(0)).astype(F)
        nf = F(feature_frames)
        return c, var, (geo[..., :3] / nf).astype(F), (geo[..., 3] / nf).astype(F), (alb[..., :3] / nf).astype(F)


def constants(sigma_n, sigma_a, sigma_z, sigma_l):
    """isn, isa, isz (double, rounded once) and sigma_l, from the f32 values the library is given."""
    sn, sa, sz = (float(F(s)) for s in (sigma_n, sigma_a, sigma_z))
    return F(1.0 / (sn * sn)), F(1.0 / (sa * sa)), F(1.0 / sz), F(sigma_l)


def atrous_pass(c, var, N, Z, A, s, isn, isa, isz, sigma_l):
    h, w = var.shape
    hk = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F)
    with np.errstate(all="ignore"):
        lum = (c[..., 0] + c[..., 1]) + c[..., 2]
        den = sigma_l * np.sqrt(var) + F(1e-6)
        sw, sc, sv = np.zeros((h, w), F), np.zeros((h, w, 3), F), np.zeros((h, w), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                ya, yb, xa, xb = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                if ya >= yb or xa >= xb:
                    continue
                P = (slice(ya, yb), slice(xa, xb))
                Q = (slice(ya + oy, yb + oy), slice(xa + ox, xb + ox))
                dN = N[P] - N[Q]
                tn = ((dN[..., 0] * dN[..., 0] + dN[..., 1] * dN[..., 1]) + dN[..., 2] * dN[..., 2]) * isn
                dA = A[P] - A[Q]
                ta = ((dA[..., 0] * dA[..., 0] + dA[..., 1] * dA[..., 1]) + dA[..., 2] * dA[..., 2]) * isa
                zs = Z[P] + Z[Q]
                tz = (np.abs(Z[P] - Z[Q]) / np.where(zs > F(1e-6), zs, F(1e-6))) * isz
                tl = np.abs(lum[P] - lum[Q]) / den[P]
                e = (tn + ta) + (tz + tl)
                e = np.where(e < F(126), e, F(126)).astype(F)
                wgt = (hk[dy + 2] * hk[dx + 2]) * exp2(-e)
                assert wgt.dtype == F
                sw[P] = sw[P] + wgt
                sc[P] = sc[P] + wgt[..., None] * c[Q]
                sv[P] = sv[P] + (wgt * wgt) * var[Q]
        return (sc / sw[..., None]).astype(F), (sv / (sw * sw)).astype(F)


def denoise_passes(acc, m2, frames, geo, alb, feature_frames, tile=None, iters=5, sigma_n=0.5, sigma_a=0.3, sigma_z=0.1,
                   sigma_l=4.0):
    """[(out, var) after pass 1, 2, ..., iters]: pass i's result is pt_denoise's with iters = i."""
    h, w = np.shape(acc)[:2]
    n = frames_of_pixels(frames, w, h, (w, h) if tile is None else tile)
    c, var, N, Z, A = prepare(acc, m2, n, geo, alb, feature_frames)
    k = constants(sigma_n, sigma_a, sigma_z, sigma_l)
    res = []
    for i in range(iters):
        c, var = atrous_pass(c, var, N, Z, A, 1 << i, *k)
        res.append((c, var))
    return res


def denoise(acc, m2, frames, geo, alb, feature_frames, tile=None, **params):
    p = {**DEFAULTS, **params}
    return denoise_passes(acc, m2, frames, geo, alb, feature_frames, tile, **p)[-1]


def rel_mse(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))
