"""numpy reference of temporal accumulation (include/pt_hip.h: pt_reproject, pt_denoise_mean,
pt_history_step), shared by test_temporal_cpu.py, test_gpu_temporal.py and test_gpu_node_temporal.py.

The header is restated operation by operation on whole images: f32, every operation rounded once, fmaf
exactly where the header writes it, numpy's correctly rounded f32 division and sqrt.  The pixel-centre ray
follows denoise_ref.camera_ray's pattern without the hashes (the jitter is (0.5, 0.5)); view_half_h is the
oracle's.  fmaf is vectorised: the product of two f32 is exact in f64, the sum is rounded to odd in f64 (the
exact error from a two-sum decides the sticky bit) and then once to f32 — 53 >= 2 * 24 + 2 bits make that the
correctly rounded result; test_temporal_cpu.py checks it against libm's fmaf.  The library's results are
compared with these bit for bit."""
import ctypes

import numpy as np

import denoise_ref as dr
import oracle

F = np.float32
D = np.float64
DEFAULTS = dict(alpha=0.2, normal_min=0.9, depth_tol=0.1, max_history=64.0)


def fmaf(a, b, c):
    """fmaf(a, b, c) elementwise for finite f32 arrays whose result does not overflow."""
    a, b, c = (np.asarray(v, F).astype(D) for v in (a, b, c))
    p = a * b  # exact
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # exact: p + c = s + err
    even = (np.atleast_1d(s).view(np.int64) & 1) == 0
    even = even.reshape(np.shape(s))
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))  # the inexact sum's other neighbour
    with np.errstate(all="ignore"):
        return np.where((err != 0) & even, odd, s).astype(F)


def view_half_h(meta):
    meta = np.ascontiguousarray(meta, F)
    return F(oracle.lib().po_view_half_h(meta.ctypes.data_as(ctypes.c_void_p)))


def warp(meta, prev_meta, Z):
    """Steps 2 and 3 for every pixel of the image with mean hit distance Z [h, w]: (u, v, zc, Ze) — where the
    pixel's surface point lies in the previous image, whether in front of its camera (zc > 0), how far from it."""
    meta, pm, Z = np.asarray(meta, F), np.asarray(prev_meta, F), np.asarray(Z, F)
    h, w = Z.shape
    with np.errstate(all="ignore"):
        # 2. the world point
        W, H, focal, inv_w, inv_h, aspect = meta[0], meta[1], meta[2], meta[8], meta[9], meta[10]
        cam, M = meta[4:8], meta[28:44]
        x = np.broadcast_to(np.arange(w, dtype=F)[None, :], (h, w))
        y = np.broadcast_to(np.arange(h, dtype=F)[:, None], (h, w))
        norm_x = fmaf(x + F(0.5), inv_w, F(-0.5))
        norm_y = fmaf(((H - F(1)) - y) + F(0.5), inv_h, F(-0.5))
        vhh = view_half_h(meta)
        vx, vy, pz = (vhh * aspect) * norm_x, vhh * norm_y, -focal
        one = np.ones((h, w), F)
        pw = [fmaf(M[12 + k], one, fmaf(M[8 + k], pz, fmaf(M[4 + k], vy, M[k] * vx))) for k in range(4)]
        d = [pw[k] - cam[k] for k in range(4)]
        ln = np.sqrt(fmaf(d[3], d[3], fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]))))
        P = [fmaf(Z, d[k] / ln, cam[k]) for k in range(3)]
        # 3. the previous camera
        V, pfocal, paspect, pcam, pvhh = pm[12:28], pm[2], pm[10], pm[4:7], view_half_h(pm)
        pc = [fmaf(V[12 + k], one, fmaf(V[8 + k], P[2], fmaf(V[4 + k], P[1], V[k] * P[0]))) for k in range(3)]
        zc = -pc[2]
        pvx, pvy = (pc[0] * pfocal) / zc, (pc[1] * pfocal) / zc
        u = ((pvx / (pvhh * paspect)) + F(0.5)) * W - F(0.5)
        v = (H - F(1)) - (((pvy / pvhh) + F(0.5)) * H - F(0.5))
        e = [P[k] - pcam[k] for k in range(3)]
        Ze = np.sqrt(fmaf(e[2], e[2], fmaf(e[1], e[1], e[0] * e[0])))
        for arr in (u, v, Ze):
            assert arr.dtype == F
        return u, v, zc, Ze


def reproject(acc, m2, n, geo, alb, meta, prev=None, **params):
    """One step: {"meta", "hist", "mom", "gbuf" [h, w, 4], "out" [h, w, 3], "var" [h, w]}; prev: None or the
    previous step's dict.  "taps" [h, w] is the reference's own: the count of the pixel's valid taps."""
    prm = {k: F(v) for k, v in {**DEFAULTS, **params}.items()}
    acc, m2, geo, alb, meta = (np.asarray(a, F) for a in (acc, m2, geo, alb, meta))
    h, w = acc.shape[:2]
    assert int(meta[0]) == w and int(meta[1]) == h
    fn = F(n)
    with np.errstate(all="ignore"):
        ck, qk = (acc / fn).astype(F), (m2 / fn).astype(F)
        hits = alb[..., 3]
        hit = hits > 0
        hd = np.where(hit, hits, F(1))
        Ncur = np.where(hit[..., None], geo[..., :3] / hd[..., None], F(0)).astype(F)
        Z = np.where(hit, geo[..., 3] / hd, F(0)).astype(F)
        c, q = ck.copy(), qk.copy()
        N1, a = np.ones((h, w), F), np.ones((h, w), F)
        taps = np.zeros((h, w), np.int64)
        if prev is not None:
            pm = np.asarray(prev["meta"], F)
            assert int(pm[0]) == w and int(pm[1]) == h
            hp, mp, gp = (np.asarray(prev[k], F) for k in ("hist", "mom", "gbuf"))
            W, H = meta[0], meta[1]
            u, v, zc, Ze = warp(meta, pm, Z)
            # 5. in float, before any index
            ok = (Z > 0) & (zc > 0) & (u > F(-1)) & (u < W) & (v > F(-1)) & (v < H)
            us, vs = np.where(ok, u, F(0)), np.where(ok, v, F(0))
            # 4. the taps
            fu, fv = np.floor(us), np.floor(vs)
            fx, fy = us - fu, vs - fv
            gx, gy = F(1) - fx, F(1) - fy
            x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
            tol = prm["depth_tol"] * Ze
            sw, sn = np.zeros((h, w), F), np.zeros((h, w), F)
            sc, sq = np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    inside = ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                    ix, iy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    hq, mq, gq = hp[iy, ix], mp[iy, ix], gp[iy, ix]
                    dt = (Ncur[..., 0] * gq[..., 0] + Ncur[..., 1] * gq[..., 1]) + Ncur[..., 2] * gq[..., 2]
                    valid = inside & (hq[..., 3] > 0) & (gq[..., 3] > 0) & (np.abs(gq[..., 3] - Ze) <= tol) & \
                        (dt >= prm["normal_min"])
                    wgt = (fx if i else gx) * (fy if j else gy)
                    sw = np.where(valid, sw + wgt, sw)
                    sc = np.where(valid[..., None], sc + wgt[..., None] * hq[..., :3], sc)
                    sq = np.where(valid[..., None], sq + wgt[..., None] * mq[..., :3], sq)
                    sn = np.where(valid, sn + wgt * hq[..., 3], sn)
                    taps = taps + valid
            use = ok & (sw > F(1e-6))
            # 6. the blend
            sws = np.where(use, sw, F(1))
            ch, qh = sc / sws[..., None], sq / sws[..., None]
            t = sn / sws + F(1)
            Nn = np.where(t < prm["max_history"], t, prm["max_history"]).astype(F)
            r = F(1) / Nn
            ab = np.where(prm["alpha"] > r, prm["alpha"], r).astype(F)
            cb = ch + ab[..., None] * (ck - ch)
            qb = qh + ab[..., None] * (qk - qh)
            c = np.where(use[..., None], cb, ck).astype(F)
            q = np.where(use[..., None], qb, qk).astype(F)
            N1 = np.where(use, Nn, F(1)).astype(F)
            a = np.where(use, ab, F(1)).astype(F)
        # 7. the outputs
        dv = q - c * c
        vv = np.where(dv > 0, dv, F(0)).astype(F)
        var = (((vv[..., 0] + vv[..., 1]) + vv[..., 2]) * a) / fn
        var = np.where(var == var, var, F(0)).astype(F)
    zero = np.zeros((h, w, 1), F)
    res = {"meta": meta.copy(), "hist": np.concatenate([c, N1[..., None]], axis=2).astype(F),
           "mom": np.concatenate([q, zero], axis=2).astype(F),
           "gbuf": np.concatenate([Ncur, Z[..., None]], axis=2).astype(F), "out": c.astype(F), "var": var,
           "taps": taps}  # not the library's: how many of the pixel's four taps were valid (0 without a previous set)
    for k in ("hist", "mom", "gbuf", "out", "var"):
        assert res[k].dtype == F
    return res


def denoise_mean(c, var, geo, alb, feature_frames, **params):
    """pt_denoise_mean: denoise_ref's passes from a given mean and variance of the mean."""
    p = {**dr.DEFAULTS, **params}
    geo, alb = np.asarray(geo, F), np.asarray(alb, F)
    nf = F(feature_frames)
    with np.errstate(all="ignore"):
        N, Z, A = (geo[..., :3] / nf).astype(F), (geo[..., 3] / nf).astype(F), (alb[..., :3] / nf).astype(F)
    c, var = np.asarray(c, F), np.asarray(var, F)
    k = dr.constants(p["sigma_n"], p["sigma_a"], p["sigma_z"], p["sigma_l"])
    for i in range(p["iters"]):
        c, var = dr.atrous_pass(c, var, N, Z, A, 1 << i, *k)
    return c, var

