"""GPU: temporal accumulation (pt_reproject, pt_reproject_async, pt_denoise_mean, pt_history_*) against the
numpy reference (temporal_ref.py): all three planes, out and var bit for bit.

Rendered inputs: 37x29 (no multiple of 8 or 16 either way), the library's own render_moments and
render_features (the oracle covers them elsewhere), three chained steps per camera sequence, so step 3 reads
the planes step 2 wrote.  Synthetic planes: 16x8 and 37x29, built in numpy so that single pixels sit on, just
below and just above every threshold of the header."""
import functools
import math

import numpy as np
import pytest

import cam_cases as cc
import denoise_ref as dr
import pt_amd
import temporal_ref as tr
from test_gpu_parity import mismatch_report, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 37, 29
DEPTH, N, FF = 8, 2, 2
POS, FOCUS = cc.CORNELL_POS, cc.CORNELL_FOCUS
KEYS = ("hist", "mom", "gbuf", "out", "var")


def yawed(deg):
    """The scenes' camera turned about its own position by deg degrees (one pixel is 45 / 29 = 1.55 degrees)."""
    a = math.radians(deg)
    return cc.cam(POS, (POS[0] - 3.6 * math.sin(a), 1.0, POS[2] - 3.6 * math.cos(a)))


def shifted(dx, dy=0.0):
    return cc.cam((POS[0] + dx, POS[1] + dy, POS[2]), (FOCUS[0] + dx, FOCUS[1] + dy, FOCUS[2]))


BASE = cc.cam(POS, FOCUS)
AWAY = cc.cam(POS, (0, 1, 8))                      # turned by 180 degrees: sees nothing, and zc <= 0 for what BASE sees
PULLED = cc.cam((2.5, 1.6, 8.0), (-2.0, 1.0, 0))   # pulled back and turned: a part of the image misses the scene
# name -> the three cameras of the chained steps
SEQUENCES = {
    "identical": [BASE, BASE, BASE],
    "yaw": [BASE, yawed(1.5), yawed(3.0)],
    "translate": [BASE, shifted(0.9, 0.35), shifted(1.8, 0.7)],  # a band leaves the previous image on two sides
    "turned": [AWAY, BASE, BASE],
    "pulled": [BASE, PULLED, BASE],
}
SCENES_ = ["CornellBox", "CornellBox-Sphere"]


def check(got, ref, what):
    for k in KEYS:
        assert np.all(np.isfinite(ref[k])), (what, k)
        assert same_bits(got[k], ref[k]), f"{what} {k}: " + mismatch_report(got[k], ref[k])


def render_inputs(s, meta, k):
    """Step k's inputs from the library: the moments of frames k N .. k N + N - 1 and the guides of the same frames."""
    acc, m2 = s.render_moments(meta, k * N, N, 1, DEPTH)
    geo, alb = s.render_features(meta, k * N, FF)
    return acc, m2, geo, alb


@pytest.mark.parametrize("seq", list(SEQUENCES))
@pytest.mark.parametrize("scene", SCENES_)
def test_reproject_rendered_inputs_bitexact(packed, ptopts, scene, seq):
    p = packed[scene]
    metas = [cc.meta_from(c, W, H) for c in SEQUENCES[seq]]
    got = ref = None
    stats, counts = [], []
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for k, meta in enumerate(metas):
            acc, m2, geo, alb = render_inputs(s, meta, k)
            got = s.reproject(acc, m2, N, geo, alb, meta, prev=got)
            ref = tr.reproject(acc, m2, N, geo, alb, meta, prev=ref)
            check(got, ref, f"{scene} {seq} step {k}")
            hit = ref["gbuf"][..., 3] > 0
            stats.append((float(hit.mean()), float((ref["hist"][..., 3][hit] > 1).mean()) if hit.any() else 0.0))
            counts.append(np.bincount(ref["taps"][hit], minlength=5).tolist())
    print(f"{scene} {seq}: (hit fraction, fraction of the hits with history) per step {stats}; hit pixels with 0..4 valid taps "
          f"per step {counts}")
    # the sequence does what its name says (of the reference: the library has its bits)
    assert stats[0][1] == 0.0  # a first step has no history
    if seq == "identical":
        assert stats[1][1] > 0.6 and stats[2][1] > 0.6 and ref["hist"][..., 3].max() == 3
    elif seq == "yaw":
        assert stats[1][1] > 0.5 and stats[2][1] > 0.5
    elif seq == "translate":
        assert 0.2 < stats[1][1] < 0.95 and 0.2 < stats[2][1] < 0.95  # a band has none
        for k in (1, 2):  # and pixels with 0, 1, 2, 3 and 4 valid taps all occur, in each of the two steps
            assert min(counts[k]) >= 1, (k, counts[k])
    elif seq == "turned":
        assert stats[0][0] == 0.0 and stats[1][0] > 0.5 and stats[1][1] == 0.0 and stats[2][1] > 0.6
    elif seq == "pulled":
        assert 0.05 < stats[1][0] < 0.9 and stats[1][1] > 0.1 and stats[2][1] > 0.1
    assert ref["var"].max() > 0 and ref["out"].max() > 0


@functools.lru_cache(maxsize=None)
def _noisy_buffers(w, h):
    rng = np.random.default_rng(10 * w + h)
    mean = rng.uniform(0.05, 2.0, (h, w, 3)).astype(F)
    acc = (mean * F(N)).astype(F)
    m2 = (mean * mean * F(N) * rng.uniform(1.0, 1.5, (h, w, 3)).astype(F)).astype(F)
    return acc, m2


def test_reproject_async_pitched_on_a_stream(packed, ptopts):
    """37 columns inside 48-wide device buffers on a non-default stream: nothing right of the 37 columns is read
    (NaN in the inputs there) or written (a sentinel in the outputs), two chained steps."""
    torch = pytest.importorskip("torch")
    p = packed["CornellBox"]
    pitch, sentinel = 48, -12345.5
    metas = [cc.meta_from(c, W, H) for c in (BASE, yawed(1.5))]

    def padded(a, fill):
        b = np.full((H, pitch) + a.shape[2:], fill, F)
        b[:, :W] = a
        return torch.from_numpy(b).cuda()

    def fresh(k):
        return torch.full((H, pitch, k) if k > 1 else (H, pitch), sentinel, dtype=torch.float32, device="cuda")

    st = torch.cuda.Stream()
    ref, dprev = None, None
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for k, meta in enumerate(metas):
            acc, m2, geo, alb = render_inputs(s, meta, k)
            ref = tr.reproject(acc, m2, N, geo, alb, meta, prev=ref)
            d_in = [padded(a, np.nan) for a in (acc, m2, geo, alb)]
            d_new = [fresh(4) for _ in range(3)]
            d_out, d_var = fresh(3), fresh(1)
            torch.cuda.synchronize()
            prev = {} if dprev is None else dict(meta_prev=metas[k - 1], d_hist_prev_ptr=dprev[0].data_ptr(),
                                                 d_mom_prev_ptr=dprev[1].data_ptr(), d_gbuf_prev_ptr=dprev[2].data_ptr())
            s.reproject_async(d_in[0].data_ptr(), d_in[1].data_ptr(), N, d_in[2].data_ptr(), d_in[3].data_ptr(), meta, W, H,
                              d_new[0].data_ptr(), d_new[1].data_ptr(), d_new[2].data_ptr(), d_out_ptr=d_out.data_ptr(),
                              d_var_ptr=d_var.data_ptr(), row_pitch=pitch, stream_ptr=st.cuda_stream, **prev)
            st.synchronize()
            s.check()
            host = dict(zip(KEYS, [t.cpu().numpy() for t in d_new + [d_out, d_var]]))
            check({k_: v[:, :W] for k_, v in host.items()}, ref, f"pitched step {k}")
            for k_, v in host.items():
                assert np.all(v[:, W:] == F(sentinel)), k_
            dprev = d_new


@pytest.mark.parametrize("lds", [0, 2, 4])
@pytest.mark.parametrize("iters", [1, 4])
def test_denoise_mean_is_denoise_on_its_prepared_inputs(packed, ptopts, iters, lds):
    p = packed["CornellBox"]
    meta = cc.meta_from(BASE, W, H)
    ptopts.set("denoise_lds", lds)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        acc, m2 = s.render_moments(meta, 0, 8, 1, DEPTH)
        geo, alb = s.render_features(meta, 0, 4)
        c, var = dr.prepare(acc, m2, np.full((H, W), 8, np.uint32), geo, alb, 4)[:2]
        want = s.denoise(acc, m2, geo, alb, 4, 8, params=dict(iters=iters))
        got = s.denoise_mean(c, var, geo, alb, 4, params=dict(iters=iters))
    assert var.max() > 0 and not same_bits(got[0], c)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    ref = tr.denoise_mean(c, var, geo, alb, 4, iters=iters)
    assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1])


@pytest.mark.parametrize("filtered", [False, True], ids=["unfiltered", "filtered"])
def test_history_steps_are_the_raw_calls_composed(packed, ptopts, filtered):
    p = packed["CornellBox"]
    metas = [cc.meta_from(c, W, H) for c in SEQUENCES["yaw"]]
    dn = dict(iters=2) if filtered else None
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        before = s.info["device_bytes"]
        with pt_amd.History(s, W, H) as hist:
            held = s.info["device_bytes"] - before
            steps = [hist.step(meta, k * N, N, 1, DEPTH, feature_frames=FF, denoise=dn, counters=True) for k, meta in enumerate(metas)]
            hist.reset()
            again = hist.step(metas[0], 0, N, 1, DEPTH, feature_frames=FF, denoise=dn)
            held_after = s.info["device_bytes"] - before
        after_close = s.info["device_bytes"]
        prev = None
        for k, meta in enumerate(metas):
            acc, m2, geo, alb = render_inputs(s, meta, k)
            prev = s.reproject(acc, m2, N, geo, alb, meta, prev=prev)
            mean, var = s.denoise_mean(prev["out"], prev["var"], geo, alb, FF, params=dn) if filtered else (prev["out"], prev["var"])
            got = steps[k]
            assert got["mean"].tobytes() == mean.tobytes(), k
            assert got["var"].tobytes() == var.tobytes(), k
            assert got["rgba"].tobytes() == pt_amd.tonemap(mean, 1).tobytes(), k
            assert got["history_len"].tobytes() == np.ascontiguousarray(prev["hist"][..., 3]).tobytes(), k
            assert got["counters"]["samples"] == W * H * (N + FF)
        assert steps[2]["history_len"].max() == 3 and steps[2]["mean"].max() > 0
    # reset(): the next step is a first step
    for k in ("mean", "var", "rgba", "history_len"):
        assert again[k].tobytes() == steps[0][k].tobytes(), k
    assert np.all(again["history_len"] == 1)
    # the history's buffers are the scene's while it lives: six planes, the step's 22 floats, the image; the
    # filter's four planes belong to the scene and stay
    assert held >= (6 * 16 + 22 * 4 + 4) * W * H and held_after >= held
    assert after_close == before + (4 * 16 * W * H if filtered else 0)


def test_history_outlives_its_scene_without_a_fault(packed, ptopts):
    p = packed["CornellBox"]
    meta = cc.meta_from(BASE, W, H)
    s = pt_amd.Scene(p.triangle_data, p.bvh_data)
    hist = pt_amd.History(s, W, H)
    hist.step(meta, 0, N, 1, DEPTH, feature_frames=FF)
    s.close()
    for call in (lambda: hist.step(meta, N, N, 1, DEPTH, feature_frames=FF), hist.reset):
        with pytest.raises(pt_amd.PtError) as e:
            call()
        assert e.value.code == -1 and "destroyed" in str(e.value)
    hist.close()


# ---------------------------------------------------------------------------------------------
# synthetic planes: single pixels on, just below and just above every threshold
# ---------------------------------------------------------------------------------------------
TH = dict(alpha=0.2, normal_min=0.9, depth_tol=0.125, max_history=9.0)  # depth_tol a power of two: tol = Ze / 8 exactly
LOOSE = dict(alpha=0.2, normal_min=-1.0, depth_tol=1000.0, max_history=64.0)  # every tap with N_q > 0 and Z_q > 0 is valid
CASES = ("depth_on", "depth_in", "depth_out", "normal_on", "normal_below", "normal_above", "len_at", "len_below", "len_above",
         "len_short")


def _current(w, h, Z):
    """Inputs of a step whose pixels all hit twice, with normal (0, 0, 1) exactly and mean distance Z."""
    acc, m2 = _noisy_buffers(w, h)
    geo = np.zeros((h, w, 4), F)
    geo[..., 2] = 2
    geo[..., 3] = Z * F(2)
    alb = np.full((h, w, 4), 2, F)
    return acc, m2, geo, alb


def _prev_planes(w, h, Zq, Nq=4.0, nz=1.0):
    rng = np.random.default_rng(w + 100 * h)
    c = rng.uniform(0.05, 2.0, (h, w, 3)).astype(F)
    q = (c * c * rng.uniform(1.0, 1.5, (h, w, 3)).astype(F)).astype(F)
    one = np.ones((h, w), F)
    return dict(hist=np.dstack([c, one * F(Nq)]).astype(F), mom=np.dstack([q, 0 * one]).astype(F),
                gbuf=np.dstack([0 * one, 0 * one, one * F(nz), np.asarray(Zq, F) * one]).astype(F))


@functools.lru_cache(maxsize=None)
def threshold_case(w, h):
    """A static camera; every third pixel both ways is a case of CASES, and the 3 x 3 pixels around it — all it
    can tap — hold the previous values that put it there.  Returns (inputs, prev, {case: [(x, y)]})."""
    meta = cc.meta_from(BASE, w, h)
    rng = np.random.default_rng(7 * w + h)
    cand = rng.uniform(2.0, 6.0, (64, h, w)).astype(F)
    Ze_c = np.stack([tr.warp(meta, meta, z)[3] for z in cand])
    tol_c = F(0.125) * Ze_c
    exact = (Ze_c + tol_c).astype(np.float64) == Ze_c.astype(np.float64) + tol_c.astype(np.float64)  # Ze + tol is an f32
    Z = cand[0].copy()
    where = {c: [] for c in CASES}
    cells = [(x, y) for y in range(1, h, 3) for x in range(1, w, 3)]
    for i, (x, y) in enumerate(cells):
        case = CASES[i % len(CASES)]
        if case == "depth_on":
            ks = np.flatnonzero(exact[:, y, x])
            if not len(ks):
                case = "depth_in"
            else:
                Z[y, x] = cand[ks[0], y, x]
        where[case].append((x, y))
    Ze = tr.warp(meta, meta, Z)[3]
    tol = F(0.125) * Ze
    prev = _prev_planes(w, h, 1.0)
    for case, pix in where.items():
        for x, y in pix:
            zq, nq, nz = Ze[y, x], F(4), F(1)
            if case.startswith("depth"):
                c = Ze[y, x] + tol[y, x]
                around = [c]
                for _ in range(3):
                    around = [np.nextafter(around[0], F(0))] + around + [np.nextafter(around[-1], F(np.inf))]
                d = [np.abs(a - Ze[y, x]) for a in around]
                if case == "depth_on":
                    zq = [a for a, dd in zip(around, d) if dd == tol[y, x]][0]
                elif case == "depth_in":
                    zq = max(a for a, dd in zip(around, d) if dd < tol[y, x])
                else:
                    zq = min(a for a, dd in zip(around, d) if dd > tol[y, x])
            elif case.startswith("normal"):
                t = F(TH["normal_min"])
                nz = {"normal_on": t, "normal_below": np.nextafter(t, F(0)), "normal_above": np.nextafter(t, F(1))}[case]
            else:
                nq = F({"len_at": 8, "len_below": 4, "len_above": 16, "len_short": 2}[case])
            ys, xs = slice(max(y - 1, 0), y + 2), slice(max(x - 1, 0), x + 2)
            prev["gbuf"][ys, xs, 3] = zq
            prev["gbuf"][ys, xs, 2] = nz
            prev["hist"][ys, xs, 3] = nq
    prev["meta"] = meta
    return _current(w, h, Z) + (meta,), prev, where


@pytest.mark.parametrize("size", [(16, 8), (37, 29)], ids=["16x8", "37x29"])
def test_reproject_synthetic_thresholds_bitexact(packed, ptopts, size):
    w, h = size
    p = packed["CornellBox"]
    (acc, m2, geo, alb, meta), prev, where = threshold_case(w, h)
    ref = tr.reproject(acc, m2, N, geo, alb, meta, prev=prev, **TH)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        got = s.reproject(acc, m2, N, geo, alb, meta, prev=prev, params=TH)
    check(got, ref, f"thresholds {w}x{h}")
    # the reference takes the branch each case is named for
    Nn = ref["hist"][..., 3]
    want = dict(depth_on=5, depth_in=5, depth_out=1, normal_on=5, normal_below=1, normal_above=5, len_at=9, len_below=5,
                len_above=9, len_short=3)
    print({c: len(v) for c, v in where.items()})
    for case, pix in where.items():
        assert pix or (case == "depth_on" and w * h < 200), case
        for x, y in pix:
            assert Nn[y, x] == want[case], (case, x, y, Nn[y, x])
    assert where["depth_on"] or w < 37
    # alpha at, below and above 1 / N': N' = 5 has 1 / N' == alpha exactly, 3 is above it, 9 below
    assert F(1) / F(5) == F(TH["alpha"])


def _bisect(make, pred, lo, hi):
    """Adjacent f32 values a < b (or a > b) between lo and hi with pred(make(a)) false and pred(make(b)) true."""
    lo, hi = F(lo), F(hi)
    assert not pred(make(lo)) and pred(make(hi))
    while np.nextafter(lo, hi) != hi:
        mid = F((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            mid = np.nextafter(lo, hi)
        if pred(make(mid)):
            hi = mid
        else:
            lo = mid
    return lo, hi


@functools.lru_cache(maxsize=None)
def edge_cases(w, h):
    """Previous cameras, the current one moved along its x or y axis, that put the surface point of pixel (tx, ty)
    at u or v on either side of -1, W and H — exactly on the bound where some mean distance Z of ZS allows it — and
    far outside; and one where the only valid tap's weight straddles 1e-6.
    [(name, inputs, prev dict, (tx, ty), None | whether the pixel has history, (u, v))]"""
    meta = cc.meta_from(BASE, w, h)
    tx, ty = 3, 2
    base12, base13 = meta[12 + 12], meta[12 + 13]
    ZS = [3.5, 3.0, 4.0, 2.5, 3.25, 3.75, 2.75, 4.5, 2.25, 5.0, 3.125, 3.375]

    def moved(v12=None, v13=None):
        m = meta.copy()
        if v12 is not None:
            m[24] = v12
        if v13 is not None:
            m[25] = v13
        return m

    def at(m, Z):
        u, v, zc, _ = tr.warp(meta, m, np.full((h, w), Z, F))
        return u[ty, tx], v[ty, tx]

    out = []
    planes = lambda Z: _prev_planes(w, h, Z)
    inputs = lambda Z: _current(w, h, np.full((h, w), Z, F)) + (meta,)
    # (name, the meta word moved, the predicate that turns true across the bound, the bound's side that is out of range)
    for name, axis, pred, bound, out_when in (("u>-1", 12, lambda uv: uv[0] > F(-1), -1.0, False), ("u>=W", 12, lambda uv: uv[0] >= F(w), w, True),
                                             ("v<H", 13, lambda uv: uv[1] < F(h), h, False), ("v<=-1", 13, lambda uv: uv[1] <= F(-1), -1.0, True)):
        mk = (lambda t: moved(v12=t)) if axis == 12 else (lambda t: moved(v13=t))
        b = base12 if axis == 12 else base13
        for Z in ZS:
            P = lambda m: pred(at(m, Z))
            ends = (b - 30, b + 30) if not P(mk(F(b - 30))) else (b + 30, b - 30)
            a, c = _bisect(mk, P, *ends)
            on = at(mk(c if out_when else a), Z)[0 if axis == 12 else 1]
            if on == F(bound):
                break
        for t, holds in ((a, False), (c, True)):
            out.append((f"{name} {'true' if holds else 'false'}", inputs(Z), dict(planes(Z), meta=mk(t)), (tx, ty),
                        False if holds == out_when else None, at(mk(t), Z)))
    Z = ZS[0]
    for t in (1e30, -3e38):
        out.append((f"huge {t}", inputs(Z), dict(planes(Z), meta=moved(v12=F(t))), (tx, ty), False, at(moved(v12=F(t)), Z)))
    # sw: only the tap (tx + 1, ty + 1) of the previous image is valid; fy about 1e-3, fx bisected across fx * fy > 1e-6f
    only = {k: v.copy() for k, v in planes(Z).items()}
    only["hist"][..., 3] = 0
    only["hist"][ty + 1, tx + 1, 3] = 4

    def frac(m):
        u, v = at(m, Z)
        return u - np.floor(u), v - np.floor(v), np.floor(u), np.floor(v)

    p13 = lambda m: frac(m)[3] == ty and frac(m)[1] >= F(1e-3)
    sgn = 1 if p13(moved(v13=F(base13 + 0.05))) else -1  # the direction in which v grows from ty
    _, v13 = _bisect(lambda t: moved(v13=t), p13, F(base13 - sgn * 0.0005), F(base13 + sgn * 0.05))
    sw = lambda m: frac(m)[2] == tx and frac(m)[0] * frac(m)[1] > F(1e-6)
    sgn = 1 if sw(moved(v12=F(base12 + 0.05), v13=v13)) else -1
    a, c = _bisect(lambda t: moved(v12=t, v13=v13), sw, F(base12 - sgn * 0.0005), F(base12 + sgn * 0.05))
    for t, holds in ((a, False), (c, True)):
        m = moved(v12=t, v13=v13)
        f = frac(m)
        if f[2] == tx and f[3] == ty:  # below the bound, but inside the same pixel: the bound itself decides
            out.append((f"sw {'above' if holds else 'below'} 1e-6 ({f[0] * f[1]:.9g})", inputs(Z), dict(only, meta=m), (tx, ty), holds,
                        at(m, Z)))
    return out


@pytest.mark.parametrize("size", [(16, 8), (37, 29)], ids=["16x8", "37x29"])
def test_reproject_synthetic_image_edges_and_weight_bound_bitexact(packed, ptopts, size):
    w, h = size
    p = packed["CornellBox"]
    cases = edge_cases(w, h)
    names = [c[0] for c in cases]
    print(w, h, [(c[0], float(c[5][0]), float(c[5][1])) for c in cases])
    assert any(n.startswith("sw above") for n in names) and any(n.startswith("sw below") for n in names)
    exact = {c[0]: (float(c[5][0]), float(c[5][1])) for c in cases}
    if (w, h) == (16, 8):  # u and v exactly on the bounds, where 1 / W and 1 / H are powers of two
        assert exact["u>-1 false"][0] == -1.0 and exact["u>=W true"][0] == float(w)
        assert exact["v<H false"][1] == float(h) and exact["v<=-1 true"][1] == -1.0
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for name, (acc, m2, geo, alb, meta), prev, (tx, ty), history, _ in cases:
            ref = tr.reproject(acc, m2, N, geo, alb, meta, prev=prev, **LOOSE)
            got = s.reproject(acc, m2, N, geo, alb, meta, prev=prev, params=LOOSE)
            check(got, ref, f"{w}x{h} {name}")
            # out of range, or the weight below the bound: no history.  (In range next to -1 the only taps inside the
            # image weigh about 1e-6 themselves, so the weight bound decides: the reference's bits are the check.)
            if history is not None:
                assert (ref["hist"][ty, tx, 3] > 1) == history, (name, ref["hist"][ty, tx, 3])
