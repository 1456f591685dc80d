"""GPU: the lens cameras (pt_scene_set_camera: thin lens, orthographic, equirectangular) against
lens_ref.py — the models restated in numpy, the oracle's radiance() on their rays — bit for bit with NaN
equal to NaN: pt_camera_rays, pt_frame and pt_render through every kernel set, batching, every slot map
(window, rectangle list, moments, adaptive, guide buffers, denoised image), the composition law with
pt_query_radiance, samples that are not admitted, and the setting's state."""

import numpy as np
import pytest

import adaptive_ref as ar
import cam_cases as cc
import denoise_ref as dr
import lens_ref as lr
import oracle
import pt_amd
import radiance_ref as rr
from test_gpu_adaptive import FLOOR, FRACTION, TOL
from test_gpu_parity import mismatch_report, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 40, 32
SETS = {"default": {}, "trace_shade": {"kernel": "wavefront", "fuse": 0}, "no_lds": {"lds": 0}, "bf_wide": {"bf_narrow": 0},
        "bf_stack": {"bf_stackless": 0}, "no_region_perm": {"region_perm": 0}, "parts4": {"parts": 4},
        "addr64": {"step_addr64": 1}}
BOAT_SETS = {"leaf_pre0": {"leaf_pre": 0}, "leaf_pre1": {"leaf_pre": 1}, "no_chunk_walks": {"leaf_walk": 0}}
IGNORED = {"mega": {"kernel": "mega"}, "literal": {"kernel": "literal"}, "fuse_gen1": {"fuse_gen": 1}, "regen2": {"regen": 2}}
MATRIX = [(c, k) for c in lr.CASES for k in list(SETS) + (list(BOAT_SETS) if c[0] == "MedievalBoat" else [])]
QUERY_COUNTS = ("samples", "ext_queries", "shadow_queries")
MODELS = {"thin_lens": ("thin_lens", 0.3, 3.6), "ortho": ("ortho", 0.0, 3.6), "equirect": ("equirect", 0.0, 1.0)}
THIN = ("CornellBox", "xml", ("thin_lens", 0.3, 3.6))  # the case the slot maps and the state tests share (lr.CASES[1])
WINDOW = (7, 5, 21, 13)  # not at the origin, odd sizes
RECTS = [(1, 2, 9, 5), (20, 0, 17, 11), (12, 19, 23, 13)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("radiance_ref"))


def open_scene(packed, scene, cam=None):
    s = pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data)
    if cam is not None:
        s.set_camera(*cam)
    return s


def check_counters(scene, got, want):
    """The oracle's sums; the boat: the query counts only (a cooperative big-leaf turn counts by wave)."""
    if scene == "MedievalBoat":
        assert {k: got[k] for k in QUERY_COUNTS} == {k: want[k] for k in QUERY_COUNTS}, (got, want)
    else:
        assert got == want, (got, want)


def clamped(frame):
    """0 + clamp(L): what the reference's accumulator holds after one frame from zeros."""
    return np.zeros_like(frame) + np.where(frame >= 0, frame, 0).astype(F)


def crop(a, win):
    x0, y0, w, h = win
    return a[y0:y0 + h, x0:x0 + w]


def test_setter_validation_and_state(packed):
    L = pt_amd.load_library()
    with open_scene(packed, "CornellBox") as s:
        assert s.camera == {"model": "pinhole", "lens_radius": 0.0, "focus_distance": 0.0}
        s.set_camera("thin_lens", 0.25, 3.5)
        assert s.camera == {"model": "thin_lens", "lens_radius": 0.25, "focus_distance": 3.5}
        bad = [(4, 0.1, 1.0), (77, 0.1, 1.0),
               ("thin_lens", -0.1, 1.0), ("thin_lens", np.nan, 1.0), ("thin_lens", np.inf, 1.0),
               ("thin_lens", 0.1, 0.0), ("thin_lens", 0.1, -1.0), ("thin_lens", 0.1, np.nan), ("thin_lens", 0.1, np.inf),
               ("ortho", 0.0, 0.0), ("ortho", 0.0, -2.0), ("ortho", 0.0, np.nan), ("ortho", 0.0, np.inf)]
        for cam in bad:
            with pytest.raises(pt_amd.PtError) as e:
                s.set_camera(*cam)
            assert e.value.code == -1 and "camera" in str(e.value), cam
            assert s.camera["model"] == "thin_lens" and s.camera["lens_radius"] == 0.25  # a refused call changes nothing
        # the fields a model does not use are ignored
        s.set_camera("ortho", np.nan, 2.0)
        s.set_camera("ortho", -1.0, 2.0)
        s.set_camera("equirect", np.nan, np.nan)
        s.set_camera("equirect", -1.0, -1.0)
        s.set_camera("thin_lens", 0.0, 1.0)  # a radius of zero is a lens
        s.set_camera("pinhole", np.nan, np.nan)
        assert s.camera["model"] == "pinhole"
        s.set_camera("ortho", 0.0, 2.0)
        assert L.pt_scene_set_camera(s._h, None) == 0 and s.camera["model"] == "pinhole"  # NULL: the pinhole
        assert L.pt_scene_set_camera(None, None) == -1 and L.pt_scene_get_camera(s._h, None) == -1
        with pytest.raises(ValueError):
            s.set_camera("fisheye")


@pytest.mark.parametrize("model", list(MODELS))
def test_camera_rays(packed, model):
    """The full image and a window not at the origin, frames 0 and 5: all eight words of every ray."""
    meta = cc.meta_of("CornellBox", "oblique", (W, H))
    with open_scene(packed, "CornellBox", MODELS[model]) as s:
        for frame in (0, 5):
            for win in (None, WINDOW):
                want, seeds, adm = lr.rays_seeds(meta, MODELS[model], frame, win)
                got = s.camera_rays(meta, frame, window=win)
                assert got.shape == want.shape and adm.all()
                assert same_bits(got, want), (frame, win, mismatch_report(got, want))
                assert np.array_equal(got[..., 7].view(np.uint32), want[..., 7].view(np.uint32))
                assert np.array_equal(s.camera_seeds(meta, win, frame), seeds)  # the seeds are the pinhole's
        pin = rr.camera_rays_seeds(meta, 0)[0]
        assert not same_bits(s.camera_rays(meta, 0), pin)
        s.set_camera("pinhole")
        assert same_bits(s.camera_rays(meta, 0), pin)


@pytest.mark.parametrize("case,kset", MATRIX, ids=[f"{lr.case_id(c)}-{k}" for c, k in MATRIX])
def test_parity(packed, ptopts, ref, case, kset):
    """pt_frame, and a 3-frame pt_render onto a non-zero accumulator, the counting and the plain build."""
    for k, v in {**SETS, **BOAT_SETS}[kset].items():
        ptopts.set(k, v)
    scene, _, cam = case
    meta, zero, wcnt, frames = lr.reference(ref, packed, case)
    onto, first = lr.reference_onto(ref, packed, case)
    h, w = zero.shape[:2]
    init = lr.initial_accum(h, w)
    assert (zero.sum(axis=2) > 0).mean() >= 0.25
    with open_scene(packed, scene, cam) as s:
        frame = s.frame(meta, lr.FRAME0, lr.DEPTH)
        counted, cnt = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH, accum=init.copy(), counters=True)
        plain = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH, accum=init.copy())
        s.check()
    assert same_bits(clamped(frame), first), mismatch_report(clamped(frame), first)
    for got in (counted, plain):
        assert same_bits(got, onto), mismatch_report(got, onto)
    check_counters(scene, cnt, wcnt)
    assert cnt["samples"] == lr.NFRAMES * w * h


@pytest.mark.parametrize("kset", list(IGNORED))
def test_options_that_do_not_apply(packed, ptopts, ref, kset):
    """kernel=mega|literal, fuse_gen and regen are ignored under a lens camera: the same bits."""
    for k, v in IGNORED[kset].items():
        ptopts.set(k, v)
    for case in (lr.CASES[1], lr.CASES[5], lr.CASES[6]):
        meta, zero, wcnt, _ = lr.reference(ref, packed, case)
        with open_scene(packed, case[0], case[2]) as s:
            for mode in (pt_amd.MODE_AUTO, pt_amd.MODE_MEGAKERNEL):
                got, cnt = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH, mode=mode, counters=True)
                assert same_bits(got, zero), (case, mode, mismatch_report(got, zero))
                assert cnt == wcnt


_BANDS = {}


@pytest.mark.parametrize("parts", (1, 2))
def test_batching(packed, ptopts, ref, parts):
    """128 x 96, 5 frames in batches of 2 + 2 + 1 (wf_paths = 2 frames' paths), on 1 and 2 parts: three
    8-row bands against the reference, each seeing light."""
    w, h, nframes = 128, 96, 5
    scene, camera, cam = "CornellBox", "oblique", ("thin_lens", 0.3, 3.6)
    meta = cc.meta_of(scene, camera, (w, h))
    ptopts.set("wf_paths", 2 * w * h)
    ptopts.set("parts", parts)
    with open_scene(packed, scene, cam) as s:
        got, cnt = s.render(meta, 1, nframes, 1, lr.DEPTH, counters=True)
        s.check()
    assert cnt["samples"] == w * h * nframes
    for y0 in (0, 44, 88):
        if y0 not in _BANDS:
            _BANDS[y0] = lr.render(ref, packed[scene], meta, cam, 1, nframes, lr.DEPTH, window=(0, y0, w, 8))[0]
        want = _BANDS[y0]
        assert want.sum() > 0
        assert same_bits(got[y0:y0 + 8], want), (y0, mismatch_report(got[y0:y0 + 8], want))


@pytest.mark.parametrize("case", (lr.CASES[1], lr.CASES[5], lr.CASES[6]), ids=lr.case_id)
def test_window_and_rects_equal_the_full_render(packed, ptopts, ref, case):
    meta, zero, _, _ = lr.reference(ref, packed, case)
    with open_scene(packed, case[0], case[2]) as s:
        win = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH, window=WINDOW)
        fw = s.frame(meta, lr.FRAME0, lr.DEPTH, window=WINDOW)
        ff = s.frame(meta, lr.FRAME0, lr.DEPTH)
        sentinel = np.full((H, W, 3), -7.5, F)
        rects, cnt = s.render_rects(meta, RECTS, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH, accum=sentinel.copy(), counters=True)
        s.check()
    assert same_bits(win, crop(zero, WINDOW)), mismatch_report(win, crop(zero, WINDOW))
    assert same_bits(fw, crop(ff, WINDOW))
    inside = np.zeros((H, W), bool)
    for r in RECTS:
        crop(inside, r)[...] = True
    onto = lr.accumulate(ref, packed[case[0]], meta, lr.reference(ref, packed, case)[3], lr.DEPTH, sentinel)[0]
    assert same_bits(rects[inside], onto[inside]), mismatch_report(rects[inside], onto[inside])
    assert np.all(rects[~inside] == F(-7.5))
    assert cnt["samples"] == lr.NFRAMES * int(inside.sum())


def test_moments(packed, ptopts, ref):
    """pt_render_moments: the accumulator bits of the plain call, m2 = sum of clamp(L)^2 in frame order."""
    meta, zero, wcnt, frames = lr.reference(ref, packed, THIN)
    per = [lr.accumulate(ref, packed[THIN[0]], meta, [f], lr.DEPTH, np.zeros_like(zero))[0] for f in frames]
    acc, m2 = ar.moments(per)
    assert same_bits(acc, zero)
    with open_scene(packed, *THIN[::2]) as s:
        gacc, gm2, cnt = s.render_moments(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH, counters=True)
        wacc, wm2 = s.render_moments(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH, window=WINDOW)
    assert same_bits(gacc, zero), mismatch_report(gacc, zero)
    assert same_bits(gm2, m2), mismatch_report(gm2, m2)
    assert same_bits(wacc, crop(zero, WINDOW)) and same_bits(wm2, crop(m2, WINDOW))
    assert cnt == wcnt


def test_adaptive_tiles_hold_plain_renders(packed, ptopts, ref):
    """pt_render_adaptive under the lens: every tile holds the bits of a plain render of its frame count."""
    meta, zero, _, _ = lr.reference(ref, packed, THIN)
    tile, (lo, step, hi) = (8, 8), (4, 4, 16)
    with open_scene(packed, *THIN[::2]) as s:
        r = s.render_adaptive(meta, lr.FRAME0, lr.DEPTH, pt_amd.MODE_AUTO, tile=tile, min_frames=lo, step_frames=step,
                              max_frames=hi, tol=TOL, floor=FLOOR, noisy_fraction=FRACTION)
        counts = sorted(set(r["tile_frames"].ravel().tolist()))
        plain = {n: s.render_moments(meta, lr.FRAME0, n, 1, lr.DEPTH) for n in counts}
        three = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH)
    assert same_bits(three, zero)  # the plain renders are the reference's
    assert len(counts) >= 2, counts
    for ty in range(r["tile_frames"].shape[0]):
        for tx in range(r["tile_frames"].shape[1]):
            win = (tx * 8, ty * 8, 8, 8)
            acc, m2 = plain[int(r["tile_frames"][ty, tx])]
            assert same_bits(crop(r["accum"], win), crop(acc, win)), (tx, ty)
            assert same_bits(crop(r["m2"], win), crop(m2, win)), (tx, ty)


@pytest.mark.parametrize("case", (lr.CASES[1], lr.CASES[5], lr.CASES[6], lr.CASES[11]), ids=lr.case_id)
def test_features_follow_the_models_rays(packed, ptopts, case):
    """pt_render_features: first hits of the model's rays (the oracle's intersect), whole image and window."""
    scene, camera, cam = case
    meta = cc.meta_of(scene, camera)
    w, h = cc.size_of(scene)
    fh = lr.FirstHits(packed[scene].triangle_data, packed[scene].bvh_data, meta, cam)
    pin = dr.FirstHits(packed[scene].triangle_data, packed[scene].bvh_data, meta)
    win = (3, 2, 15, 9)
    rg, ra, rc = fh.features((0, 0, w, h), lr.FRAME0, 2, 3)
    wg, wa, _ = fh.features(win, lr.FRAME0, 2, 3)
    pg, _, _ = pin.features(win, lr.FRAME0, 2, 3)
    assert ra[..., 3].sum() > 0 and not same_bits(wg, pg)
    with open_scene(packed, scene, cam) as s:
        g, a, c = s.render_features(meta, lr.FRAME0, 2, 3, counters=True)
        g2, a2 = s.render_features(meta, lr.FRAME0, 2, 3, window=win)
    assert same_bits(g, rg), mismatch_report(g, rg)
    assert same_bits(a, ra), mismatch_report(a, ra)
    assert same_bits(g2, wg) and same_bits(a2, wa)
    check_counters(scene, c, rc)


def test_denoised_image_is_the_reference_pipeline(packed, ptopts, ref):
    """pt_render_denoised_image under the thin lens: 8 frames, 4 feature frames, the defaults — the tone map
    of denoise_ref's composition over the lens's moments and guides, byte for byte."""
    scene, camera, cam = THIN
    meta = cc.meta_of(scene, camera)
    nframes, feature_frames = 8, 4
    zeros = np.zeros((H, W, 3), F)
    per = [lr.render(ref, packed[scene], meta, cam, k, 1, lr.DEPTH, acc=zeros)[0] for k in range(nframes)]
    acc, m2 = ar.moments(per)
    geo, alb, _ = lr.FirstHits(packed[scene].triangle_data, packed[scene].bvh_data, meta, cam).features((0, 0, W, H), 0, feature_frames, 1)
    sig = {k: v for k, v in dr.DEFAULTS.items() if k != "iters"}
    img = dr.denoise_passes(acc, m2, nframes, geo, alb, feature_frames, iters=5, **sig)[3][0]
    want = oracle.tonemap(img, 1).reshape(H, W, 4)
    with open_scene(packed, scene, cam) as s:
        rgba, cnt = s.render_denoised(meta, 0, nframes, 1, lr.DEPTH, feature_frames=feature_frames, counters=True)
        raw = s.render_image(meta, 0, nframes, 1, lr.DEPTH)
        s.set_camera("pinhole")
        pin = s.render_denoised(meta, 0, nframes, 1, lr.DEPTH, feature_frames=feature_frames)
    assert want[..., :3].max() > 0
    assert rgba.tobytes() == want.tobytes()
    assert raw.tobytes() == oracle.tonemap(acc, nframes).reshape(H, W, 4).tobytes()
    assert pin.tobytes() != want.tobytes()
    assert cnt["samples"] == W * H * (nframes + feature_frames)


@pytest.mark.parametrize("case", (lr.CASES[1], lr.CASES[5], lr.CASES[6]), ids=lr.case_id)
def test_composition_with_the_radiance_query(packed, ptopts, ref, case):
    """pt_camera_rays + pt_camera_seeds + pt_query_radiance(nsamples = 1) over three frames = the render."""
    scene, _, cam = case
    meta, zero, _, _ = lr.reference(ref, packed, case)
    h, w = zero.shape[:2]
    with open_scene(packed, scene, cam) as s:
        acc = np.zeros((h * w, 3), F)
        for k in range(lr.NFRAMES):
            rays, seeds = s.camera_rays(meta, lr.FRAME0 + k), s.camera_seeds(meta, None, lr.FRAME0 + k)
            acc = s.query_radiance(rays.reshape(-1, 8), seeds.reshape(-1), 1, lr.DEPTH, float(meta[45]), out=acc)
        got = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH)
    assert same_bits(acc.reshape(h, w, 3), got) and same_bits(got, zero)


def test_samples_that_are_not_admitted(packed, ptopts, ref):
    """A lens of radius 0 far from the origin with a plane of focus so near that, for part of the pixels,
    the target X(c) rounds to the lens point X(0) itself: 0 / 0, a NaN direction.  Those samples leave
    accumulator words of -0, NaN and inf as they are, and `samples` counts only the rest."""
    scene = "CornellBox"
    cam = ("thin_lens", 0.0, 4.5e-5)
    meta = cc.meta_from(cc.cam((1000, 1000, 1000), (0, 1, 0)), W, H)
    nframes = 3
    frames = [lr.rays_seeds(meta, cam, k) for k in range(nframes)]
    adm = np.stack([f[2] for f in frames])
    dead = ~adm.any(axis=0)  # pixels none of whose samples is admitted
    assert 0 < dead.sum() and 0 < adm.sum() < adm.size, (dead.sum(), adm.sum())
    for rays, _, a in frames:
        assert np.isnan(rays[~a][:, 4:7]).all()  # the lens point equals its target
    init = np.zeros((H, W, 3), F)
    init[..., 0], init[..., 1], init[..., 2] = -0.0, np.nan, np.inf
    want, wcnt = lr.accumulate(ref, packed[scene], meta, frames, lr.DEPTH, init)
    with open_scene(packed, scene, cam) as s:
        got, cnt = s.render(meta, 0, nframes, 1, lr.DEPTH, accum=init.copy(), counters=True)
        plain = s.render(meta, 0, nframes, 1, lr.DEPTH, accum=init.copy())
        rays = s.camera_rays(meta, 0)
        g, a, fc = s.render_features(meta, 0, nframes, counters=True)
        s.check()
    assert same_bits(rays, frames[0][0])  # reported as computed
    for out in (got, plain):
        assert np.array_equal(out.view(np.uint32)[dead], init.view(np.uint32)[dead])  # -0 stays -0
        assert same_bits(out, want), mismatch_report(out, want)
    assert cnt["samples"] == int(adm.sum()) == wcnt["samples"]
    assert cnt == wcnt
    assert fc["samples"] == fc["ext_queries"] == int(adm.sum())
    assert not a[dead].any() and not g[dead].any()


def test_pinhole_then_lens_then_pinhole(packed, ptopts, ref):
    scene, camera, cam = THIN
    meta, zero, _, _ = lr.reference(ref, packed, THIN)
    p = packed[scene]
    want, _ = oracle.render(p.triangle_data, p.bvh_data, meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH)
    with open_scene(packed, scene) as s:
        first = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH)
        s.set_camera(*cam)
        lens = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH)
        s.set_camera("pinhole")
        third = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH)
    assert first.tobytes() == third.tobytes() == want.tobytes()
    assert same_bits(lens, zero) and not same_bits(lens, first)


def test_async_renders_with_set_camera_between(packed, ptopts, ref):
    """Two render_async calls on one stream with set_camera between them: each takes the camera set when it
    was called."""
    torch = pytest.importorskip("torch")
    scene, camera, cam = THIN
    meta, zero, _, _ = lr.reference(ref, packed, THIN)
    ortho = lr.CASES[2]
    assert ortho[:2] == THIN[:2]
    ozero = lr.reference(ref, packed, ortho)[1]
    a = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    b = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with open_scene(packed, scene, cam) as s:
        s.render_async(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH, pt_amd.MODE_AUTO, a.data_ptr(), stream_ptr=st.cuda_stream)
        s.set_camera(*ortho[2])
        s.render_async(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH, pt_amd.MODE_AUTO, b.data_ptr(), stream_ptr=st.cuda_stream)
        st.synchronize()
        s.check()
    assert same_bits(a.cpu().numpy(), zero) and same_bits(b.cpu().numpy(), ozero)


def test_render_multi(packed, ptopts, ref):
    """Devices [0, 0] with the camera on both scenes: the shards' single renders (frames 0, 2 and frame 1 of
    the call) summed in device order, as for the pinhole; mismatched cameras are refused."""
    scene, camera, cam = THIN
    meta, zero, wcnt, frames = lr.reference(ref, packed, THIN)
    z = np.zeros_like(zero)
    want = lr.accumulate(ref, packed[scene], meta, frames[0::2], lr.DEPTH, z)[0] + \
        lr.accumulate(ref, packed[scene], meta, frames[1::2], lr.DEPTH, z)[0]
    ptopts.set("reduce", "ordered")
    with open_scene(packed, scene, cam) as s0, open_scene(packed, scene, cam) as s1:
        got, cnt = pt_amd.render_multi([s0, s1], meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH, counters=True)
        single = s0.render(meta, lr.FRAME0, 2, 2, lr.DEPTH) + s0.render(meta, lr.FRAME0 + 1, 1, 2, lr.DEPTH)
        assert same_bits(got, want), mismatch_report(got, want)
        assert same_bits(got, single) and cnt == wcnt
        assert np.allclose(got, zero, rtol=1e-5, atol=1e-6)
        for other in (("thin_lens", 0.25, 3.6), ("ortho", 0.3, 3.6), ("pinhole", 0.0, 1.0)):
            s1.set_camera(*other)
            with pytest.raises(pt_amd.PtError) as e:
                pt_amd.render_multi([s0, s1], meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH)
            assert e.value.code == -1 and "camera" in str(e.value)
