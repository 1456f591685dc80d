"""GPU: view-list renders (pt_render_views: many cameras in one call) against views_ref.py — every view its
own window render by the oracle's radiance(), placed into the atlas — bit for bit with NaN equal to NaN,
through every kernel set; and against the entry points that exist already (Scene.render with a window and
set_camera), byte for byte: the ignored options, batching, the list's order, two asynchronous calls on one
stream, a row pitch, samples that are not admitted, and every refusal with the accumulator untouched."""

import numpy as np
import pytest

import cam_cases as cc
import lens_ref as lr
import pt_amd
import radiance_ref as rr
import views_ref as vr
from test_gpu_parity import mismatch_report, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
SETS = {"default": {}, "trace_shade": {"kernel": "wavefront", "fuse": 0}, "no_lds": {"lds": 0}, "bf_wide": {"bf_narrow": 0},
        "bf_stack": {"bf_stackless": 0}, "no_region_perm": {"region_perm": 0}, "parts4": {"parts": 4},
        "addr64": {"step_addr64": 1}}
BOAT_SETS = {"leaf_pre0": {"leaf_pre": 0}, "leaf_pre1": {"leaf_pre": 1}, "no_chunk_walks": {"leaf_walk": 0}}
IGNORED = {"mega": {"kernel": "mega"}, "literal": {"kernel": "literal"}, "fuse_gen1": {"fuse_gen": 1}, "regen2": {"regen": 2}}
MATRIX = [(n, k) for n in vr.SETS for k in list(SETS) + (list(BOAT_SETS) if n == "boat3" else [])]
QUERY_COUNTS = ("samples", "ext_queries", "shadow_queries")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("radiance_ref"))


def open_scene(packed, scene):
    return pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data)


def check_counters(scene, got, want):
    """The oracle's sums; the boat: the query counts only (a cooperative big-leaf turn counts by wave)."""
    if scene == "MedievalBoat":
        assert {k: got[k] for k in QUERY_COUNTS} == {k: want[k] for k in QUERY_COUNTS}, (got, want)
    else:
        assert got == want, (got, want)


def raw(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def alone(s, v, nframes=vr.NFRAMES, stride=1, accum=None, mode=pt_amd.MODE_AUTO):
    """The view by the entry points that exist already: set_camera, then the window's render."""
    s.set_camera(*(v["camera"] or ("pinhole",)))
    out = s.render(v["meta"], v["frame0"], nframes, stride, vr.DEPTH, mode=mode, window=v["window"], accum=accum)
    s.set_camera("pinhole")
    return out


@pytest.mark.parametrize("name,kset", MATRIX, ids=[f"{n}-{k}" for n, k in MATRIX])
def test_parity(packed, ptopts, ref, name, kset):
    """3 frames at depth 8 onto a non-zero atlas, the counting and the plain build: every word of the atlas."""
    for k, v in {**SETS, **BOAT_SETS}[kset].items():
        ptopts.set(k, v)
    scene, views, atlas = vr.views_of(name)
    want, wcnt, _ = vr.reference(ref, packed, name)
    init = vr.initial_atlas(atlas)
    inside = vr.inside_mask(views, atlas)
    with open_scene(packed, scene) as s:
        counted, cnt = s.render_views(views, vr.NFRAMES, 1, vr.DEPTH, atlas=atlas, accum=init.copy(), counters=True)
        plain = s.render_views(views, vr.NFRAMES, 1, vr.DEPTH, atlas=atlas, accum=init.copy())
        s.check()
    for got in (counted, plain):
        assert same_bits(got, want), mismatch_report(got, want)
        assert np.array_equal(raw(got)[~inside], raw(init)[~inside])  # nothing outside the destinations changed
        assert not np.array_equal(raw(got)[inside], raw(init)[inside])
    check_counters(scene, cnt, wcnt)
    assert cnt["samples"] == vr.NFRAMES * int(inside.sum())


@pytest.mark.parametrize("kset", list(IGNORED))
def test_options_that_do_not_apply(packed, ptopts, ref, kset):
    """kernel=mega|literal, fuse_gen, regen and PT_MODE_MEGAKERNEL are ignored: the same bits."""
    for k, v in IGNORED[kset].items():
        ptopts.set(k, v)
    for name in ("mixed5", "models4"):
        scene, views, atlas = vr.views_of(name)
        want, wcnt, _ = vr.reference(ref, packed, name)
        with open_scene(packed, scene) as s:
            for mode in (pt_amd.MODE_AUTO, pt_amd.MODE_MEGAKERNEL):
                got, cnt = s.render_views(views, vr.NFRAMES, 1, vr.DEPTH, mode=mode, atlas=atlas,
                                          accum=vr.initial_atlas(atlas), counters=True)
                assert same_bits(got, want), (name, mode, mismatch_report(got, want))
                assert cnt == wcnt


def test_twins_are_the_plain_renders_frames(packed, ptopts):
    """The same meta twice with frame0 0 and 3: the plain render's frames 0..2 and 3..5, which differ."""
    scene, views, atlas = vr.views_of("twins")
    with open_scene(packed, scene) as s:
        got = s.render_views(views, 3, 1, vr.DEPTH, atlas=atlas)
        a = s.render(views[0]["meta"], 0, 3, 1, vr.DEPTH)
        b = s.render(views[0]["meta"], 3, 3, 1, vr.DEPTH)
    assert vr.place(got, views[0]).tobytes() == a.tobytes()
    assert vr.place(got, views[1]).tobytes() == b.tobytes()
    assert a.tobytes() != b.tobytes()


@pytest.mark.parametrize("name", ("mixed5", "models4"))
def test_tiles_are_the_existing_entry_points(packed, ptopts, name):
    """Without the oracle: each tile is byte-identical to Scene.render(window=...) of that view alone, under
    set_camera for the lens views; a one-view list is pt_render_window; the scene's own camera is not read."""
    scene, views, atlas = vr.views_of(name)
    init = vr.initial_atlas(atlas)
    with open_scene(packed, scene) as s:
        got = s.render_views(views, vr.NFRAMES, 1, vr.DEPTH, atlas=atlas, accum=init.copy())
        for k, v in enumerate(views):
            want = alone(s, v, accum=vr.place(init, v).copy())
            assert vr.place(got, v).tobytes() == want.tobytes(), (name, k)
            one = dict(v, dst=(0, 0))
            single = s.render_views([one], vr.NFRAMES, 1, vr.DEPTH, atlas=v["window"][2:],
                                    accum=vr.place(init, v).copy())
            assert single.tobytes() == want.tobytes(), (name, k)
        s.set_camera("thin_lens", 0.3, 3.6)  # the views carry their cameras: a pinhole view stays the pinhole's
        again = s.render_views(views, vr.NFRAMES, 1, vr.DEPTH, atlas=atlas, accum=init.copy())
        assert s.camera["model"] == "thin_lens"
        s.check()
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("parts", (1, 2))
def test_batching(packed, ptopts, ref, parts):
    """mixed5, 5 frames in batches of 2 + 2 + 1 (wf_paths = 2 frames' paths), on 1 and 2 parts."""
    nframes = 5
    scene, views, atlas = vr.views_of("mixed5")
    want, wcnt, _ = vr.reference(ref, packed, "mixed5", nframes=nframes)
    ptopts.set("wf_paths", 2 * vr.MIXED5_NPIX)
    ptopts.set("parts", parts)
    with open_scene(packed, scene) as s:
        got, cnt = s.render_views(views, nframes, 1, vr.DEPTH, atlas=atlas, accum=vr.initial_atlas(atlas), counters=True)
        s.check()
    assert same_bits(got, want), mismatch_report(got, want)
    assert cnt == wcnt and cnt["samples"] == nframes * vr.MIXED5_NPIX


def test_the_lists_order_changes_nothing(packed, ptopts):
    """Permuting the list, each view keeping its destination, leaves the atlas bytes as they were."""
    for name in ("mixed5", "models4"):
        scene, views, atlas = vr.views_of(name)
        init = vr.initial_atlas(atlas)
        with open_scene(packed, scene) as s:
            base = s.render_views(views, vr.NFRAMES, 1, vr.DEPTH, atlas=atlas, accum=init.copy())
            for perm in (views[::-1], views[2:] + views[:2]):
                got = s.render_views(perm, vr.NFRAMES, 1, vr.DEPTH, atlas=atlas, accum=init.copy())
                assert got.tobytes() == base.tobytes(), name


def test_two_async_calls_on_one_stream(packed, ptopts, ref):
    """Two render_views_async calls with different lists back to back on one stream into two atlases: each
    its own reference (the second call's table copy cannot overtake the first call's kernels)."""
    torch = pytest.importorskip("torch")
    (scene, va, aa), (scene_b, vb, ab) = vr.views_of("mixed5"), vr.views_of("models4")
    assert scene == scene_b
    wa, wb = vr.reference(ref, packed, "mixed5")[0], vr.reference(ref, packed, "models4")[0]
    a = torch.from_numpy(vr.initial_atlas(aa)).cuda()
    b = torch.from_numpy(vr.initial_atlas(ab)).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with open_scene(packed, scene) as s:
        assert s.render_views_async(va, vr.NFRAMES, 1, vr.DEPTH, pt_amd.MODE_AUTO, a.data_ptr(), atlas=aa,
                                    stream_ptr=st.cuda_stream) == aa
        s.render_views_async(vb, vr.NFRAMES, 1, vr.DEPTH, pt_amd.MODE_AUTO, b.data_ptr(), atlas=ab, stream_ptr=st.cuda_stream)
        st.synchronize()
        s.check()
    assert same_bits(a.cpu().numpy(), wa), mismatch_report(a.cpu().numpy(), wa)
    assert same_bits(b.cpu().numpy(), wb), mismatch_report(b.cpu().numpy(), wb)


def test_row_pitch_renders_in_place(packed, ptopts, ref):
    """row_pitch > atlas_w: the atlas inside a larger buffer whose other words keep their bits."""
    torch = pytest.importorskip("torch")
    scene, views, atlas = vr.views_of("mixed5")
    want = vr.reference(ref, packed, "mixed5")[0]
    aw, ah = atlas
    BW, BH, ox, oy = aw + 13, ah + 5, 7, 3
    host = np.full((BH, BW, 3), -7.5, F)
    host[oy:oy + ah, ox:ox + aw] = vr.initial_atlas(atlas)
    expect = host.copy()
    expect[oy:oy + ah, ox:ox + aw] = want
    buf = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    with open_scene(packed, scene) as s:
        s.render_views_async(views, vr.NFRAMES, 1, vr.DEPTH, pt_amd.MODE_AUTO, buf.data_ptr() + 12 * (oy * BW + ox),
                             atlas=atlas, row_pitch=BW)
        torch.cuda.synchronize()
        s.check()
    got = buf.cpu().numpy()
    assert same_bits(got, expect), mismatch_report(got, expect)
    outside = np.ones((BH, BW), bool)
    outside[oy:oy + ah, ox:ox + aw] = ~vr.inside_mask(views, atlas)
    assert np.array_equal(raw(got)[outside], raw(host)[outside])


def test_samples_that_are_not_admitted(packed, ptopts, ref):
    """test_gpu_lens.py's degenerate thin lens (part of its samples have a NaN direction) as one view of a
    list, beside a pinhole view, on accumulator words -0, NaN and inf: those samples leave the words as they
    are and count nothing."""
    scene, W, H, nframes = "CornellBox", 40, 32, 3
    cam = ("thin_lens", 0.0, 4.5e-5)
    views = [{"meta": cc.meta_of(scene, "xml"), "window": (5, 4, 9, 7), "camera": None, "frame0": 1, "dst": (41, 2)},
             {"meta": cc.meta_from(cc.cam((1000, 1000, 1000), (0, 1, 0)), W, H), "window": (0, 0, W, H), "camera": cam,
              "frame0": 0, "dst": (0, 0)}]
    atlas = (52, 32)
    init = np.zeros((atlas[1], atlas[0], 3), F)
    init[..., 0], init[..., 1], init[..., 2] = -0.0, np.nan, np.inf
    want, total, dead = init.copy(), {}, None
    for v in views:
        frames = vr.view_frames(v, nframes)
        if v["camera"]:
            adm = np.stack([f[2] for f in frames])
            dead = ~adm.any(axis=0)
            assert 0 < dead.sum() and 0 < adm.sum() < adm.size
        onto, cnt = lr.accumulate(ref, packed[scene], v["meta"], frames, vr.DEPTH, vr.place(want, v))
        vr.place(want, v)[...] = onto
        for k, c in cnt.items():
            total[k] = total.get(k, 0) + c
    with open_scene(packed, scene) as s:
        got, cnt = s.render_views(views, nframes, 1, vr.DEPTH, atlas=atlas, accum=init.copy(), counters=True)
        plain = s.render_views(views, nframes, 1, vr.DEPTH, atlas=atlas, accum=init.copy())
        s.check()
    for out in (got, plain):
        assert np.array_equal(raw(vr.place(out, views[1]))[dead], raw(vr.place(init, views[1]))[dead])  # -0 stays -0
        assert same_bits(out, want), mismatch_report(out, want)
    assert cnt == total and cnt["samples"] == 9 * 7 * nframes + int(adm.sum())


def _refusals():
    scene, views, atlas = vr.views_of("models4")
    v = lambda k, **kw: [dict(x, **(kw if i == k else {})) for i, x in enumerate(views)]  # noqa: E731
    meta = lambda **kw: _edit(views[1]["meta"], **kw)  # noqa: E731
    return atlas, views, [
        ("empty", [], atlas, {}, ["empty"]),
        ("no_area", v(1, window=(3, 3, 0, 2)), atlas, {}, ["views[1]", "at least 1"]),
        ("outside_image", v(2, window=(1, 1, 40, 32)), atlas, {}, ["views[2]", "within its image"]),
        ("outside_atlas", v(3, dst=(41, 32)), atlas, {}, ["views[3]", "outside the atlas"]),
        ("overlap", v(3, dst=(40, 31)), atlas, {}, ["views[1]", "views[3]", "overlap"]),  # one row of view 1
        ("frames", v(1, frame0=(1 << 24) - 2), atlas, {}, ["views[1]", "2^24"]),
        ("camera", v(2, camera=("ortho", 0.0, -1.0)), atlas, {}, ["views[2]", "camera"]),
        ("model", v(0, camera=(9, 0.0, 1.0)), atlas, {}, ["views[0]", "unknown model"]),
        ("rr", v(1, meta=meta(m45=0.5)), atlas, {}, ["views[1]", "meta[45]"]),
        ("direct", v(1, meta=meta(m46=1.0)), atlas, {}, ["views[1]", "meta[46]"]),
        ("image", v(1, meta=meta(m0=40.5)), atlas, {}, ["views[1]", "meta[0..1]"]),
        ("depth", views, atlas, {"max_depth": 4000}, ["max_depth"]),
        ("mode", views, atlas, {"mode": 7}, ["mode"]),
    ]


def _edit(m, **kw):
    m = np.array(m, F)
    for k, x in kw.items():
        m[int(k[1:])] = x
    return m


@pytest.mark.parametrize("case", [c[0] for c in _refusals()[2]])
def test_refusals_leave_the_accumulator_alone(packed, ptopts, case):
    """Every refusal through the real entry points: PT_ERR_INVALID, the view named, no word of the atlas touched."""
    torch = pytest.importorskip("torch")
    atlas, good, cases = _refusals()
    _, views, atl, kw, words = next(c for c in cases if c[0] == case)
    init = vr.initial_atlas(atlas)
    buf = torch.from_numpy(init).cuda()
    torch.cuda.synchronize()
    with open_scene(packed, "CornellBox") as s:
        host = init.copy()
        with pytest.raises(pt_amd.PtError) as e:
            s.render_views(views, vr.NFRAMES, 1, kw.get("max_depth", vr.DEPTH), mode=kw.get("mode", 0), atlas=atl, accum=host)
        assert e.value.code == -1
        for word in words:
            assert word in str(e.value), str(e.value)
        assert host.tobytes() == init.tobytes()
        with pytest.raises(pt_amd.PtError) as e:
            s.render_views_async(views, vr.NFRAMES, 1, kw.get("max_depth", vr.DEPTH), kw.get("mode", 0), buf.data_ptr(), atlas=atl)
        assert e.value.code == -1
        if case == "empty":  # ... and the reserved word, NULL and the pitch, which the binding itself never produces
            L = pt_amd.load_library()
            arr, n, _ = pt_amd._lib._views(good, atlas)
            arr[2].reserved = 5
            assert L.pt_render_views_async(s._h, arr, n, atlas[0], atlas[1], 3, 1, 8, 0, buf.data_ptr(), atlas[0], None, None) == -1
            assert b"views[2]" in L.pt_last_error() and b"reserved" in L.pt_last_error()
            arr[2].reserved = 0
            assert L.pt_render_views_async(s._h, arr, n, atlas[0], atlas[1], 3, 1, 8, 0, buf.data_ptr(), atlas[0] - 1, None, None) == -1
            assert b"row_pitch" in L.pt_last_error()
            assert L.pt_render_views_async(s._h, None, n, atlas[0], atlas[1], 3, 1, 8, 0, buf.data_ptr(), atlas[0], None, None) == -1
            assert b"NULL" in L.pt_last_error()
            assert L.pt_render_views_async(s._h, arr, n, atlas[0], atlas[1], 3, 1, 8, 0, None, atlas[0], None, None) == -1
            # a last frame index of 2^24 through the stride
            arr[0].frame0 = (1 << 24) - 3
            assert L.pt_render_views_async(s._h, arr, n, atlas[0], atlas[1], 3, 2, 8, 0, buf.data_ptr(), atlas[0], None, None) == -1
            assert b"views[0]" in L.pt_last_error() and b"2^24" in L.pt_last_error()
        s.check()
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == init.tobytes()
