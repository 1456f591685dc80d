"""Scenes built on the device (pt_scene_create_mesh, csrc/pt_build.hip): the tree, its device records and
what every entry point makes of them.  Every comparison is bit for bit.

1. The device's tree (Scene.from_mesh(t).export_bvh()) equals the host builder's (bvh_build_lbvh(t), checked
   on the CPU by tests/test_lbvh_cpu.py) byte for byte: every input of the CPU list at max_leaf 1, 4, 8 with
   and without the emitter root, and a 100,000-triangle mesh (the sort's tiles and the level
   launches span many workgroups).
2. Renders on the mesh-built scene equal oracle.render on (triangle_data, exported tree), and the scene
   pt_amd.Scene(triangle_data, exported tree) makes under leaf_skip=0, counters included: frame and 3-frame
   render, depth 8, counted and uncounted, under AUTO, the literal kernel, the megakernel and the wavefront
   with the scene in global memory.
3. One band of a full-size render (synthetic 100,000, 1024^2, 4 frames) against the oracle; k_wf_trace runs.
4. pt_query_hits / pt_query_occluded against oracle.intersect on the exported tree.
5. render_window, render_features and a one-point gather equal the packed-route scene's.
6. Vertex normals on: a frame equals the oracle's with po_set_vertex_normals.
7. The 2^63 / 2^61 meshes of tests/cond_scenes.py (fast_rcp off / on) equal the oracle.
8. A bad index and a mesh without emitters are PT_ERR_INVALID with a message; export_bvh of a packed-route
   scene is refused.
"""
import types

import numpy as np
import pytest

import oracle
import pt_amd
import query_ref as qr
from lbvh_inputs import MAX_LEAVES, handmade, scene_inputs, synth_packed
from test_gpu_step_narrow import report, same_bits
from test_lbvh_cpu import HAND_NAMES, SCENE_NAMES

pytestmark = pytest.mark.gpu

PARAMS = [(m, iso) for m in MAX_LEAVES for iso in (True, False)]
WF = {"kernel": "wavefront"}
KSETS = {"auto": {}, "literal": {"kernel": "literal"}, "mega": {"kernel": "mega"}, "wf_global": {**WF, "lds": "0"}}
RENDERED = ["CornellBox-Glossy", "MedievalBoat", "synth1000", "emitters288"]
DEPTH, SALT = 8, 3


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, packed):
    base = tmp_path_factory.mktemp("lbvh_gpu")
    sc = scene_inputs(base, packed)
    out = {n: (p.triangle_data, p) for n, p in sc.items()}
    out.update({n: (t, None) for n, t in handmade().items()})
    out["synth100000"] = (lambda p: (p.triangle_data, p))(synth_packed(base, 100000))
    return out


def size_of(name):
    return (24, 16) if name == "MedievalBoat" else (40, 32)


@pytest.fixture(scope="module")
def built(inputs):
    """name -> (mesh-built scene, its exported tree, packed-route scene on that tree under leaf_skip=0, meta),
    at the default parameters; one of each per module."""
    pool = {}

    def get(name):
        if name not in pool:
            tri, p = inputs[name]
            pt_amd.reset_options()
            s = pt_amd.Scene.from_mesh(tri)
            bvh = s.export_bvh()
            with pt_amd.options(leaf_skip="0"):
                s2 = pt_amd.Scene(tri, bvh)
            pool[name] = (s, bvh, s2, p.meta_for(*size_of(name)))
        return pool[name]
    yield get
    for s, _, s2, _ in pool.values():
        s.close()
        s2.close()


# ---- 1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf,iso", PARAMS)
@pytest.mark.parametrize("name", SCENE_NAMES + HAND_NAMES)
def test_device_tree_equals_host_builder(inputs, name, max_leaf, iso):
    tri, _ = inputs[name]
    want = pt_amd.bvh_build_lbvh(tri, max_leaf=max_leaf, isolate_emitters=iso)
    with pt_amd.Scene.from_mesh(tri, max_leaf=max_leaf, isolate_emitters=iso) as s:
        got = s.export_bvh()
        info = s.info
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{bad.size} floats differ; first at {bad[:8].tolist()}"
    assert info["leaf_refs"] == int((tri[4] - tri[3]) / 4) and info["max_stack"] < 32


@pytest.mark.parametrize("max_leaf,iso", [(4, True), (8, False)])
def test_device_tree_equals_host_builder_100k(inputs, max_leaf, iso):
    tri, _ = inputs["synth100000"]
    want = pt_amd.bvh_build_lbvh(tri, max_leaf=max_leaf, isolate_emitters=iso)
    with pt_amd.Scene.from_mesh(tri, max_leaf=max_leaf, isolate_emitters=iso) as s:
        got = s.export_bvh()
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_build_profile_by_stage(inputs):
    """pt_build_params.profile: the build's launches are timed by stage, the tree is the same."""
    tri, _ = inputs["synth12500"]
    with pt_amd.Scene.from_mesh(tri, profile=True) as s, pt_amd.Scene.from_mesh(tri) as plain:
        prof = s.profile_read()
        assert np.array_equal(s.export_bvh().view(np.uint32), plain.export_bvh().view(np.uint32))
        assert plain.profile_read() == {}
    stages = ["k_build_bounds", "k_build_keys", "k_build_sort", "k_build_karras", "k_build_depth", "k_build_level",
              "k_build_offsets", "k_build_emit"]
    assert sorted(prof) == sorted(stages)
    assert (prof["k_build_sort"]["launches"], prof["k_build_level"]["launches"], prof["k_build_bounds"]["launches"]) == (12, 27, 2)
    assert all(prof[k]["total_ms"] > 0 for k in stages)


# ---- 2 -----------------------------------------------------------------------------------------
_ORACLE = {}


def reference(name, tri, bvh, meta):
    if name not in _ORACLE:
        _ORACLE[name] = (oracle.frame(tri, bvh, meta, SALT, DEPTH)[0], oracle.render(tri, bvh, meta, 0, 3, 1, DEPTH)[0])
    return _ORACLE[name]


@pytest.mark.parametrize("kset", list(KSETS))
@pytest.mark.parametrize("name", RENDERED)
def test_render_parity(inputs, built, ptopts, name, kset):
    tri, _ = inputs[name]
    s, bvh, s2, meta = built(name)
    ref_frame, ref_acc = reference(name, tri, bvh, meta)
    assert ref_acc.any()
    with pt_amd.options(KSETS[kset]):
        got = []
        for sc in (s, s2):
            frame = sc.frame(meta, SALT, DEPTH)
            plain = sc.render(meta, 0, 3, 1, DEPTH, pt_amd.MODE_AUTO)
            acc, cnt = sc.render(meta, 0, 3, 1, DEPTH, pt_amd.MODE_AUTO, counters=True)
            got.append((frame, plain, acc, cnt))
    (frame, plain, acc, cnt), (frame2, plain2, acc2, cnt2) = got
    assert same_bits(frame, ref_frame), f"{name} {kset} frame vs oracle: " + report(frame, ref_frame)
    assert same_bits(plain, ref_acc), f"{name} {kset} render vs oracle: " + report(plain, ref_acc)
    assert same_bits(acc, ref_acc), f"{name} {kset} counted render vs oracle: " + report(acc, ref_acc)
    assert same_bits(frame, frame2) and same_bits(plain, plain2) and same_bits(acc, acc2), f"{name} {kset} vs the packed route"
    assert cnt == cnt2, (cnt, cnt2)


# ---- 3 -----------------------------------------------------------------------------------------
def test_full_size_band_100k(inputs):
    tri, p = inputs["synth100000"]
    meta = p.meta_for(1024, 1024)
    with pt_amd.Scene.from_mesh(tri) as s:
        bvh = s.export_bvh()
        s.profile_enable(True)
        gpu = s.render(meta, 0, 4, 1, DEPTH, pt_amd.MODE_AUTO)
        prof = s.profile_read()
    assert "k_wf_trace" in prof, prof.keys()
    ref, _ = oracle.render(tri, bvh, meta, 0, 4, 1, DEPTH, y0=192, y1=208)
    assert ref.any()
    assert same_bits(gpu[192:208], ref), report(gpu[192:208], ref)


# ---- 4 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["CornellBox-Glossy", "synth1000"])
def test_queries(inputs, built, name):
    tri, p = inputs[name]
    s, bvh, _, _ = built(name)
    b = qr.Batch(name, types.SimpleNamespace(triangle_data=tri, bvh_data=bvh, meta_for=p.meta_for))
    assert b.hit.any() and not b.hit.all() and b.occ.any() and not b.occ.all()
    got = s.query_hits(b.rays)
    assert not qr.hits_mismatch(got, b), qr.hits_mismatch(got, b)
    assert np.array_equal(s.query_occluded(b.occ_rays), b.occ)


# ---- 5 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["CornellBox-Glossy", "emitters288"])
def test_other_entry_points(built, name):
    s, _, s2, meta = built(name)
    W, H = int(meta[0]), int(meta[1])
    win = (W - 17, H - 9, 16, 8)
    a, b = (sc.render(meta, 0, 3, 1, DEPTH, pt_amd.MODE_AUTO, window=win) for sc in (s, s2))
    assert a.any() and same_bits(a, b), report(a, b)
    (g, al), (g2, al2) = (sc.render_features(meta, SALT, 2, 1) for sc in (s, s2))
    assert al[..., 3].any() and same_bits(g, g2) and same_bits(al, al2)
    pt, nrm = [(0.0, 0.5, 0.0)], [(0.0, 1.0, 0.0)]
    ga, gb = (sc.gather(pt, nrm, [7], 16, max_depth=DEPTH, rr=float(meta[45])) for sc in (s, s2))
    assert ga.any() and same_bits(ga, gb), (ga, gb)


# ---- 6 -----------------------------------------------------------------------------------------
def test_vertex_normals(inputs):
    """CornellBox-Sphere carries vertex normals (triangle_data[6] > 0)."""
    tri, p = inputs["CornellBox-Sphere"]
    assert tri[6] > 0
    meta = p.meta_for(40, 32)
    with pt_amd.Scene.from_mesh(tri) as s:
        bvh = s.export_bvh()
        flat = s.frame(meta, SALT, DEPTH)
        s.set_vertex_normals(True)
        got = s.frame(meta, SALT, DEPTH)
    oracle.set_vertex_normals(True)
    try:
        ref, _ = oracle.frame(tri, bvh, meta, SALT, DEPTH)
    finally:
        oracle.set_vertex_normals(False)
    assert same_bits(got, ref), report(got, ref)
    assert not same_bits(got, flat), "vertex normals change this frame"


# ---- 7 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["giant", "nearly_giant"])
def test_conditioning(inputs, name):
    tri, p = inputs[name]
    meta = p.meta_for(40, 32)
    with pt_amd.Scene.from_mesh(tri) as s:
        bvh = s.export_bvh()
        got = s.render(meta, 0, 3, 1, DEPTH, pt_amd.MODE_AUTO)
    ref, _ = oracle.render(tri, bvh, meta, 0, 3, 1, DEPTH)
    assert ref.any() and same_bits(got, ref), report(got, ref)


# ---- 8 -----------------------------------------------------------------------------------------
def test_errors(inputs, packed):
    tri, _ = inputs["CornellBox"]
    bad = tri.copy()
    bad[int(tri[3]) + 1] = tri[0] + 1  # a vertex index past the last
    with pytest.raises(pt_amd.PtError) as e:
        pt_amd.Scene.from_mesh(bad)
    assert e.value.code == -1 and "vertex out of range" in str(e.value)
    dark = tri.copy()
    dark[8:16] = -1.0  # no emissive ranges
    with pytest.raises(pt_amd.PtError) as e:
        pt_amd.Scene.from_mesh(dark)
    assert e.value.code == -1 and "emissive" in str(e.value)
    nan = tri.copy()
    nan[16 + 3 * (int(tri[int(tri[3])]) - 1)] = np.nan
    with pytest.raises(pt_amd.PtError) as e:
        pt_amd.Scene.from_mesh(nan)
    assert e.value.code == -1 and "non-finite" in str(e.value)
    p = packed["CornellBox"]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        with pytest.raises(pt_amd.PtError) as e:
            s.export_bvh()
        assert e.value.code == -1
    # the library still builds after the refusals
    with pt_amd.Scene.from_mesh(tri) as s:
        assert s.info["leaf_refs"] == 36
