"""Kernels against the oracle from cameras the scenes never use (tests/cam_cases.py): general
rotations, rolled and inside views, views from which every ray or almost every ray misses, extreme
height angles, and single meta fields no scene varies (focal, cam[3], the matrix's fourth row, aspect,
inv_w / inv_h, the roulette probability at its ends, NaN in the fields the kernels must not read).
tests/test_gpu_parity.py's bit-exact claims rest on one camera per scene, and the four Cornell
scenes' is the identity plus a translation.  Bar: bit-exact, counters equal, NaN equal to NaN, as
there.  tests/test_cam_cpu.py checks on the oracle alone that the images are worth comparing.

Per camera and kernel set: one frame (salt 3) and a 3-frame render, counted and uncounted.  All
cameras and kernel sets of one scene go through ONE Scene object (scene_for: none of these sets
changes an option that is read at scene creation), so the fused kernel's camera table (k_wf_camtab)
and the leaf pass's per-camera probe (pt_scene::pre_cam) are rebuilt between them;
test_one_scene_several_cameras does the same on a fresh Scene in a fixed order, and
test_two_cameras_back_to_back queues two renders without synchronising between them.
"""
import numpy as np
import pytest

import cam_cases as cc
import denoise_ref as dr
import oracle
import pt_amd
from test_gpu_parity import KERNELS, mismatch_report, same_bits
from test_gpu_shade import KSETS as SHADE_KSETS
from test_gpu_step_narrow import oracle_frame, oracle_render

pytestmark = pytest.mark.gpu

KSETS = dict(SHADE_KSETS)
for _k in ("wavefront_gen", "wavefront_nogen", "wavefront_region_perm", "wavefront_regen8_1block",
           "wavefront_bf_stack_replay", "wavefront_4parts"):
    KSETS[_k] = KERNELS[_k]
KSETS["wavefront_wide"] = {"PT_KERNEL": "wavefront", "PT_BF_NARROW": "0"}
BOAT_KSETS = {
    "auto": {},
    "leaf_pre0": {"PT_LEAF_PRE": "0"},
    "leaf_pre1": {"PT_LEAF_PRE": "1"},
    "wavefront_big8": KERNELS["wavefront_big8"],
    "mega": {"PT_KERNEL": "mega"},
}
PERT_KSETS = {k: KSETS[k] for k in ("auto", "literal", "mega", "wavefront_gen", "wavefront_nogen")}

CORNELL_CASES = [(s, c) for s, c in cc.CASES if s != "MedievalBoat"]
BOAT_CASES = [(s, c) for s, c in cc.CASES if s == "MedievalBoat"]


def ids(cases):
    return [cc.case_id(s, c) for s, c in cases]


def apply(ptopts, opts):
    for k, v in opts.items():
        ptopts.set(k, v)


@pytest.fixture(scope="module")
def scene_for(packed):
    """scene -> one pt_amd.Scene for the whole module, created under the default options (the options
    read at creation are mb_uid_order, leaf_bvh and leaf_skip; no kernel set here sets one), closed at
    the end."""
    pool = {}

    def get(scene):
        if scene not in pool:
            pt_amd.reset_options()
            pool[scene] = pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data)
        return pool[scene]
    yield get
    for s in pool.values():
        s.close()


def check_renders(s, p, key, meta):
    ref = oracle_frame(p, key, meta, cc.SALT, cc.DEPTH)
    racc, rc = oracle_render(p, key, meta, 3, cc.DEPTH)
    gpu = s.frame(meta, cc.SALT, cc.DEPTH)
    acc, gc = s.render(meta, 0, 3, 1, cc.DEPTH, pt_amd.MODE_AUTO, counters=True)
    plain = s.render(meta, 0, 3, 1, cc.DEPTH, pt_amd.MODE_AUTO)
    assert same_bits(gpu, ref), f"{key} frame: " + mismatch_report(gpu, ref)
    assert same_bits(acc, racc), f"{key} counted render: " + mismatch_report(acc, racc)
    assert same_bits(plain, racc), f"{key} render: " + mismatch_report(plain, racc)
    assert gc == rc, (gc, rc)


# ---------------------------------------------------------------------------------------------
# 1. named cameras
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kset", list(KSETS))
@pytest.mark.parametrize("scene,name", CORNELL_CASES, ids=ids(CORNELL_CASES))
def test_cameras_bitexact(packed, scene_for, ptopts, scene, name, kset):
    s = scene_for(scene)
    apply(ptopts, KSETS[kset])
    check_renders(s, packed[scene], "cam-" + cc.case_id(scene, name), cc.meta_of(scene, name))


@pytest.mark.parametrize("kset", list(BOAT_KSETS))
@pytest.mark.parametrize("scene,name", BOAT_CASES, ids=ids(BOAT_CASES))
def test_boat_cameras_bitexact(packed, scene_for, ptopts, scene, name, kset):
    s = scene_for(scene)
    apply(ptopts, BOAT_KSETS[kset])
    check_renders(s, packed[scene], "cam-" + cc.case_id(scene, name), cc.meta_of(scene, name))


# ---------------------------------------------------------------------------------------------
# 2. single meta fields
# ---------------------------------------------------------------------------------------------
FINITE_PERTS = [n for n in cc.PERTURBATIONS if n not in cc.NONFINITE]


@pytest.mark.parametrize("kset", list(PERT_KSETS))
@pytest.mark.parametrize("name", FINITE_PERTS)
def test_meta_fields_bitexact(packed, scene_for, ptopts, name, kset):
    s = scene_for(cc.PERT_SCENE)
    apply(ptopts, PERT_KSETS[kset])
    check_renders(s, packed[cc.PERT_SCENE], "cam-pert-" + name, cc.perturbed(name))


@pytest.mark.parametrize("kset", list(PERT_KSETS))
@pytest.mark.parametrize("name", cc.NONFINITE)
def test_nonfinite_cameras_give_no_hit(packed, ptopts, name, kset):
    """Every camera ray's direction is NaN (M all NaN; cam[0] = inf: inf - inf): no hit on any path,
    the frame is all-miss and the loops end (DESIGN.md §4 says why for each of these kernel sets)."""
    apply(ptopts, PERT_KSETS[kset])
    p = packed[cc.PERT_SCENE]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        check_renders(s, p, "cam-pert-" + name, cc.perturbed(name))


# ---------------------------------------------------------------------------------------------
# 3. one scene object, several cameras
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kset", ["auto", "wavefront_gen", "wavefront_nogen", "mega"])
def test_one_scene_several_cameras(packed, ptopts, kset):
    """XML, oblique, away, oblique, XML on a fresh Scene, each against its own reference: a camera
    table or probe kept from the render before would show in the second and in the last two."""
    apply(ptopts, KSETS[kset])
    scene = "CornellBox"
    p = packed[scene]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for name in ("xml", "oblique", "away", "oblique", "xml"):
            check_renders(s, p, "cam-" + cc.case_id(scene, name), cc.meta_of(scene, name))


def test_one_boat_several_cameras(packed, ptopts):
    """AUTO on the boat: the leaf-pass choice is probed per camera (pt_scene::pre_cam)."""
    scene = "MedievalBoat"
    p = packed[scene]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for name in ("xml", "rigging", "away", "rigging", "xml"):
            check_renders(s, p, "cam-" + cc.case_id(scene, name), cc.meta_of(scene, name))


@pytest.mark.parametrize("dual", [None, "1"], ids=["default", "dual"])
@pytest.mark.parametrize("scene,a,b", [("CornellBox", "oblique", "xml"), ("CornellBox", "away", "rolled"),
                                       ("MedievalBoat", "rigging", "xml")])
def test_two_cameras_back_to_back(packed, ptopts, scene, a, b, dual):
    """Two render_async calls with different cameras queued on one stream into two accumulators,
    nothing between them: the second call's camera table must not reach the first call's launches."""
    torch = pytest.importorskip("torch")
    if dual:
        ptopts.set("PT_DUAL", dual)
    p = packed[scene]
    W, H = cc.size_of(scene)
    acc = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for buf, name in zip(acc, (a, b)):
            s.render_async(cc.meta_of(scene, name), 0, 3, 1, cc.DEPTH, pt_amd.MODE_AUTO, buf.data_ptr(), st.cuda_stream)
        st.synchronize()
        s.check()
    for buf, name in zip(acc, (a, b)):
        key = "cam-" + cc.case_id(scene, name)
        ref, _ = oracle_render(p, key, cc.meta_of(scene, name), 3, cc.DEPTH)
        got = buf.cpu().numpy()
        assert same_bits(got, ref), f"{key}: " + mismatch_report(got, ref)


# ---------------------------------------------------------------------------------------------
# 4. several batches, a ragged last one
# ---------------------------------------------------------------------------------------------
BIG = (128, 96)
BANDS = [(0, 8), (44, 52), (88, 96)]


@pytest.mark.parametrize("parts", ["1", "2"])
@pytest.mark.parametrize("name", ["oblique", "wide170"])
def test_cameras_several_batches(packed, ptopts, name, parts):
    """128 x 96, 5 frames, wf_paths = 2 frames' paths: batches of 2 + 2 + 1 frames on 1 and 2 parts;
    three 8-row bands (top, middle, bottom) against the oracle's rows."""
    scene = "CornellBox"
    p = packed[scene]
    W, H = BIG
    meta = cc.meta_of(scene, name, BIG)
    ptopts.set("PT_KERNEL", "wavefront")
    ptopts.set("PT_WF_PATHS", str(2 * W * H))
    ptopts.set("PT_PARTS", parts)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        got = s.render(meta, 0, 5, 1, cc.DEPTH, pt_amd.MODE_AUTO)
    light = 0.0
    for y0, y1 in BANDS:
        ref, _ = oracle.render(p.triangle_data, p.bvh_data, meta, 0, 5, 1, cc.DEPTH, y0=y0, y1=y1)
        light += float(ref.sum())
        assert same_bits(got[y0:y1], ref), f"rows {y0}..{y1}: " + mismatch_report(got[y0:y1], ref)
    assert light > 0


# ---------------------------------------------------------------------------------------------
# 5. the camera's other consumers
# ---------------------------------------------------------------------------------------------
CONSUMERS = [("CornellBox", "oblique"), ("CornellBox", "wide170")]
FRAME = 5


@pytest.mark.parametrize("scene,name", CONSUMERS, ids=ids(CONSUMERS))
def test_camera_rays_ray_by_ray(scene_for, ptopts, scene, name):
    W, H = cc.size_of(scene)
    meta = cc.meta_of(scene, name)
    got = scene_for(scene).camera_rays(meta, FRAME)
    want = np.zeros((H, W, 8), np.float32)
    for y in range(H):
        for x in range(W):
            o, d = dr.camera_ray(meta, x, y, FRAME)
            want[y, x, 0:3], want[y, x, 3], want[y, x, 4:7] = o[:3], np.inf, d[:3]
    assert same_bits(got, want), mismatch_report(got, want)


@pytest.mark.parametrize("scene,name", CONSUMERS, ids=ids(CONSUMERS))
def test_features_from_other_cameras(packed, scene_for, ptopts, scene, name):
    p = packed[scene]
    W, H = cc.size_of(scene)
    meta = cc.meta_of(scene, name)
    rg, ra, rc = dr.FirstHits(p.triangle_data, p.bvh_data, meta).features((0, 0, W, H), 3, 2, 4)
    hits = int(ra[..., 3].sum())
    assert 0 < hits < rc["samples"]  # both hits and misses
    s = scene_for(scene)
    g, a, c = s.render_features(meta, 3, 2, 4, counters=True)
    g2, a2 = s.render_features(meta, 3, 2, 4)
    for got, ref in ((g, rg), (g2, rg), (a, ra), (a2, ra)):
        assert same_bits(got, ref), mismatch_report(got, ref)
    assert c == rc, (c, rc)


WIN = (5, 3, 19, 7)
RECTS = ((39, 31, 1, 1), (13, 12, 17, 10))


@pytest.mark.parametrize("kset", ["auto", "mega"])
def test_window_and_rects_keep_the_bits(packed, ptopts, kset):
    """A window and a two-rectangle list of the oblique render carry the full render's bits."""
    apply(ptopts, KSETS[kset])
    scene = "CornellBox"
    p = packed[scene]
    meta = cc.meta_of(scene, "oblique")
    full, _ = oracle_render(p, "cam-" + cc.case_id(scene, "oblique"), meta, 3, cc.DEPTH)

    def cut(img, r):
        return np.ascontiguousarray(img[r[1]:r[1] + r[3], r[0]:r[0] + r[2]])
    want = np.zeros_like(full)
    for r in RECTS:
        want[r[1]:r[1] + r[3], r[0]:r[0] + r[2]] = cut(full, r)
    assert cut(full, WIN).any() and cut(full, RECTS[1]).any()
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        win = s.render(meta, 0, 3, 1, cc.DEPTH, pt_amd.MODE_AUTO, window=WIN)
        lst = s.render_rects(meta, RECTS, 0, 3, 1, cc.DEPTH, pt_amd.MODE_AUTO)
    assert same_bits(win, cut(full, WIN)), mismatch_report(win, cut(full, WIN))
    assert same_bits(lst, want), mismatch_report(lst, want)
