"""Kernels against the oracle on trees no builder here produces (tests/tree_cases.py): traversal stacks
of 20 and 31 levels (thin stilts, fat stilts whose stack really fills, chains), node and entry counts
on both sides of every threshold of the brute-force kernels (narrow replay <= 32 / <= 32, replay tree
<= 63 / <= 64, mailbox <= 64), added leaves of 1 .. 129 entries around the lean flavours' turn widths
(with a repeated entry, and empty leaf pairs), and the same trees stored in other record orders.
tests/test_tree_cpu.py checks on the CPU that the cases are what they claim and worth comparing.

Bar: bit-exact, counters equal, NaN equal to NaN, as tests/test_gpu_parity.py.  Per case and kernel
set: one frame (salt 3) and a 3-frame render, counted and uncounted, against the oracle on the same
buffers.  Every case keeps ONE Scene for all its kernel sets (none sets an option read at creation).

Which instance ran is asserted from the layout rules (tree_cases.facts), not from the run: under the
wavefront sets a mailbox scene launches k_wf_step (flavour 4xx) and no k_wf_trace, any other scene the
reverse (the library's launch profile names the kernel families); pt_last_bf_width is 32 for the
narrow replay (scene in LDS, uncounted), 64 for the stackless replay tree, 0 for the stack walk; AUTO
takes the megakernel (k_regen) below 2^19 paths unless the scene is a mailbox scene or has a leaf of
at least 128 entries.
Whether a scene is staged in LDS is not observable through the C ABI: tests/test_tree_cpu.py asserts
scene_fits_lds' verdict per case from the harness's span (the synthetic 200-triangle scene crosses it
between max_stack 8 and 9), and the sets here run with option lds on and off.

Cases x kernel sets are thinned (FULL and sets_of below), the catalogue is not.
"""
import numpy as np
import pytest

import denoise_ref as dr
import oracle
import pt_amd
import query_ref as qr
import tree_cases as tc
from pt_amd import _lib
from test_gpu_step_narrow import report, same_bits

pytestmark = pytest.mark.gpu

WF = {"kernel": "wavefront"}
MB_KSETS = {
    "auto": {}, "literal": {"kernel": "literal"}, "mega": {"kernel": "mega"},
    "wf_lds": WF, "wf_global": {**WF, "lds": "0"}, "nofuse": {**WF, "fuse": "0"}, "nobf": {**WF, "bf": "0"},
    "nomailbox": {**WF, "mailbox": "0"}, "slots1": {**WF, "bf_slots": "1"}, "addr64": {**WF, "step_addr64": "1"},
}
TR_KSETS = {
    "auto": {}, "mega": {"kernel": "mega"},
    "lean": {**WF, "trav": "lean"}, "lean4": {**WF, "trav": "lean4"}, "lean16": {**WF, "trav": "lean16"},
    "lean32": {**WF, "trav": "lean32"}, "flat": {**WF, "trav": "flat1"},
    "leaf_pre1": {**WF, "leaf_pre": "1"}, "leaf_pre0": {**WF, "leaf_pre": "0"},
    "big16": {**WF, "big_leaf": "16"}, "wf_default": WF,
    "ring128": {**WF, "trace_ring": "128"}, "ring256": {**WF, "trace_ring": "256"},
    # each lane walks its own leaf pairs K entries a turn (lean_leaf_loop<K>): by default every leaf turn
    # of k_wf_trace is pooled over the wave (lean_leaf_pool, the same code for every K) and a leaf of
    # >= 128 entries goes to the cooperative turns or the leaf pass
    **{f"lean{k}_np": {**WF, "trav": f"lean{k}".rstrip("1"), "leaf_pool": "0", "big_leaf": "0"} for k in (1, 4, 16, 32)},
}
BIG_LEAF = 128  # pt_capi_render.hip kBigLeafDefault
UNPOOLED = ("lean4_np", "lean16_np", "lean32_np")
# Cases x kernel sets, thinned (the full product ran 992 tests in 27 s, tests/test_gpu_cam.py takes 8 s):
# FULL cases run every set of their kind; every other case runs AUTO and, in turn through the
# catalogue, two of the other sets (the boat trees, 0.3 s a render, one; the stride is odd, so a scene's
# cases meet every set in turn); every added leaf runs the unpooled lean4, lean16 and lean32 turns.
FULL = ("stilts-CornellBox-31Z", "fat-stilts-CornellBox-31L", "fat-stilts-CornellBox-Glossy-31L", "chain-CornellBox-Z",
        "bush-CornellBox-32", "bush-CornellBox-33", "bush-CornellBox-64", "bush-CornellBox-65", "trim-synth80-63",
        "trim-synth80-64", "trim-synth80-65", "stilts-synth200-9Z", "leaf-CornellBox-Sphere-129dup", "leaf-synth200-64",
        "stilts-MedievalBoat-31Z")


@pytest.fixture(scope="module")
def bases(packed, tmp_path_factory):
    return tc.bases(packed, tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def scene_of(bases):
    pool = {}

    def get(cid):
        if cid not in pool:
            pt_amd.reset_options()
            b = tc.built(bases, cid)
            pool[cid] = (pt_amd.Scene(b.triangle_data, b.bvh_data), b, tc.facts(b.bvh_data))
        return pool[cid]
    yield get
    for s, _, _ in pool.values():
        s.close()


_ORACLE = {}


def reference(b):
    if b.case.id not in _ORACLE:
        _ORACLE[b.case.id] = (oracle.frame(b.triangle_data, b.bvh_data, b.meta, tc.SALT, tc.DEPTH)[0],
                              oracle.render(b.triangle_data, b.bvh_data, b.meta, 0, 3, 1, tc.DEPTH))
    return _ORACLE[b.case.id]


def check_case(s, b, f, kset, opts):
    ref, (racc, rc) = reference(b)
    s.profile_enable(True)
    gpu = s.frame(b.meta, tc.SALT, tc.DEPTH)
    width = _lib.last_bf_width()
    plain = s.render(b.meta, 0, 3, 1, tc.DEPTH, pt_amd.MODE_AUTO)
    prof = s.profile_read()
    s.profile_enable(False)
    acc, gc = s.render(b.meta, 0, 3, 1, tc.DEPTH, pt_amd.MODE_AUTO, counters=True)
    assert same_bits(gpu, ref), f"{b.case.id} {kset} frame: " + report(gpu, ref)
    assert same_bits(plain, racc), f"{b.case.id} {kset} render: " + report(plain, racc)
    assert same_bits(acc, racc), f"{b.case.id} {kset} counted render: " + report(acc, racc)
    assert gc == rc, (gc, rc)
    # the instance, from the layout rules
    if not opts:  # AUTO (pt_capi_render.hip: the wavefront from one path on for mailbox scenes and big leaves)
        wave = f["mailbox"] or f["max_leaf"] >= BIG_LEAF
        assert ("k_regen" in prof) == (not wave) and ("k_wf_step" in prof) == f["mailbox"], (f, prof.keys())
        assert ("k_wf_trace" in prof) == (wave and not f["mailbox"]), (f, prof.keys())
        if not f["mailbox"]:
            return
    elif opts.get("kernel") != "wavefront":
        return
    brute = f["mailbox"] and "trav" not in opts and opts.get("mailbox") != "0" and opts.get("bf") != "0"
    fused = brute and opts.get("fuse") != "0"
    assert ("k_wf_step" in prof) == fused, (f, prof.keys())
    assert ("k_wf_trace" in prof) == (not fused), (f, prof.keys())
    if fused:
        lds = opts.get("lds") != "0"  # every mailbox case fits (tests/test_tree_cpu.py)
        assert width == (32 if f["narrow"] and lds else 64 if f["replay"] else 0), (width, f)


def sets_of(case, i):
    ks = list(MB_KSETS if tc_mailbox(case) else TR_KSETS)
    if case.id in FULL:
        return ks
    rest = ks[1:]
    boat = case.base == "MedievalBoat"  # its scenes cost 0.5 s each: one set beside AUTO
    out = ["auto"] + [rest[(3 * i + j) % len(rest)] for j in range(1 if boat else 2)]
    if case.probe == "added" and not tc_mailbox(case):
        out += UNPOOLED
    return list(dict.fromkeys(out))


def tc_mailbox(case):
    """The mailbox verdict the catalogue fixes for the case (U <= 64); test_tree_cpu.py holds it to the harness's."""
    if "mailbox" in case.expect:
        return case.expect["mailbox"]
    if "U" in case.expect:
        return case.expect["U"] <= tc.MAILBOX_U
    return case.base == "CornellBox"  # trees over CornellBox's 32 entries; every other base has more than 64


PARAMS = [(c.id, k) for i, c in enumerate(tc.CASES) for k in sets_of(c, i)]


@pytest.mark.parametrize("cid,kset", PARAMS, ids=[f"{c}-{k}" for c, k in PARAMS])
def test_trees_bitexact(scene_of, ptopts, cid, kset):
    s, b, f = scene_of(cid)
    assert f["mailbox"] == tc_mailbox(b.case)
    opts = (MB_KSETS if f["mailbox"] else TR_KSETS)[kset]
    for k, v in opts.items():
        ptopts.set(k, v)
    check_case(s, b, f, kset, opts)


# ---------------------------------------------------------------------------------------------
# the deepest trees through the other calls
# ---------------------------------------------------------------------------------------------
DEEP = ["stilts-CornellBox-31Z", "stilts-CornellBox-Glossy-31Z", "stilts-CornellBox-Sphere-31Z", "stilts-MedievalBoat-31Z",
        "fat-stilts-CornellBox-31L", "fat-stilts-CornellBox-Glossy-31L", "chain-CornellBox-Z"]
SIDES = {"stilts-CornellBox-31Z": ("stilts-CornellBox-31L", "stilts-CornellBox-31R"),
         "stilts-CornellBox-Glossy-31Z": ("stilts-CornellBox-Glossy-31L", "stilts-CornellBox-Glossy-31R"),
         "stilts-CornellBox-Sphere-31Z": ("stilts-CornellBox-Sphere-31L", "stilts-CornellBox-Sphere-31R"),
         "stilts-MedievalBoat-31Z": ("stilts-MedievalBoat-31L", "stilts-MedievalBoat-31R")}
N_RAYS = 4096
_BATCH = {}


def batch_of(b):
    if b.case.id not in _BATCH:
        _BATCH[b.case.id] = qr.Batch(b.case.base, b)
    return _BATCH[b.case.id]


@pytest.mark.parametrize("cid", DEEP)
def test_deep_queries(scene_of, ptopts, cid):
    """query_ref's families on the case's own buffers: every hit record and the counters of the hits
    batch, the first 4,096 occlusion rays byte for byte; the stilts' other two sides answer the same
    rays with the same records (their trees differ only in the side of the empty leaves)."""
    s, b, f = scene_of(cid)
    q = batch_of(b)
    assert q.hit.any() and not q.hit.all()
    counted, cnt = s.query_hits(q.rays, counters=True)
    plain = s.query_hits(q.rays)
    for got in (counted, plain):
        assert not qr.hits_mismatch(got, q), qr.hits_mismatch(got, q)
    if b.case.base == "MedievalBoat":  # a cooperative turn counts by wave (tests/test_gpu_query.py)
        assert (cnt["samples"], cnt["ext_queries"], cnt["shadow_queries"]) == (0, len(q.rays), 0), cnt
    else:
        assert cnt == q.counters, (cnt, q.counters)
    rays, occ = q.occ_rays[:N_RAYS], q.occ[:N_RAYS]
    assert occ.any() and not occ.all()
    assert np.array_equal(s.query_occluded(rays), occ)
    for other in SIDES.get(cid, ()):
        s2, _, _ = scene_of(other)
        got = s2.query_hits(q.rays)
        assert not qr.hits_mismatch(got, q), (other, qr.hits_mismatch(got, q))
        assert np.array_equal(s2.query_occluded(rays), occ), other


@pytest.mark.parametrize("cid", DEEP)
def test_deep_camera_rays_features_window(scene_of, ptopts, cid):
    """pt_camera_rays then pt_query_hits gives the first hits pt_render_features sums (the oracle's, ray
    by ray), and a 16 x 8 window of the render carries the full render's bits."""
    s, b, f = scene_of(cid)
    W, H = b.size
    rays = s.camera_rays(b.meta, tc.SALT)
    hits = s.query_hits(rays.reshape(-1, 8)).reshape(H, W, 8)
    fh = dr.FirstHits(b.triangle_data, b.bvh_data, b.meta)
    rg, ra, rcnt = fh.features((0, 0, W, H), tc.SALT, 1, 1)
    g, a, c = s.render_features(b.meta, tc.SALT, 1, 1, counters=True)
    assert same_bits(g, rg), report(g, rg)
    assert same_bits(a, ra), report(a, ra)
    if b.case.base != "MedievalBoat":
        assert c == rcnt, (c, rcnt)
    hit = ra[..., 3] > 0
    assert hit.any()
    assert np.array_equal(hits[..., 3] > 0, hit)
    assert same_bits(hits[..., 3][hit], rg[..., 3][hit]) and same_bits(hits[..., 4:7][hit] + np.float32(0), rg[..., :3][hit])  # 0 + n, as the sum makes it
    win = (W - 17, H - 9, 16, 8)
    full = reference(b)[1][0]
    want = np.ascontiguousarray(full[win[1]:win[1] + win[3], win[0]:win[0] + win[2]])
    assert want.any()
    got = s.render(b.meta, 0, 3, 1, tc.DEPTH, pt_amd.MODE_AUTO, window=win)
    assert same_bits(got, want), report(got, want)
