"""Trees no builder here produces (tests/tree_cases.py), on the oracle and the host alone: the layout
harness (scripts/scene_layout_harness.cpp) accepts every case and reports what the catalogue states;
the trees that must not change the image do not; the images are worth comparing; and the rays reach
the leaves the cases are about.  The figures are conditions on the test's inputs, no tolerances of
anything under test.  CPU only.

- facts: the harness's max_stack, node count, max_leaf and mailbox verdict equal tree_cases.facts() of
  the packed buffer and what the case's construction fixes; the replay tree exists exactly for
  U <= 63 and <= 64 nodes, its narrow payload exactly for U <= 32 and <= 32 nodes, and every word of
  both follows from the harness's own node and uid tables (an empty child's word is 0; a leaf's set
  never has the inner flag).  max_stack 32 is refused with code -2.
- stilts, bushes and relayouts keep the oracle's frame and 3-frame render bit for bit; the counters
  grow by the walked nodes added per query that enters the outer bounds: linearly in k, and on the
  camera rays of one frame by k times the rays for which oracle.ray_bbox of the bounds is positive.
- every 3-frame render is finite and lit in >= 1/4 of its pixels (U <= 2: measured 0.518 and 0.255 from
  cam_cases' tele3, not bounded).
- chains and added leaves: the camera rays of the frame hit an entry of the deepest (added) leaf in
  >= 16 pixels.
"""
import numpy as np
import pytest

import cam_cases as cc
import denoise_ref as dr
import oracle
import tree_cases as tc
from test_cond_cpu import lit
from test_scene_layout import harness  # noqa: F401  (the fixture: the harness, compiled once per module)

REFUSED = "BVH deeper than the device traversal stack"


@pytest.fixture(scope="module")
def bases(packed, tmp_path_factory):
    return tc.bases(packed, tmp_path_factory.mktemp("trees"))


def run_harness(harness, tmp_path, tri, bvh, *args):  # noqa: F811
    np.asarray(tri, np.float32).tofile(str(tmp_path / "triangle_data.f32"))
    np.asarray(bvh, np.float32).tofile(str(tmp_path / "bvh_data.f32"))
    return harness(str(tmp_path), *args)


def field(lines, head, key):
    words = next(ln for ln in lines if ln.startswith(head + " ")).split()
    return int(words[words.index(key) + 1])


_RENDERS = {}


def render(b, key):
    if key not in _RENDERS:
        _RENDERS[key] = (oracle.frame(b.triangle_data, b.bvh_data, b.meta, tc.SALT, tc.DEPTH),
                         oracle.render(b.triangle_data, b.bvh_data, b.meta, 0, 3, 1, tc.DEPTH))
    return _RENDERS[key]


class Plain:
    """The case's base scene under the case's camera."""

    def __init__(self, case, p):
        self.triangle_data, self.bvh_data = p.triangle_data, p.bvh_data
        self.meta = cc.meta_of(tc.camera_scene(case.base), case.cam, tc.size_of(case.base))


# ---------------------------------------------------------------------------------------------
# the layout harness
# ---------------------------------------------------------------------------------------------
def check_replay_words(lines, f):
    nd = {int(w[1]): tuple(map(int, w[2:6])) for w in (ln.split() for ln in lines if ln.startswith("nd "))}
    uid = {int(w[1]): int(w[2]) for w in (ln.split() for ln in lines if ln.startswith("uid "))}
    bf = [ln.split() for ln in lines if ln.startswith("bf ")]
    bn = [ln.split() for ln in lines if ln.startswith("bn ")]
    assert len(bf) == (f["nodes"] if f["replay"] else 0), (len(bf), f)
    assert len(bn) == (f["nodes"] if f["narrow"] else 0), (len(bn), f)
    if not bf:
        return
    order, st = [], [0]  # the visiting order: pre-order, right subtree first
    while st:
        n = st.pop()
        order.append(n)
        lref, rref, lcnt, rcnt = nd[n]
        st += [lref] * (lcnt < 0) + [rref] * (rcnt < 0)
    pre = {n: i for i, n in enumerate(order)}
    assert [int(w[2]) for w in bf] == order

    def leaf_set(ref, cnt):
        m = 0
        for r in range(ref, ref + cnt):
            m |= 1 << uid[r]
        return m

    def below(ref, cnt):
        if cnt >= 0:
            return leaf_set(ref, cnt)
        lref, rref, lcnt, rcnt = nd[ref]
        return below(lref, lcnt) | below(rref, rcnt)
    for i, w in enumerate(bf):
        lref, rref, lcnt, rcnt = nd[order[i]]
        for word, ref, cnt in ((int(w[3], 16), lref, lcnt), (int(w[4], 16), rref, rcnt)):
            want = (1 << 63) | pre[ref] if cnt < 0 else leaf_set(ref, cnt)
            assert word == want and (cnt < 0 or word >> 63 == 0), (i, hex(word), hex(want), cnt)
        if bn:
            for word, ref, cnt in ((int(bn[i][2], 16), lref, lcnt), (int(bn[i][3], 16), rref, rcnt)):
                hi = (0x80000000 | pre[ref]) if cnt < 0 else 0
                assert word == (hi << 32 | below(ref, cnt)), (i, hex(word), cnt)


@pytest.mark.parametrize("cid", tc.IDS)
def test_harness_reports_what_the_catalogue_states(harness, bases, tmp_path, cid):  # noqa: F811
    b = tc.built(bases, cid)
    f = tc.facts(b.bvh_data)
    for k, v in b.case.expect.items():
        if k != "fits_lds":
            assert f[k] == v, (k, f)
    got = run_harness(harness, tmp_path, b.triangle_data, b.bvh_data, "dump_bf")
    assert got[0] == "rc 0", got[:2]
    assert field(got, "info", "max_stack") == f["max_stack"] < tc.STACK_MAX
    assert field(got, "info", "nodes") == f["nodes"] and field(got, "info", "leaves") == f["leaves"]
    assert field(got, "info", "max_leaf") == f["max_leaf"]
    assert field(got, "leaf_min", "mailbox") == int(f["mailbox"])
    check_replay_words(got, f)
    fits = tc.fits_lds(f["max_stack"], field(got, "span_end", "span_end"))
    print(f"{cid}: {f}, span {field(got, 'span_end', 'span_end')} B, fits LDS {fits}")
    if "fits_lds" in b.case.expect:
        assert fits == b.case.expect["fits_lds"]
    elif b.case.base in ("CornellBox-Glossy", "CornellBox-Sphere", "MedievalBoat"):
        assert not fits  # their spans alone are 0.4 .. 3.6 MB
    elif f["mailbox"]:
        assert fits


@pytest.mark.parametrize("scene,k", [("CornellBox", 27), ("MedievalBoat", 17)])
def test_max_stack_32_is_refused(harness, packed, tmp_path, scene, k):  # noqa: F811
    p = packed[scene]
    ok = tc.stilts(p.bvh_data, k - 1, "Z")
    assert tc.facts(ok)["max_stack"] == 31 and run_harness(harness, tmp_path, p.triangle_data, ok)[0] == "rc 0"
    deep = tc.stilts(p.bvh_data, k, "Z")
    assert tc.facts(deep)["max_stack"] == 32
    got = run_harness(harness, tmp_path, p.triangle_data, deep)
    assert got[0] == "rc -2" and got[1] == f"msg [{REFUSED}]", got


def test_decode_and_pack_round_trip(bases):
    """decode() then scene_oracle.pack_bvh gives back every builder tree byte for byte, and each
    relayout decodes to the same tree."""
    for name, p in bases.items():
        assert tc.pack(tc.decode(p.bvh_data)).tobytes() == p.bvh_data.tobytes(), name
        for how in tc.LAYOUTS:
            again = tc.relayout(p.bvh_data, how)
            assert again.tobytes() != p.bvh_data.tobytes()
            assert tc.pack(tc.decode(again)).tobytes() == p.bvh_data.tobytes(), (name, how)


# ---------------------------------------------------------------------------------------------
# the oracle's images
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", tc.IDS)
def test_render_is_finite_and_lit(bases, cid):
    b = tc.built(bases, cid)
    (fr, _), (img, cnt) = render(b, cid)
    share = float(lit(img).mean())
    print(f"{cid}: lit {share:.3f}, nodes {cnt['nodes']}, tri_tests {cnt['tri_tests']}")
    assert np.isfinite(img).all() and np.isfinite(fr).all()
    if not b.case.dim:
        assert share >= 0.25, share
    else:
        assert share > 0


SAME = [c.id for c in tc.CASES if c.same_image]


@pytest.mark.parametrize("cid", SAME)
def test_same_image_more_nodes(bases, cid):
    b = tc.built(bases, cid)
    base = Plain(b.case, bases[b.case.base])
    (fr, fc), (img, rc) = render(b, cid)
    (fr0, fc0), (img0, rc0) = render(base, ("plain", b.case.base, b.case.cam))
    assert fr.tobytes() == fr0.tobytes() and img.tobytes() == img0.tobytes()
    added = tc.facts(b.bvh_data)["nodes"] - tc.facts(base.bvh_data)["nodes"]
    for c, c0 in ((fc, fc0), (rc, rc0)):
        for key in ("samples", "ext_queries", "shadow_queries", "tri_tests"):
            assert c[key] == c0[key], (key, c, c0)
        dn = c["nodes"] - c0["nodes"]
        assert c["box_tests"] - c0["box_tests"] == 2 * dn
        if added == 0:
            assert dn == 0
        else:  # every added node is walked by the same queries: those that enter the outer bounds
            assert dn > 0 and dn % added == 0 and dn // added <= c["ext_queries"] + c["shadow_queries"], (dn, added)


@pytest.mark.parametrize("cid", ["stilts-CornellBox-31Z", "fat-stilts-CornellBox-31L", "bush-CornellBox-65",
                                 "stilts-MedievalBoat-31L"])
def test_added_nodes_are_walked_by_the_rays_that_enter_the_bounds(bases, cid):
    """Frame SALT's camera rays one by one: oracle.intersect's node count grows by the nodes added
    where oracle.ray_bbox of the outer bounds is positive, and by nothing elsewhere."""
    b = tc.built(bases, cid)
    base = bases[b.case.base]
    added = tc.facts(b.bvh_data)["nodes"] - tc.facts(base.bvh_data)["nodes"]
    W, H = b.size
    inside = 0
    for y in range(H):
        for x in range(W):
            o, d = dr.camera_ray(b.meta, x, y, tc.SALT)
            enters = oracle.ray_bbox(o[:3], d[:3], base.bvh_data[0:3], base.bvh_data[3:6]) > 0
            _, _, c0 = oracle.intersect(base.triangle_data, base.bvh_data, o, d)
            _, _, c1 = oracle.intersect(b.triangle_data, b.bvh_data, o, d)
            assert c1["nodes"] - c0["nodes"] == (added if enters else 0), (x, y, enters)
            assert c1["tri_tests"] == c0["tri_tests"]
            inside += enters
    assert 0 < inside
    print(f"{cid}: {inside} of {W * H} camera rays enter the bounds, {added} nodes each")


PROBED = [c.id for c in tc.CASES if c.probe]
_RAYS = {}


def camera_rays(b):
    key = b.meta.tobytes()
    if key not in _RAYS:
        W, H = b.size
        _RAYS[key] = [dr.camera_ray(b.meta, x, y, tc.SALT) for y in range(H) for x in range(W)]
    return _RAYS[key]


@pytest.mark.parametrize("cid", PROBED)
def test_reach(bases, cid):
    b = tc.built(bases, cid)
    want = tc.EntrySet(b.triangle_data, sorted(tc.probe_entries(b.bvh_data, b.case.probe)))
    n = 0
    for o, d in camera_rays(b):
        ok, out, _ = oracle.intersect(b.triangle_data, b.bvh_data, o, d)
        n += bool(ok) and want.on(o, d, out[6])
    print(f"{cid}: {n} pixels hit an entry of the {b.case.probe} leaf")
    assert n >= 16, n
