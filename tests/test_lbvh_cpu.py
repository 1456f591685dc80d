"""The LBVH on the host (pt_bvh_build_lbvh, csrc/pt_lbvh_host.cpp; the tree's rules: include/pt_hip.h) —
CPU only.  The device builder is compared with this one byte for byte in tests/test_gpu_lbvh.py, so what
is checked here is that the host's tree is the one the header describes and a tree the unchanged
traversal can walk:
  * tests/test_bvh_sah.py's check_sah: every record in exactly one leaf, boxes that contain what is below
    them and are nowhere flat, pre-order layout; and the leaf-size rule: a leaf exceeds max_leaf only at
    the depth cap or as the emitter leaf;
  * the leaves' entries, read in pre-order, are the records in the order of a numpy restatement of the
    key (tests/lbvh_inputs.py restated_order), the emitter leaf first in record order;
  * scripts/scene_layout_harness.cpp (build_layout) accepts tree and mesh, max_stack < 32;
  * the oracle's 3-frame 40x32 render on the tree carries light (scene inputs: the hand-made meshes
    have no camera).  The lit shares are printed, and recorded in DESIGN.md §5.18, not gated;
  * bad indices, materials and a NaN vertex are refused;
  * scripts/lbvh_harness.cpp runs the builder under -fsanitize=address,undefined in a program of its own.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import pt_amd
from conftest import ROOT, SCENES, pack_with_node
from lbvh_inputs import K_MAX_DEPTH, MAX_LEAVES, handmade, restated_order, scene_inputs, triangle_data
from test_bvh_sah import check_sah, walk_packed

CSRC = os.path.join(ROOT, "brown-cs2240-path-tracer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SCENE_NAMES = ["CornellBox", "CornellBox-Mirror", "CornellBox-Glossy", "CornellBox-Sphere", "MedievalBoat", "CornellBox2-all",
               "synth36", "synth1000", "synth12500", "emitters288", "giant", "nearly_giant"]
HAND_NAMES = ["copies40", "single", "shrinking400", "flat_axis", "chain", "all_flagged", "none_flagged"]
PARAMS = [(m, iso) for m in MAX_LEAVES for iso in (True, False)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, packed):
    base = tmp_path_factory.mktemp("lbvh")
    sc = scene_inputs(base, packed)
    out = {n: (p.triangle_data, p) for n, p in sc.items()}
    out.update({n: (t, None) for n, t in handmade().items()})
    assert sorted(out) == sorted(SCENE_NAMES + HAND_NAMES)
    return out


@pytest.fixture(scope="module")
def layout_harness(tmp_path_factory):
    assert os.path.exists(HIPCC) or shutil.which("hipcc"), "no hipcc"
    d = tmp_path_factory.mktemp("lbvh_layout")
    exe = str(d / "scene_layout_harness")
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                    "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "scripts", "scene_layout_harness.cpp"),
                    *[os.path.join(CSRC, n) for n in ("pt_scene_layout.cpp", "pt_leafbvh.cpp", "pt_leafskip.cpp")],
                    "-o", exe], check=True, capture_output=True)

    def run(tri, bvh):
        tri.tofile(str(d / "triangle_data.f32"))
        bvh.tofile(str(d / "bvh_data.f32"))
        return subprocess.run([exe, str(d / "triangle_data.f32"), str(d / "bvh_data.f32")], check=True,
                              capture_output=True, text=True, timeout=300).stdout.splitlines()
    return run


def mesh_of(tri):
    nv, i0, m0 = int(tri[0]), int(tri[3]), int(tri[4])
    return tri[16:16 + 3 * nv].reshape(-1, 3).astype(np.float64), tri[i0:m0].reshape(-1, 4).astype(np.int32)


@pytest.mark.parametrize("max_leaf,iso", PARAMS)
@pytest.mark.parametrize("name", SCENE_NAMES + HAND_NAMES)
def test_lbvh_tree(inputs, layout_harness, name, max_leaf, iso):
    tri, p = inputs[name]
    bvh = pt_amd.bvh_build_lbvh(tri, max_leaf=max_leaf, isolate_emitters=iso)
    verts, recs = mesh_of(tri)
    lit, rest = restated_order(tri, iso)
    leaves = check_sah(verts, recs, bvh, emitter_leaf=lit is not None)
    # the leaf-size rule, and the depth cap
    for i, (e, _, _, depth) in enumerate(leaves):
        assert len(e) <= max_leaf or depth >= K_MAX_DEPTH or (i == 0 and lit is not None), (len(e), depth)
        assert depth <= K_MAX_DEPTH
    # the order of the entries
    if lit is not None:
        assert np.array_equal(leaves[0][0], lit), "the emitter leaf: the flagged records in record order"
        leaves = leaves[1:]
    assert np.array_equal(np.concatenate([e for e, _, _, _ in leaves]), rest), "the leaves follow the sorted keys"
    # build_layout takes the tree
    got = layout_harness(tri, bvh)
    assert got[0] == "rc 0", got[:2]
    info = next(ln for ln in got if ln.startswith("info ")).split()
    assert int(info[info.index("max_stack") + 1]) < 32
    # the oracle's render on it carries light
    if p is not None:
        W, H = (24, 16) if name == "MedievalBoat" else (40, 32)
        acc, _ = oracle.render(tri, bvh, p.meta_for(W, H), 0, 3, 1, 8)
        share = float((acc.reshape(-1, 3).sum(1) > 0).mean())
        print(f"lit share {name} max_leaf={max_leaf} isolate={int(iso)}: {share:.3f}")
        assert share > 0, "the render on the LBVH tree is black"


def test_lbvh_two_leaf_root(inputs):
    """A tree that would be one leaf: two leaves under the root, the first n / 2 records and the rest; a
    single record leaves the left one empty with a zero box."""
    tri, _ = inputs["single"]
    bvh = pt_amd.bvh_build_lbvh(tri, max_leaf=4, isolate_emitters=False)
    leaves, _ = walk_packed(bvh)
    assert [len(e) for e, _, _, _ in leaves] == [0, 1]
    assert not bvh[6 + 5: 6 + 11].any() and len(bvh) == 6 + 17 + 17 + 17 + 4
    five = triangle_data([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 2, 3, 0]] * 5, [(1.0, 1.0, 1.0)])
    bvh = pt_amd.bvh_build_lbvh(five, max_leaf=8, isolate_emitters=False)
    assert [len(e) for e, _, _, _ in walk_packed(bvh)[0]] == [2, 3]


def test_lbvh_depth_cap(inputs):
    """The chain's comb is cut at the cap: a leaf at depth PT_LBVH_MAX_DEPTH holding more than max_leaf."""
    tri, _ = inputs["chain"]
    for iso in (True, False):
        leaves, _ = walk_packed(pt_amd.bvh_build_lbvh(tri, max_leaf=1, isolate_emitters=iso))
        assert max(d for _, _, _, d in leaves) == K_MAX_DEPTH
        assert any(len(e) > 1 for e, _, _, d in leaves if d == K_MAX_DEPTH)


def test_lbvh_default_params(inputs):
    tri, _ = inputs["synth1000"]
    assert np.array_equal(pt_amd.bvh_build_lbvh(tri).view(np.uint32),
                          pt_amd.bvh_build_lbvh(tri, max_leaf=4, isolate_emitters=True).view(np.uint32))


def test_lbvh_refuses_bad_input(inputs):
    tri, _ = inputs["CornellBox"]
    i0 = int(tri[3])
    for at, val in ((i0, 0.0), (i0 + 1, tri[0] + 1), (i0 + 3, tri[1]), (i0 + 3, -1.0)):
        bad = tri.copy()
        bad[at] = val
        with pytest.raises(pt_amd.PtError):
            pt_amd.bvh_build_lbvh(bad)
    bad = tri.copy()
    bad[16 + 3 * (int(tri[i0]) - 1) + 1] = np.nan  # a coordinate of the first record's first vertex
    with pytest.raises(pt_amd.PtError):
        pt_amd.bvh_build_lbvh(bad)
    for max_leaf in (0, 9):
        with pytest.raises(pt_amd.PtError):
            pt_amd.bvh_build_lbvh(tri, max_leaf=max_leaf)


def test_node_lbvh_pack(tmp_path):
    """The Node host's --bvh lbvh packs through pt_bvh_build_lbvh (bvhBuildLbvh), --max-leaf reaching it."""
    xml = os.path.join(SCENES, "scene_assets", "CornellBox-Glossy.xml")
    p = pack_with_node(xml, str(tmp_path / "p"), "--bvh", "lbvh")
    assert np.array_equal(p.bvh_data.view(np.uint32), pt_amd.bvh_build_lbvh(p.triangle_data).view(np.uint32))
    p8 = pack_with_node(xml, str(tmp_path / "p8"), "--bvh", "lbvh", "--max-leaf", "8")
    assert np.array_equal(p8.bvh_data.view(np.uint32), pt_amd.bvh_build_lbvh(p.triangle_data, max_leaf=8).view(np.uint32))
    assert p8.bvh_data.size != p.bvh_data.size


def test_lbvh_host_builder_under_sanitizers(inputs, tmp_path):
    """The host builder in a program of its own (scripts/lbvh_harness.cpp) under ASan and UBSan: clean, and
    the same bytes as the library's."""
    exe = str(tmp_path / "lbvh_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "scripts", "lbvh_harness.cpp"),
                    os.path.join(CSRC, "pt_lbvh_host.cpp"), "-o", exe], check=True, capture_output=True)
    for name in ("CornellBox-Glossy", "synth1000", "emitters288", "shrinking400", "single", "copies40", "giant"):
        tri, _ = inputs[name]
        tri.tofile(str(tmp_path / "t.f32"))
        for max_leaf, iso in ((1, 1), (4, 1), (8, 0)):
            r = subprocess.run([exe, str(tmp_path / "t.f32"), str(tmp_path / "b.f32"), str(max_leaf), str(iso)],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr[-2000:]
            want = pt_amd.bvh_build_lbvh(tri, max_leaf=max_leaf, isolate_emitters=bool(iso))
            assert np.array_equal(np.fromfile(str(tmp_path / "b.f32"), np.uint32), want.view(np.uint32))
