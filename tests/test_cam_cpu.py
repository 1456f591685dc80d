"""Cameras the scenes never use (tests/cam_cases.py), on the oracle and the host alone: the images
tests/test_gpu_cam.py compares the kernels with can see a wrong camera, and the host derives the
camera's fields as the oracle does.  CornellBox scenes at 40 x 32, the boat at 24 x 16, depth 8, a
3-frame render.  The figures are conditions on the test's inputs, no tolerances of anything under test.

- seeing cameras: light in >= 0.25 of the pixels (test_cond_cpu.lit); mixed ones (wide, top-down, the
  boat's own) in 0.05 .. 0.30, and frame 0's camera rays both hit and miss; all-miss cameras: no
  light, no shadow query, W * H * frames extension queries; `under`: no light, more queries than that.
- oblique and rolled leave no zero among the nine rotation entries of M.
- every perturbation of the oblique meta changes the bits, or keeps them, as cam_cases says; the
  roulette twins (rr 0 and -0.5; 1 and 1.5) ask the same queries.  No image has a non-finite value.
- the Node host packs a copy of each scene's XML with each camera written in: its meta equals
  scene_oracle.make_meta's byte for byte.  `up` parallel to the view direction: make_meta raises, the
  Node host writes a meta whose u and v axes are NaN.
- view_half_h as the library's host code computes it (pt_selftest_view_half_h) equals the oracle's
  po_view_half_h for meta[3] over 0.01 .. 179.99 degrees with meta[2] in {0.25, 1, 4}.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cam_cases as cc
import denoise_ref as dr
import oracle
import pt_amd
from conftest import PACK_JS, Packed, pack_with_node
from test_cond_cpu import lit

_RENDERS = {}


def render(p, key, meta):
    """(3-frame image, counters) of the oracle, once per key."""
    if key not in _RENDERS:
        _RENDERS[key] = oracle.render(p.triangle_data, p.bvh_data, meta, 0, 3, 1, cc.DEPTH)
    return _RENDERS[key]


# ---------------------------------------------------------------------------------------------
# the oracle's images
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,name", cc.CASES, ids=[cc.case_id(s, c) for s, c in cc.CASES])
def test_oracle_sees_what_the_kind_says(packed, scene, name):
    p, meta = packed[scene], cc.meta_of(scene, name)
    W, H = cc.size_of(scene)
    img, cnt = render(p, cc.case_id(scene, name), meta)
    share = float(lit(img).mean())
    print(f"{scene} {name}: lit {share:.3f}, ext {cnt['ext_queries']}, shadow {cnt['shadow_queries']}")
    assert np.isfinite(img).all()
    kind = cc.kind_of(scene, name)
    if kind == "seeing":
        assert share >= 0.25, share
    elif kind == "mixed":
        assert 0.05 <= share <= 0.30, share
        fh = dr.FirstHits(p.triangle_data, p.bvh_data, meta)
        hits = sum(fh.hit(x, y, 0)[0] is not None for y in range(H) for x in range(W))
        print(f"  frame 0: {hits} of {W * H} camera rays hit")
        assert 0 < hits < W * H, hits
    elif kind == "miss":
        assert share == 0.0 and not img.any()
        assert cnt["shadow_queries"] == 0 and cnt["ext_queries"] == W * H * 3, cnt
    else:
        assert kind == "under"
        assert share == 0.0 and not img.any()
        assert cnt["ext_queries"] > W * H * 3, cnt


def test_xml_cameras_are_the_packed_ones(packed):
    """cam_cases' "xml" meta is the `packed` fixture's own at the case's size."""
    for scene in cc.CAMERAS:
        assert cc.meta_of(scene, "xml").tobytes() == packed[scene].meta_for(*cc.size_of(scene)).tobytes(), scene


def test_the_cornell_camera_hides_the_matrix():
    """What the layer is for: the shared Cornell camera's M is the identity plus a translation; oblique
    and rolled have no zero among the nine rotation entries."""
    rot = [0, 1, 2, 4, 5, 6, 8, 9, 10]
    M = cc.meta_of("CornellBox", "xml")[28:44]
    assert [float(M[i]) for i in rot] == [1, 0, 0, 0, 1, 0, 0, 0, 1] and M[3] == M[7] == M[11] == 0 and M[15] == 1
    for scene, name in [("CornellBox", "oblique"), ("CornellBox", "rolled"), ("MedievalBoat", "rolled_low")]:
        M = cc.meta_of(scene, name)[28:44]
        assert all(M[i] != 0 for i in rot), (scene, name, M)


@pytest.mark.parametrize("name", list(cc.PERTURBATIONS))
def test_perturbations_change_or_keep_the_bits(packed, name):
    p = packed[cc.PERT_SCENE]
    base, _ = render(p, cc.case_id(cc.PERT_SCENE, "oblique"), cc.meta_of(cc.PERT_SCENE, "oblique"))
    img, cnt = render(p, "pert-" + name, cc.perturbed(name))
    expect = cc.PERTURBATIONS[name][1]
    same = img.tobytes() == base.tobytes()
    print(f"{name}: {expect}; lit {lit(img).mean():.3f}, ext {cnt['ext_queries']}, shadow {cnt['shadow_queries']}")
    assert np.isfinite(img).all()
    if expect == "same":
        assert same
    else:
        assert not same
    if expect == "dark":
        W, H = cc.size_of(cc.PERT_SCENE)
        assert not img.any() and cnt["shadow_queries"] == 0 and cnt["ext_queries"] == W * H * 3, cnt
    else:
        assert lit(img).mean() >= 0.2  # they keep light (the least: rr = NaN, 0.249)


def test_roulette_twins(packed):
    """rr <= 0 never continues a path and rr >= 1 always does: the twins ask the same queries; below 0
    nothing is ever divided by rr, so those two images are the same, from 1 on the weights differ."""
    p = packed[cc.PERT_SCENE]
    r = {n: render(p, "pert-" + n, cc.perturbed(n)) for pair in cc.RR_TWINS for n in pair}
    for a, b in cc.RR_TWINS:
        assert r[a][1] == r[b][1], (a, b, r[a][1], r[b][1])
    assert r["rr0"][0].tobytes() == r["rr-0.5"][0].tobytes()
    assert r["rr1"][0].tobytes() != r["rr1.5"][0].tobytes()
    W, H = cc.size_of(cc.PERT_SCENE)
    assert r["rr0"][1]["ext_queries"] == W * H * 3  # no second bounce


# ---------------------------------------------------------------------------------------------
# the Node host's meta for the catalogue's cameras
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    """A scene_assets directory for rewritten scene files: the shipped models by link."""
    d = tmp_path_factory.mktemp("cam") / "scene_assets"
    d.mkdir()
    os.symlink(os.path.join(cc.ASSETS, "models"), d / "models")
    return d


@pytest.mark.parametrize("scene", list(cc.CAMERAS))
def test_node_host_meta_equals_make_meta(assets, scene):
    W, H = cc.size_of(scene)
    for name in cc.CAMERAS[scene]:
        xml = cc.write_xml(scene, cc.camera(scene, name), str(assets / f"{scene}-{name}.xml"))
        p = pack_with_node(xml, str(assets.parent / f"packed-{scene}-{name}"), "--width", str(W), "--height", str(H))
        want = cc.meta_of(scene, name)
        assert p.meta.tobytes() == want.tobytes(), (scene, name, np.flatnonzero(p.meta.view(np.uint32) != want.view(np.uint32)))


def test_degenerate_up(assets):
    """`up` along the view direction leaves nothing to orthogonalise: make_meta divides by zero and
    raises; the Node host (IEEE division) packs the scene and writes NaN for the u and v axes, w and the
    position stay.  Such a meta renders an all-miss image (cam_cases' m_nan); it is no parity case."""
    c = cc.DEGENERATE_UP
    with pytest.raises(ZeroDivisionError):
        cc.meta_from(c, 40, 32)
    xml = cc.write_xml("CornellBox", c, str(assets / "CornellBox-degenerate.xml"))
    r = subprocess.run(["node", PACK_JS, xml, str(assets.parent / "packed-degenerate"), "--width", "40", "--height", "32"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    M = Packed(str(assets.parent / "packed-degenerate")).meta[28:44]
    assert np.isnan(M[[0, 1, 2, 4, 5, 6]]).all(), M
    assert M[[3, 7, 11]].tolist() == [0, 0, 0] and M[8:16].tolist() == [0, 1, 0, 0, 0, 4, 0, 1], M


# ---------------------------------------------------------------------------------------------
# view_half_h on the host
# ---------------------------------------------------------------------------------------------
def vfov_sweep():
    """meta[3] values: 0.01 .. 179.99 degrees evenly (both ends), 45 and 90 degrees with their f32
    neighbours, and 4,096 random angles in between."""
    F = np.float32
    deg = np.concatenate([np.linspace(0.01, 179.99, 2048), np.random.default_rng(7).uniform(0.01, 179.99, 4096)])
    v = (deg * np.pi / 180).astype(F)
    edge = []
    for d in (45.0, 90.0):
        x = F(d * np.pi / 180)
        edge += [np.nextafter(x, F(0)), x, np.nextafter(x, F(4))]
    return np.concatenate([v, np.array(edge, F)])


@pytest.mark.parametrize("focal", [0.25, 1.0, 4.0])
def test_view_half_h_on_the_host_equals_the_oracles(focal):
    v = vfov_sweep()
    assert v[0] == np.float32(0.01 * np.pi / 180) and v[2047] == np.float32(179.99 * np.pi / 180) and len(v) == 6150
    metas = np.tile(cc.meta_of("CornellBox", "oblique"), (len(v), 1))
    metas[:, 2], metas[:, 3] = focal, v
    got = pt_amd.selftest_view_half_h(metas)
    f = oracle.lib().po_view_half_h
    want = np.array([f(m.ctypes.data_as(ctypes.c_void_p)) for m in metas], np.float32)
    assert np.isfinite(want).all() and (want > 0).all()
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), v[bad][:5], got[bad][:5], want[bad][:5])
