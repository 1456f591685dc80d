"""No GPU: the restatement of the lens cameras (lens_ref.py) pinned against what is not itself — the
pinhole's seeds and rays (radiance_ref.camera_seed, denoise_ref.camera_ray), the geometry each model
promises — and, on the oracle alone, the light the shared cases carry.  What of the feature needs no device
is checked here too: the header, the symbols, the kernels' names in the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import cam_cases as cc
import denoise_ref as dr
import lens_ref as lr
import oracle
import pt_amd
import radiance_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W, H = 40, 32
FRAMES = (0, 5)
GEOMETRY = [("CornellBox", "oblique"), ("CornellBox", "rolled")]  # no zero in M's rotation: a transposed block shows
BIG = 1 << 22  # an image so fine that a pixel is a point of the unit square to 2.4e-7


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("radiance_ref"))


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def pixels(step=3):
    return [(x, y) for y in range(0, H, step) for x in range(0, W, step)] + [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]


def test_header_and_symbols():
    with open(os.path.join(ROOT, "include", "pt_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define PT_ABI_VERSION 3\b", text)  # additions keep the version
    for name in ("pt_scene_set_camera", "pt_scene_get_camera"):
        assert re.search(rf"\bint {name}\(", text), name
        assert hasattr(pt_amd.load_library(), name), name
    assert "pt_camera_model" in text and ctypes.sizeof(pt_amd.Camera) == 16
    assert pt_amd.CAMERA_MODELS == ("pinhole", "thin_lens", "ortho", "equirect")
    assert "pt_capi_camera.hip" in pt_amd._lib._BUILD_SRCS
    with open(pt_amd.lib_path(), "rb") as f:
        data = f.read()
    for kernel in (b"k_wf_generate_cam", b"k_features_cam", b"k_camera_rays_cam"):
        assert kernel in data, kernel


@pytest.mark.parametrize("model", lr.MODELS[1:])
def test_seeds_are_the_pinholes(model):
    meta = cc.meta_of("CornellBox", "oblique", (W, H))
    for t in FRAMES:
        for x, y in pixels(5):
            assert lr.camera_ray(meta, (model, 0.2, 3.6), x, y, t)[2] == rr.camera_seed(meta, x, y, t), (x, y, t)


@pytest.mark.parametrize("scene,camera", GEOMETRY, ids=[c for _, c in GEOMETRY])
def test_thin_lens_geometry(scene, camera):
    meta = cc.meta_of(scene, camera, (W, H))
    M = np.asarray(meta[28:44], np.float64)
    c0, c1, c2, x0 = M[0:3], M[4:7], M[8:11], M[12:15]
    radius, focus = 0.3, 3.6
    quadrants = set()
    for t in FRAMES:
        for y in range(H):
            for x in range(W):
                if t == FRAMES[1] and (x % 3 or y % 3):
                    continue
                o, d, _, target = (np.asarray(v, np.float64) for v in lr.camera_ray(meta, ("thin_lens", radius, focus), x, y, t))
                # o + |X(c) - o| d returns to X(c)
                s = np.linalg.norm(target - o)
                assert np.linalg.norm(o + s * d - target) <= 1e-5 * s, (x, y, t)
                # X(c) lies on the pinhole's ray of the same pixel and frame
                po, pd = dr.camera_ray(meta, x, y, t)
                po, pd = np.asarray(po[:3], np.float64), unit(pd[:3])
                v = target - po
                assert np.linalg.norm(v - np.dot(v, pd) * pd) <= 1e-5 * np.linalg.norm(v), (x, y, t)
                assert abs(np.dot(v, -unit(c2)) - focus) <= 1e-5 * focus  # ... on the plane of focus
                # the lens point: within the radius of X(0), in the plane of M's first two columns
                lp = o - x0
                a, b = np.dot(lp, c0) / np.dot(c0, c0), np.dot(lp, c1) / np.dot(c1, c1)
                assert abs(np.dot(lp, unit(c2))) <= 1e-5 * radius
                assert np.hypot(a, b) <= radius * (1 + 1e-5)
                if t == FRAMES[0]:
                    quadrants.add((a > 0, b > 0))
    assert len(quadrants) == 4


@pytest.mark.parametrize("scene,camera", GEOMETRY, ids=[c for _, c in GEOMETRY])
def test_ortho_geometry(scene, camera):
    meta = cc.meta_of(scene, camera, (W, H))
    M = np.asarray(meta[28:44], np.float64)
    focus = 3.6
    dirs, origins = [], {}
    for x, y in pixels():
        o, d, _, _ = lr.camera_ray(meta, ("ortho", 0.0, focus), x, y, 0)
        dirs.append(d.view(np.uint32).copy())
        origins[(x, y)] = np.asarray(o, np.float64)
        # the image is what the pinhole sees at the plane of focus
        po, pd = dr.camera_ray(meta, x, y, 0)
        v = origins[(x, y)] + focus * np.asarray(d, np.float64) - np.asarray(po[:3], np.float64)
        pd = unit(pd[:3])
        assert np.linalg.norm(v - np.dot(v, pd) * pd) <= 1e-5 * np.linalg.norm(v), (x, y)
    assert all((b == dirs[0]).all() for b in dirs)
    assert np.allclose(unit(np.asarray(lr.camera_ray(meta, ("ortho", 0.0, focus), 0, 0, 0)[1], np.float64)), -unit(M[8:11]), atol=1e-6)
    # the origins span the pinhole's extent there: 2 tan(vfov / 2) * focus high, aspect times as wide, to a pixel
    vhh = float(F(oracle.lib().po_view_half_h(np.ascontiguousarray(meta, F).ctypes.data_as(ctypes.c_void_p))))
    height, width = vhh * focus / float(meta[2]), vhh * float(meta[10]) * focus / float(meta[2])
    span_w = np.linalg.norm(origins[(W - 1, 0)] - origins[(0, 0)])
    span_h = np.linalg.norm(origins[(0, H - 1)] - origins[(0, 0)])
    assert width * (1 - 2.5 / W) <= span_w <= width and height * (1 - 2.5 / H) <= span_h <= height


def test_equirect_geometry():
    cam = ("equirect", 0.0, 1.0)
    for scene, camera in GEOMETRY:
        big = cc.meta_of(scene, camera, (BIG, BIG))
        M = np.asarray(big[28:44], np.float64)
        # the centre pixel looks along the pinhole's centre ray
        o, d, _, _ = lr.camera_ray(big, cam, BIG // 2, BIG // 2, 0)
        po, pd = dr.camera_ray(big, BIG // 2, BIG // 2, 0)
        assert (o == po[:3]).all()
        assert np.linalg.norm(unit(d) - unit(pd[:3])) <= 1e-5
        assert np.linalg.norm(unit(d) + unit(M[8:11])) <= 1e-5
        # the left and the right edge meet (behind the camera)
        dl = lr.camera_ray(big, cam, 0, BIG // 2, 0)[1]
        dr_ = lr.camera_ray(big, cam, BIG - 1, BIG // 2, 0)[1]
        assert np.linalg.norm(unit(dl) - unit(dr_)) <= 1e-5
        assert np.linalg.norm(unit(dl) - unit(M[8:11])) <= 1e-5
        # a quarter turn to the right of the centre looks along M's first column
        dq = lr.camera_ray(big, cam, 3 * BIG // 4, BIG // 2, 0)[1]
        assert np.linalg.norm(unit(dq) - unit(M[0:3])) <= 1e-5
        # row 0 looks up
        meta = cc.meta_of(scene, camera, (W, H))
        for x in range(0, W, 7):
            assert np.dot(unit(lr.camera_ray(meta, cam, x, 0, 0)[1]), unit(M[4:7])) >= np.cos(np.pi / H) - 1e-5
        assert np.linalg.norm(unit(lr.camera_ray(big, cam, BIG // 3, 0, 0)[1]) - unit(M[4:7])) <= 1e-5


@pytest.mark.parametrize("case", lr.CASES, ids=[lr.case_id(c) for c in lr.CASES])
def test_cases_are_admitted_and_lit(packed, ref, case):
    """Every ray of the shared cases is admitted, and the 3-frame image carries light in >= 0.25 of its
    pixels: a test that compares these images does not pass on black."""
    meta, acc, cnt, frames = lr.reference(ref, packed, case)
    for rays, seeds, adm in frames:
        assert np.isfinite(rays[..., :3]).all() and np.isfinite(rays[..., 4:7]).all()
        assert adm.all()
    assert cnt["samples"] == lr.NFRAMES * acc.shape[0] * acc.shape[1]
    share = float((acc.sum(axis=2) > 0).mean())
    print(f"lit share {lr.case_id(case)}: {share:.3f}")
    assert share >= 0.25
