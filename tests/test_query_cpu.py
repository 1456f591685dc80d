"""Ray queries (pt_query_hits, pt_query_occluded, pt_camera_rays), the checks that need no GPU: the
header and the ABI, the structs' sizes, the exported symbols, every argument check that precedes the
first device call, the two options, the reference batches' mix (query_ref.py) on all four scenes, the
oracle's termination on the odd rays, and the kernels' hand-out arithmetic (csrc/pt_query_plan.h) in a
stand-alone program (scripts/query_plan_harness.cpp) built with -fsanitize=address,undefined."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pt_amd
import query_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "brown-cs2240-path-tracer_amd")
HEADER = os.path.join(ROOT, "include", "pt_hip.h")
FUNCTIONS = ("pt_query_hits", "pt_query_hits_async", "pt_query_occluded", "pt_query_occluded_async", "pt_camera_rays",
             "pt_camera_rays_async")
SCENES = ("CornellBox", "CornellBox-Glossy", "CornellBox-Sphere", "MedievalBoat")


def test_header_declares_queries_and_structs():
    text = open(HEADER).read()
    for f in FUNCTIONS:
        assert re.search(rf"\bint {f}\s*\(pt_scene\*", text), f
    assert re.search(r"typedef struct \{ float o\[3\]; float tmax; float d\[3\]; uint32_t reserved; \} pt_ray;", text)
    assert re.search(r"typedef struct \{ float p\[3\]; float t;\s+float n\[3\]; int32_t\s+material; \} pt_hit;", text)
    assert re.search(r"#define PT_ABI_VERSION 3\b", text)
    for opt in ("query_refill", "query_blocks"):
        assert f'"{opt}"' in text


def test_struct_sizes_and_abi():
    assert ctypes.sizeof(pt_amd.Ray) == 32 and ctypes.sizeof(pt_amd.Hit) == 32
    assert pt_amd.Ray.d.offset == 16 and pt_amd.Ray.tmax.offset == 12 and pt_amd.Hit.t.offset == 12
    assert pt_amd.Hit.n.offset == 16 and pt_amd.Hit.material.offset == 28
    assert pt_amd.RAY_DTYPE.itemsize == 32 and pt_amd.HIT_DTYPE.itemsize == 32
    assert pt_amd.abi_version() == 3 == pt_amd.ABI_VERSION


def test_library_exports_the_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", pt_amd.lib_path()], capture_output=True, text=True).stdout
    for f in FUNCTIONS:
        assert re.search(rf"\bT {f}\b", out), f
    # the kernels are in the device code: hits and occlusion, plain and big-leaf, counting and not
    data = open(pt_amd.lib_path(), "rb").read()
    assert data.count(b"k_camera_rays") >= 1 and b"k_query" in data


def _err(lib):
    return lib.pt_last_error().decode()


def test_argument_checks_before_any_device_call():
    """Every check here precedes the scene's first use, so a NULL scene reaches each of them; the message
    tells which one answered."""
    lib = pt_amd.load_library()
    buf = np.zeros(64, np.float32)  # numpy allocations are 16-byte aligned
    base = buf.ctypes.data
    assert base % 16 == 0
    p = ctypes.c_void_p
    for fn, asyn in ((lib.pt_query_hits, False), (lib.pt_query_hits_async, True), (lib.pt_query_occluded, False),
                     (lib.pt_query_occluded_async, True)):
        tail = (None, None) if asyn else (None,)
        assert fn(None, p(base), (1 << 30) + 1, p(base + 64), *tail) == -1 and "2^30" in _err(lib)
        assert fn(None, None, 1, p(base + 64), *tail) == -1 and "null ray or result" in _err(lib)
        assert fn(None, p(base), 1, None, *tail) == -1 and "null ray or result" in _err(lib)
        assert fn(None, p(base), 1, p(base + 64), *tail) == -1 and "null scene" in _err(lib)
        assert fn(None, None, 0, None, *tail) == -1 and "null scene" in _err(lib)  # n = 0 still needs a scene
    for fn, out in ((lib.pt_query_hits_async, base + 64), (lib.pt_query_occluded_async, base + 64)):
        assert fn(None, p(base + 4), 1, p(out), None, None) == -1 and "16-byte aligned" in _err(lib)
    assert lib.pt_query_hits_async(None, p(base), 1, p(base + 72), None, None) == -1 and "16-byte aligned" in _err(lib)
    # the blocking forms take host buffers of any alignment the types allow (they copy into the scene's scratch):
    # rays at base + 4 pass the alignment rule and reach the next check
    for fn in (lib.pt_query_hits, lib.pt_query_occluded):
        assert fn(None, p(base + 4), 1, p(base + 68), None) == -1 and "null scene" in _err(lib)
    # the occlusion bytes may sit anywhere
    assert lib.pt_query_occluded_async(None, p(base), 1, p(base + 65), None, None) == -1 and "null scene" in _err(lib)
    meta = np.zeros(48, np.float32)
    meta[0] = meta[1] = 8
    mp = meta.ctypes.data_as(p)
    assert lib.pt_camera_rays(None, mp, None, 1 << 24, p(base)) == -1 and "2^24" in _err(lib)
    assert lib.pt_camera_rays_async(None, mp, None, 1 << 24, p(base), None) == -1 and "2^24" in _err(lib)
    assert lib.pt_camera_rays(None, None, None, 0, p(base)) == -1 and "null" in _err(lib)
    assert lib.pt_camera_rays(None, mp, None, 0, None) == -1 and "null" in _err(lib)
    assert lib.pt_camera_rays_async(None, mp, None, 0, p(base + 4), None) == -1 and "16-byte aligned" in _err(lib)
    assert lib.pt_camera_rays(None, mp, None, (1 << 24) - 1, p(base)) == -1 and "null scene" in _err(lib)


def test_binding_rejects_ragged_rays():
    with pytest.raises(pt_amd.PtError):
        pt_amd._lib._rays(np.zeros(7, np.float32))
    r = pt_amd._lib._rays(np.zeros(3, pt_amd.RAY_DTYPE))
    assert r.shape == (3, 8) and r.dtype == np.float32


def test_options_accept_and_reject():
    pt_amd.reset_options()
    try:
        for v in (0, 1):
            pt_amd.set_option("query_refill", v)
            assert pt_amd.get_option("query_refill") == str(v)
        for bad in ("2", "-1", "on", ""):
            with pytest.raises(pt_amd.PtError):
                pt_amd.set_option("query_refill", bad)
        for v in (0, 1, 4096):
            pt_amd.set_option("query_blocks", v)
            assert pt_amd.get_option("query_blocks") == str(v)
        for bad in ("-1", "x", "1.5"):
            with pytest.raises(pt_amd.PtError):
                pt_amd.set_option("query_blocks", bad)
        pt_amd.set_option("query_refill", None)
        assert pt_amd.get_option("query_refill") == ""
    finally:
        pt_amd.reset_options()


@pytest.mark.parametrize("scene", SCENES)
def test_batches_are_mixed(packed, scene):
    """With the oracle alone: the odd rays terminate, the hits batch holds at least 10 % hits and 10 %
    misses, the occlusion batch at least 25 % of each value, and the derived rays pin the boundary."""
    b = qr.batch(scene, packed)
    assert b.odd_terminate
    assert (b.family == "odd").sum() == 6
    sh = b.shares()
    print(scene, sh)
    assert sh["hits"] >= 0.10 and sh["misses"] >= 0.10, sh
    assert sh["ones"] >= 0.25 and sh["zeros"] >= 0.25, sh
    w, h = qr.camera_size(scene)
    assert sh["rays"] == w * h + qr.N_INSIDE + 2 * qr.N_SCALED + qr.N_AXIS + 6
    for fam in ("camera", "inside", "scaled", "axis"):
        assert b.hit[b.family == fam].any(), fam
    # a miss record is the defined one; a hit has t > 0 and a material
    assert np.array_equal(b.ref[~b.hit].view(np.uint32), np.tile(qr.MISS, ((~b.hit).sum(), 1)).view(np.uint32))
    assert (b.ref[b.hit][:, 3] > 0).all() and (b.ref[b.hit][:, 7:8].copy().view(np.int32) >= 0).all()
    # the occlusion batch: finite tmax rays come in fours, two on each side of the hit
    fin = np.isfinite(b.occ_rays[:, 3])
    assert fin.sum() % 4 == 0 and b.occ[fin].sum() * 2 == fin.sum() and not b.occ[~fin].any()


def test_vertex_normals_change_only_normals(packed):
    flat, smooth = qr.batch("CornellBox-Sphere", packed), qr.batch("CornellBox-Sphere", packed, True)
    assert np.array_equal(flat.rays.view(np.uint32), smooth.rays.view(np.uint32))
    assert np.array_equal(flat.ref[:, :4].view(np.uint32), smooth.ref[:, :4].view(np.uint32))
    assert not np.array_equal(flat.ref[:, 4:7].view(np.uint32), smooth.ref[:, 4:7].view(np.uint32))
    assert np.array_equal(flat.occ, smooth.occ)


# ---------------------------------------------------------------------------------------------
# the hand-out arithmetic, in a stand-alone program under the address and undefined-behaviour sanitizers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler (g++ or clang++): the hand-out arithmetic has no other check, so this is a failure, not a skip"
    exe = str(tmp_path_factory.mktemp("query_plan") / "query_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "scripts", "query_plan_harness.cpp"),
                    "-o", exe], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("refill", [0, 1])
@pytest.mark.parametrize("waves", [1, 4, 7, 1024])
def test_hand_out_model(harness, waves, refill):
    """Lanes finish in a seeded random order: every ray handed out once, every slot written once, the
    loop over within n + windows + 2 iterations (the program checks all three and says ok)."""
    for n in (0, 1, 63, 64, 65, 127, 4099):
        for seed in (1, 20261020):
            r = subprocess.run([harness, str(n), str(waves), str(refill), str(seed)], capture_output=True, text=True,
                               timeout=120)
            assert r.returncode == 0 and r.stdout.startswith(f"ok n={n} waves={waves} refill={refill} "), r.stdout + r.stderr
            m = re.search(r"windows=(\d+) max_iters=(\d+)", r.stdout)
            assert int(m.group(1)) == -(-n // 64) and int(m.group(2)) <= n + int(m.group(1)) + 2
