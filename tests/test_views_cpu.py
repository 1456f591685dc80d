"""View-list renders (pt_render_views, pt_render_views_async, pt_selftest_view_plan), the checks that need
no GPU: the planner's prefix sums on the shared view sets, every refusal with the offending view named, the
list's size limit, pt_amd.view_atlas, the light the shared sets carry (the oracle alone) — through the
library, and the planner again in a stand-alone program (scripts/view_plan_harness.cpp, which links
csrc/pt_view_plan.cpp and csrc/pt_rect_plan.cpp and nothing else) built with -fsanitize=address,undefined."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cam_cases as cc
import oracle
import pt_amd
import radiance_ref as rr
import views_ref as vr
from conftest import PKG

ROOT = os.path.dirname(PKG)
VIEW_FNS = ("pt_render_views", "pt_render_views_async", "pt_selftest_view_plan")
F = np.float32
NAN, INF = float("nan"), float("inf")


def meta_wh(W, H, rr_prob=0.9, direct=0.0):
    m = np.zeros(48, F)
    m[0], m[1], m[45], m[46] = W, H, rr_prob, direct
    return m


def view(W=8, H=8, window=None, camera=None, dst=(0, 0), frame0=0, **kw):
    return {"meta": meta_wh(W, H, **kw), "window": window, "camera": camera, "dst": dst, "frame0": frame0}


A, B = view(dst=(0, 0)), view(dst=(8, 0))
# (atlas, views, what the message must say): every refusal of pt_render_views that the planner makes
REJECTED = [
    ((16, 8), [], ["empty"]),
    ((16, 8), [A, view(window=(2, 2, 0, 3), dst=(8, 0))], ["views[1]", "(2, 2, 0, 3)", "at least 1"]),
    ((16, 8), [view(window=(2, 2, 3, 0))], ["views[0]", "at least 1"]),
    ((16, 8), [A, view(window=(6, 0, 3, 2), dst=(8, 0))], ["views[1]", "(6, 0, 3, 2)", "within its image (8 x 8)"]),
    ((16, 8), [view(window=(0, 7, 1, 2))], ["views[0]", "within its image"]),
    ((16, 8), [view(window=(0xFFFFFFFF, 0, 2, 1))], ["views[0]", "within its image"]),
    ((16, 8), [A, view(dst=(9, 0))], ["views[1]", "(9, 0, 8, 8)", "outside the atlas (16 x 8)"]),
    ((16, 8), [view(dst=(0, 1))], ["views[0]", "outside the atlas"]),
    ((16, 8), [view(dst=(0xFFFFFFFF, 0))], ["views[0]", "outside the atlas"]),
    ((16, 8), [A, view(dst=(7, 0))], ["views[0]", "views[1]", "overlap"]),  # they share a column
    ((24, 16), [A, view(dst=(16, 8)), view(window=(0, 0, 1, 1), dst=(7, 7))], ["views[0]", "views[2]", "overlap"]),  # one pixel
    ((16, 8), [A, B, A], ["views[0]", "views[2]", "overlap"]),  # twice the same
    ((16, 8), [A, view(frame0=1 << 24, dst=(8, 0))], ["views[1]", "2^24"]),
    ((16, 8), [A, view(camera=(4, 0.1, 1.0), dst=(8, 0))], ["views[1]", "camera", "unknown model"]),
    ((16, 8), [view(camera=("thin_lens", -0.1, 1.0))], ["views[0]", "camera", "lens_radius"]),
    ((16, 8), [view(camera=("thin_lens", NAN, 1.0))], ["views[0]", "camera", "lens_radius"]),
    ((16, 8), [view(camera=("thin_lens", 0.1, 0.0))], ["views[0]", "camera", "focus_distance"]),
    ((16, 8), [view(camera=("ortho", 0.0, INF))], ["views[0]", "camera", "focus_distance"]),
    ((16, 8), [A, view(dst=(8, 0), rr_prob=np.nextafter(F(0.9), F(1)))], ["views[1]", "meta[45]", "views[0]"]),
    ((16, 8), [view(rr_prob=0.0), view(dst=(8, 0), rr_prob=-0.0)], ["views[1]", "meta[45]"]),  # bitwise
    ((16, 8), [A, view(dst=(8, 0), direct=1e-30)], ["views[1]", "meta[46]", "views[0]"]),
    ((16, 8), [view(W=8.5)], ["views[0]", "meta[0..1]"]),
    ((16, 8), [A, view(W=40000, window=(0, 0, 8, 8), dst=(8, 0))], ["views[1]", "meta[0..1]"]),
    ((0, 8), [A], ["atlas", "[1, 32768]"]),
    ((16, 40000), [A], ["atlas", "[1, 32768]"]),
]
ACCEPTED = [
    # destinations that touch but do not overlap: side by side, one above the other, corner to corner
    ((16, 16), [view(dst=(0, 0)), view(dst=(8, 0)), view(dst=(0, 8)), view(window=(1, 1, 1, 1), dst=(8, 8))], [0, 64, 128, 192]),
    ((32768, 32768), [view(W=32768, H=32768, window=(0, 0, 32768, 32767), dst=(0, 1)), view(window=(7, 7, 1, 1), dst=(32767, 0))],
     [0, 32768 * 32767]),
    ((16, 8), [view(frame0=(1 << 24) - 1), view(dst=(8, 0), camera=("thin_lens", 0.0, 1.0))], [0, 64]),
    ((16, 8), [view(direct=0.0), view(dst=(8, 0), direct=-3.0)], [0, 64]),  # the flag is meta[46] > 0
]


def test_library_exports_the_view_functions():
    lib = ctypes.CDLL(pt_amd.lib_path())
    assert [f for f in VIEW_FNS if not hasattr(lib, f)] == []
    header = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    for f in VIEW_FNS:
        assert f + "(" in header
    assert re.search(r"#define\s+PT_ABI_VERSION\s+3\b", header)  # additions keep the version
    assert ctypes.sizeof(pt_amd.View) == 240
    for name in ("pt_capi_views.hip", "pt_view_plan.cpp", "pt_view_plan.h"):
        assert name in pt_amd._lib._BUILD_SRCS
    with open(pt_amd.lib_path(), "rb") as f:
        data = f.read()
    for kernel in (b"k_wf_generate_views", b"k_wf_accum_views"):
        assert kernel in data, kernel


@pytest.mark.parametrize("name", list(vr.SETS))
def test_plan_of_the_shared_sets(name):
    scene, views, atlas = vr.views_of(name)
    first, npix = pt_amd.view_plan(views, atlas)
    areas = [v["window"][2] * v["window"][3] for v in views]
    assert first.dtype == np.uint64 and first.tolist() == np.concatenate([[0], np.cumsum(areas)[:-1]]).tolist()
    assert npix == sum(areas)
    inside = np.zeros((atlas[1], atlas[0]), np.int32)
    for v in views:
        (x, y), (_, _, w, h) = v["dst"], v["window"]
        inside[y:y + h, x:x + w] += 1
    assert inside.max() == 1 and inside.sum() == npix


def test_mixed5_is_the_list_the_gpu_tests_describe():
    scene, views, atlas = vr.views_of("mixed5")
    first, npix = pt_amd.view_plan(views, atlas)
    assert atlas == (96, 64) and npix == vr.MIXED5_NPIX and first.tolist() == vr.MIXED5_FIRST
    assert all(f % 64 for f in first.tolist()[1:])  # every border inside a 64-path batch, so inside a wave
    assert [v["window"][2] * v["window"][3] for v in views] == [891, 384, 1, 143, 1209]
    assert [v["frame0"] for v in views] == [2, 0, 7, 2, 1000]
    order = [v["dst"][1] * atlas[0] + v["dst"][0] for v in views]
    assert order != sorted(order)  # not listed in atlas order
    assert len({(float(v["meta"][0]), float(v["meta"][1])) for v in views}) == 2  # two image sizes
    assert not inside_touching(views)  # gaps between the destinations


def inside_touching(views):
    """Any two destinations closer than one pixel of gap."""
    for a in range(len(views)):
        for b in range(a + 1, len(views)):
            (ax, ay), (_, _, aw, ah) = views[a]["dst"], views[a]["window"]
            (bx, by), (_, _, bw, bh) = views[b]["dst"], views[b]["window"]
            if ax <= bx + bw and bx <= ax + aw and ay <= by + bh and by <= ay + ah:
                return True
    return False


@pytest.mark.parametrize("case", ACCEPTED, ids=[str(k) for k in range(len(ACCEPTED))])
def test_accepted(case):
    atlas, views, want = case
    first, npix = pt_amd.view_plan(views, atlas)
    assert first.tolist() == want
    assert npix == want[-1] + (views[-1]["window"] or (0, 0, 8, 8))[2] * (views[-1]["window"] or (0, 0, 8, 8))[3]


@pytest.mark.parametrize("case", REJECTED, ids=[str(k) for k in range(len(REJECTED))])
def test_refusals_name_the_views(case):
    atlas, views, words = case
    with pytest.raises(pt_amd.PtError) as e:
        if atlas[0] < 1:  # the binding refuses an atlas of no width itself
            arr, n, _ = pt_amd._lib._views(views, (1, atlas[1]))
            pt_amd._lib._check(pt_amd.load_library().pt_selftest_view_plan(arr, n, atlas[0], atlas[1], None, None))
        else:
            pt_amd.view_plan(views, atlas)
    assert e.value.code == -1
    for word in words:
        assert word in str(e.value), str(e.value)


def _raw(n, mutate=None):
    """n views of 1 x 1 (8 x 8 images) at disjoint places of a 256-wide atlas, in no raster order."""
    arr = (pt_amd.View * n)()
    a = np.frombuffer(arr, np.uint32).reshape(n, 60)
    k = np.arange(n)
    a[:, 0] = a[:, 1] = np.array([8.0], F).view(np.uint32)[0]
    a[:, 45] = np.array([0.9], F).view(np.uint32)[0]
    a[:, 48], a[:, 49], a[:, 50], a[:, 51] = k % 8, k // 8 % 8, 1, 1
    a[:, 56], a[:, 57] = (k * 97) % 256, k // 256
    if mutate:
        mutate(a)
    return arr


def test_the_size_limit_reserved_and_npix():
    lib = pt_amd.load_library()
    for n, ok in ((65536, True), (65537, False)):
        arr = _raw(n)
        first = np.zeros(n, np.uint64)
        npix = ctypes.c_uint64(0)
        rc = lib.pt_selftest_view_plan(arr, n, 256, 32768, first.ctypes.data_as(ctypes.c_void_p), ctypes.byref(npix))
        if ok:
            assert rc == 0 and npix.value == n and np.array_equal(first, np.arange(n, dtype=np.uint64))
        else:
            assert rc == -1 and b"65537" in lib.pt_last_error() and b"65536" in lib.pt_last_error()
    # an overlap hidden among 65,536 is still found, and named
    def clash(a):
        a[40000, 56:58] = a[123, 56:58]
    assert lib.pt_selftest_view_plan(_raw(65536, clash), 65536, 256, 32768, None, None) == -1
    assert b"views[123]" in lib.pt_last_error() and b"views[40000]" in lib.pt_last_error()
    # reserved != 0

    def reserved(a):
        a[2, 59] = 1
    assert lib.pt_selftest_view_plan(_raw(4, reserved), 4, 256, 32768, None, None) == -1
    assert b"views[2]" in lib.pt_last_error() and b"reserved" in lib.pt_last_error()
    # npix >= 2^31: the third window of 32768 x 32767 (disjointness is never reached)

    def huge(a):
        a[:, 0] = a[:, 1] = np.array([32768.0], F).view(np.uint32)[0]
        a[:, 48], a[:, 49], a[:, 50], a[:, 51] = 0, 0, 32768, 32767
        a[:, 56], a[:, 57] = 0, 0
    assert lib.pt_selftest_view_plan(_raw(3, huge), 3, 32768, 32768, None, None) == -1
    assert b"2^31" in lib.pt_last_error() and b"views[2]" in lib.pt_last_error()
    # NULL
    assert lib.pt_selftest_view_plan(None, 1, 8, 8, None, None) == -1 and b"NULL" in lib.pt_last_error()
    assert lib.pt_render_views(None, _raw(1), 1, 8, 8, 1, 1, 8, 0, None, None) == -1 and b"null" in lib.pt_last_error()
    assert lib.pt_render_views_async(None, _raw(1), 1, 8, 8, 1, 1, 8, 0, None, 8, None, None) == -1
    assert b"null" in lib.pt_last_error()


def test_view_atlas_places_rectangles_disjointly_inside_its_atlas():
    rng = np.random.default_rng(20261021)
    for trial in range(40):
        n = int(rng.integers(1, 40))
        sizes = [(int(rng.integers(1, 50)), int(rng.integers(1, 50))) for _ in range(n)]
        cols = None if trial % 2 else int(rng.integers(1, n + 1))
        dsts, (aw, ah) = pt_amd.view_atlas(sizes, cols)
        cover = np.zeros((ah, aw), np.int32)
        for (x, y), (w, h) in zip(dsts, sizes):
            assert 0 <= x and x + w <= aw and 0 <= y and y + h <= ah
            cover[y:y + h, x:x + w] += 1
        assert cover.max() == 1
        views = [view(W=w, H=h, dst=d) for d, (w, h) in zip(dsts, sizes)]
        assert pt_amd.view_plan(views, (aw, ah))[1] == sum(w * h for w, h in sizes)  # the planner agrees
    assert pt_amd.view_atlas([(4, 3)] * 6, 3) == ([(0, 0), (4, 0), (8, 0), (0, 3), (4, 3), (8, 3)], (12, 6))
    # a list without dst is packed by it
    assert pt_amd.view_plan([{"meta": meta_wh(4, 3)}] * 6)[0].tolist() == [0, 12, 24, 36, 48, 60]
    with pytest.raises(pt_amd.PtError):
        pt_amd.view_plan([{"meta": meta_wh(4, 3), "dst": (0, 0)}, {"meta": meta_wh(4, 3)}], (8, 3))


BAD_LISTS = [7, [3], [{"window": (0, 0, 1, 1)}], [{"meta": np.zeros(47, F)}], [{"meta": meta_wh(8, 8), "windov": 1}],
             [{"meta": meta_wh(8, 8), "window": (0, 0, -1, 1)}], [{"meta": meta_wh(8, 8), "frame0": 0.5}],
             [{"meta": meta_wh(8, 8), "dst": (1, 2, 3)}]]


@pytest.mark.parametrize("views", BAD_LISTS, ids=[str(k) for k in range(len(BAD_LISTS))])
def test_malformed_lists_are_rejected_on_the_host(views):
    with pytest.raises(pt_amd.PtError) as e:
        pt_amd.view_plan(views, (8, 8))
    assert e.value.code == -1


# ---------------------------------------------------------------------------------------------
# the light the shared sets carry, and the pinhole path of views_ref, on the oracle alone
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("radiance_ref"))


@pytest.mark.parametrize("name", list(vr.SETS))
def test_every_view_carries_light(packed, ref, name):
    scene, views, atlas = vr.views_of(name)
    _, cnt, tiles = vr.reference(ref, packed, name)
    shares = [float((t.sum(axis=2) > 0).mean()) for t in tiles]
    print(name, "lit shares:", " ".join(f"{s:.3f}" for s in shares))
    assert min(shares) >= 0.25, shares
    assert cnt["samples"] == vr.NFRAMES * sum(v["window"][2] * v["window"][3] for v in views)


def test_the_pinhole_reference_is_the_oracles_render(packed, ref):
    """views_ref's pinhole tiles against oracle.render: the whole 24 x 16 view of mixed5, and the rows of
    its 39 x 31 window cropped from a full render."""
    scene, views, atlas = vr.views_of("mixed5")
    tiles = vr.reference(ref, packed, "mixed5")[2]
    p = packed[scene]
    for k in (1, 4):
        v = views[k]
        x0, y0, w, h = v["window"]
        want, _ = oracle.render(p.triangle_data, p.bvh_data, v["meta"], v["frame0"], vr.NFRAMES, 1, vr.DEPTH, y0=y0, y1=y0 + h)
        assert tiles[k].tobytes() == np.ascontiguousarray(want[:, x0:x0 + w]).tobytes(), k
    twins = vr.reference(ref, packed, "twins")[2]
    assert twins[0].tobytes() != twins[1].tobytes()


# ---------------------------------------------------------------------------------------------
# the stand-alone program, under the address and undefined-behaviour sanitizers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("view_plan")
    exe = str(d / "view_plan_harness")
    csrc = os.path.join(PKG, "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-I", csrc, os.path.join(ROOT, "scripts", "view_plan_harness.cpp"), os.path.join(csrc, "pt_view_plan.cpp"),
                    os.path.join(csrc, "pt_rect_plan.cpp"), "-o", exe], check=True, capture_output=True)
    return exe, d


def _line(atlas, views):
    arr, n, _ = pt_amd._lib._views(views, (max(1, atlas[0]), atlas[1]))
    out = [atlas[0], atlas[1], n]
    for k in range(n):
        v = arr[k]
        out += [repr(float(v.meta[0])), repr(float(v.meta[1])), v.win.x0, v.win.y0, v.win.w, v.win.h, v.cam.model,
                repr(float(v.cam.lens_radius)), repr(float(v.cam.focus_distance)), v.dst_x, v.dst_y, v.frame0, v.reserved,
                int(np.array([v.meta[45]], F).view(np.uint32)[0]), repr(float(v.meta[46]))]
    return " ".join(str(t) for t in out)


def test_harness_agrees_on_every_case(harness):
    exe, d = harness
    sets = [vr.views_of(name) for name in vr.SETS]
    cases = [(atlas, views) for _, views, atlas in sets] + [(a, v) for a, v, _ in ACCEPTED] + [(a, v) for a, v, _ in REJECTED]
    path = str(d / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(_line(a, v) for a, v in cases) + "\n")
    r = subprocess.run([exe, "cases", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    nok = len(sets) + len(ACCEPTED)
    for (atlas, views), line in zip(cases[:nok], out):
        first, npix = pt_amd.view_plan(views, atlas)
        assert line.split() == ["ok", str(npix), *map(str, first.tolist())], line
    for (atlas, views, words), line in zip(REJECTED, out[nok:]):
        assert line.startswith("invalid "), line
        for word in words:
            assert word in line, line
        if atlas[0] >= 1:
            with pytest.raises(pt_amd.PtError) as e:
                pt_amd.view_plan(views, atlas)
            assert line[len("invalid "):] in str(e.value)  # the library's message, word for word


def test_harness_random_lists(harness):
    exe, _ = harness
    r = subprocess.run([exe, "random", "20261021", "3000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"lists 3000 accepted (\d+) rejected (\d+) mismatches 0", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 1000, r.stdout


def test_harness_size_limit(harness):
    exe, _ = harness
    ok = subprocess.run([exe, "ones", "65536"], capture_output=True, text=True, timeout=120)
    assert ok.returncode == 0 and ok.stdout.startswith("ok 65536\n"), ok.stdout + ok.stderr
    bad = subprocess.run([exe, "ones", "65537"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 0 and bad.stdout.startswith("invalid ") and "65537" in bad.stdout, bad.stdout + bad.stderr
