"""Rectangle-list renders (pt_render_rects, pt_render_rects_async, pt_selftest_rect_plan), the checks
that need no GPU: the planner's prefix sums, every rejection with its message, the list's size
limit, the header and the ABI version — through the library, and again in a stand-alone program
(scripts/rect_plan_harness.cpp, which links csrc/pt_rect_plan.cpp alone) built with
-fsanitize=address,undefined."""
import ctypes
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import pt_amd
from conftest import PKG

ROOT = os.path.dirname(PKG)
RECT_FNS = ("pt_render_rects", "pt_render_rects_async", "pt_selftest_rect_plan")
W, H = 40, 24
A, B = (5, 3, 19, 7), (13, 9, 17, 11)
L1 = [(39, 23, 1, 1), A, (13, 10, 17, 10), (0, 0, 3, 2)]

# (W, H, frame, rects, first slots)
ACCEPTED = [
    (W, H, None, L1, [0, 1, 134, 304]),
    (W, H, None, L1[::-1], [0, 6, 176, 309]),
    (W, H, None, [B], [0]),
    (W, H, None, [(0, 0, W, H)], [0]),
    (W, H, (4, 2, 30, 20), [A, (13, 10, 17, 10)], [0, 133]),
    # sharing an edge is no overlap: side by side, one above the other, and corner to corner
    (W, H, None, [(0, 0, 4, 4), (4, 0, 4, 4), (0, 4, 4, 4), (4, 4, 1, 1)], [0, 16, 32, 48]),
    (W, H, None, [(10, 10, 5, 5), (15, 15, 5, 5), (15, 5, 5, 5), (5, 15, 5, 5)], [0, 25, 50, 75]),
    (32768, 32768, None, [(32767, 32767, 1, 1), (0, 0, 32768, 32767)], [0, 1]),
]
# (W, H, frame, rects, what the message must say)
REJECTED = [
    (W, H, None, [], ["empty"]),
    (W, H, None, [A, (7, 7, 0, 3)], ["rects[1]", "(7, 7, 0, 3)", "at least 1"]),
    (W, H, None, [(7, 7, 3, 0)], ["rects[0]", "at least 1"]),
    (W, H, None, [A, (30, 20, 11, 2)], ["rects[1]", "(30, 20, 11, 2)", "outside"]),
    (W, H, None, [(0, 23, 2, 2)], ["rects[0]", "outside"]),
    (W, H, None, [(0xFFFFFFFF, 0, 2, 1)], ["rects[0]", "outside"]),
    (W, H, (4, 2, 30, 20), [A, (3, 3, 2, 2)], ["rects[1]", "outside the frame (4, 2, 30, 20)"]),
    (W, H, (4, 2, 30, 20), [(33, 21, 2, 1)], ["rects[0]", "outside the frame"]),
    (W, H, (4, 2, 40, 20), [A], ["frame (4, 2, 40, 20)", "image"]),
    (W, H, None, [A, B], ["rects[0]", "rects[1]", "overlap"]),  # they share row 9
    (W, H, None, [(0, 0, 3, 2), (30, 1, 2, 2), A, (23, 9, 4, 4)], ["rects[2]", "rects[3]", "overlap"]),  # one pixel: (23, 9)
    (W, H, None, [(2, 2, 10, 10), (4, 4, 2, 2)], ["rects[0]", "rects[1]", "overlap"]),  # one inside the other
    (W, H, None, [A, (20, 20, 1, 1), A], ["rects[0]", "rects[2]", "overlap"]),  # twice the same
    (W, H, None, [(0, 5, 40, 1), (7, 0, 1, 24)], ["rects[0]", "rects[1]", "overlap"]),  # a cross
]


def test_library_exports_the_rect_functions():
    lib = ctypes.CDLL(pt_amd.lib_path())
    assert [f for f in RECT_FNS if not hasattr(lib, f)] == []
    header = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    for f in RECT_FNS:
        assert f + "(" in header
    assert re.search(r"#define\s+PT_ABI_VERSION\s+3\b", header)
    assert pt_amd.abi_version() == 3 == pt_amd.ABI_VERSION


@pytest.mark.parametrize("case", ACCEPTED, ids=[str(k) for k in range(len(ACCEPTED))])
def test_prefix_sums(case):
    w, h, frame, rects, want = case
    first, npix = pt_amd.rect_plan(rects, w, h, frame=frame)
    assert first.dtype == np.uint64 and first.tolist() == want
    assert npix == sum(r[2] * r[3] for r in rects)


def test_l1_is_the_list_the_gpu_tests_describe():
    first, npix = pt_amd.rect_plan(L1, W, H)
    assert npix == 310 and first.tolist() == [0, 1, 134, 304]
    assert all(f % 64 for f in first.tolist()[1:])  # every border inside a 64-path batch


@pytest.mark.parametrize("case", REJECTED, ids=[str(k) for k in range(len(REJECTED))])
def test_rejections_name_the_rectangles(case):
    w, h, frame, rects, words = case
    with pytest.raises(pt_amd.PtError) as e:
        pt_amd.rect_plan(rects, w, h, frame=frame)
    assert e.value.code == -1
    for word in words:
        assert word in str(e.value), str(e.value)


def _ones(n):
    """n disjoint 1 x 1 rectangles of a 256-wide image, in no raster order"""
    k = np.arange(n)
    return np.stack([(k * 97) % 256, k // 256, np.ones(n, np.int64), np.ones(n, np.int64)], axis=1)


def test_the_size_limit():
    """65,536 rectangles are planned (an O(n^2) overlap check would take minutes, the sweep
    milliseconds), 65,537 are one too many.  The ctypes conversion is kept out of the time."""
    lib = pt_amd.load_library()
    for n, ok in ((65536, True), (65537, False)):
        arr = np.ascontiguousarray(_ones(n), np.uint32)
        first = np.zeros(n, np.uint64)
        npix = ctypes.c_uint64(0)
        t0 = time.perf_counter()
        rc = lib.pt_selftest_rect_plan(None, 256, 32768, arr.ctypes.data_as(ctypes.POINTER(pt_amd.Window)), n,
                                       first.ctypes.data_as(ctypes.c_void_p), ctypes.byref(npix))
        dt = time.perf_counter() - t0
        if ok:
            assert rc == 0 and npix.value == n and np.array_equal(first, np.arange(n, dtype=np.uint64))
            assert dt < 0.5, dt
        else:
            assert rc == -1 and b"65537" in lib.pt_last_error() and b"65536" in lib.pt_last_error()
    # ... and an overlap hidden among 65,536 is still found
    arr = np.ascontiguousarray(_ones(65536), np.uint32)
    arr[40000] = arr[123]
    rc = lib.pt_selftest_rect_plan(None, 256, 32768, arr.ctypes.data_as(ctypes.POINTER(pt_amd.Window)), 65536, None, None)
    assert rc == -1 and b"rects[123]" in lib.pt_last_error() and b"rects[40000]" in lib.pt_last_error()


def test_null_arguments_are_invalid():
    lib = pt_amd.load_library()
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    buf = np.zeros(8 * 8 * 3, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    r = pt_amd.Window(0, 0, 2, 2)
    assert lib.pt_render_rects(None, p(meta), None, ctypes.byref(r), 1, 0, 1, 1, 8, 0, p(buf), None, None) == -1
    assert b"null" in lib.pt_last_error()
    assert lib.pt_render_rects_async(None, p(meta), None, ctypes.byref(r), 1, 0, 1, 1, 8, 0, p(buf), None, 8, None, None) == -1
    assert b"null" in lib.pt_last_error()
    assert lib.pt_selftest_rect_plan(None, 8, 8, None, 1, None, None) == -1
    assert b"NULL" in lib.pt_last_error()


class _NoDevice:
    _lib = None
    _h = None


BAD_LISTS = [7, [(1, 2, 3)], [(0, 0, 1, 1), (1, 2)], [(0, 0, -1, 1)], [(0.5, 0, 1, 1)], [(0, 0, 1, 1 << 32)], [("0", 0, 1, 1)],
             [3]]


@pytest.mark.parametrize("rects", BAD_LISTS, ids=[repr(r) for r in BAD_LISTS])
def test_malformed_lists_are_rejected_on_the_host(rects):
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    s = _NoDevice()
    s._lib = pt_amd.load_library()
    for call in (lambda: pt_amd.Scene.render_rects(s, meta, rects, 0, 1),
                 lambda: pt_amd.Scene.render_rects_async(s, meta, rects, 0, 1, 1, 8, 0, 0),
                 lambda: pt_amd.rect_plan(rects, 8, 8)):
        with pytest.raises(pt_amd.PtError) as e:
            call()
        assert e.value.code == -1 and "rects" in str(e.value)


# ---------------------------------------------------------------------------------------------
# the stand-alone program, under the address and undefined-behaviour sanitizers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("rect_plan")
    exe = str(d / "rect_plan_harness")
    csrc = os.path.join(PKG, "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-I", csrc, os.path.join(ROOT, "scripts", "rect_plan_harness.cpp"),
                    os.path.join(csrc, "pt_rect_plan.cpp"), "-o", exe], check=True, capture_output=True)
    return exe, d


def _line(case):
    w, h, frame, rects = case[:4]
    f = frame or (0, 0, 0, 0)
    return " ".join(str(v) for v in (w, h, *f, len(rects), *[c for r in rects for c in r]))


def test_harness_agrees_on_every_case(harness):
    exe, d = harness
    path = str(d / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(_line(c) for c in ACCEPTED + REJECTED) + "\n")
    r = subprocess.run([exe, "cases", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(ACCEPTED) + len(REJECTED)
    for (w, h, frame, rects, want), line in zip(ACCEPTED, out):
        assert line.split() == ["ok", str(sum(x[2] * x[3] for x in rects)), *map(str, want)], line
    for (w, h, frame, rects, words), line in zip(REJECTED, out[len(ACCEPTED):]):
        assert line.startswith("invalid "), line
        with pytest.raises(pt_amd.PtError) as e:
            pt_amd.rect_plan(rects, w, h, frame=frame)
        assert line[len("invalid "):] in str(e.value)  # the library's message, word for word
        for word in words:
            assert word in line, line


def test_harness_random_lists(harness):
    exe, _ = harness
    r = subprocess.run([exe, "random", "20261019", "4000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"lists 4000 accepted (\d+) rejected (\d+) mismatches 0", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 1000, r.stdout


def test_harness_size_limit(harness):
    exe, _ = harness
    ok = subprocess.run([exe, "ones", "65536"], capture_output=True, text=True, timeout=120)
    assert ok.returncode == 0 and ok.stdout.startswith("ok 65536\n"), ok.stdout + ok.stderr
    bad = subprocess.run([exe, "ones", "65537"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 0 and bad.stdout.startswith("invalid ") and "65537" in bad.stdout, bad.stdout + bad.stderr
