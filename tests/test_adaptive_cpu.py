"""Second moments, tile noise and the adaptive driver: the checks that need no GPU.  The symbols and
structs match the header, null arguments and malformed parameters are rejected before any device
call, and pt_selftest_tile_rects merges masks of active tiles as documented."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as ar
import pt_amd
from conftest import PKG

NEW_FNS = ("pt_render_moments", "pt_render_moments_async", "pt_noise_tiles_async", "pt_noise_tiles", "pt_tile_mean_async",
           "pt_render_adaptive", "pt_selftest_tile_rects")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---------------------------------------------------------------------------------------------
# 10. symbols and header
# ---------------------------------------------------------------------------------------------
def test_library_exports_the_new_functions():
    lib = ctypes.CDLL(pt_amd.lib_path())
    assert [f for f in NEW_FNS if not hasattr(lib, f)] == []
    header = open(os.path.join(os.path.dirname(PKG), "include", "pt_hip.h")).read()
    for f in NEW_FNS:
        assert f + "(" in header
    assert "} pt_tile_noise;" in header and "} pt_adaptive;" in header
    assert "#define PT_ABI_VERSION 3" in header


def test_abi_version_unchanged():
    assert pt_amd.abi_version() == 3 == pt_amd.ABI_VERSION


def test_structs_match_the_header():
    assert ctypes.sizeof(pt_amd.TileNoise) == 16 == pt_amd.TILE_NOISE_DTYPE.itemsize
    assert (pt_amd.TileNoise.noisy.offset, pt_amd.TileNoise.pixels.offset, pt_amd.TileNoise.max_err.offset) == (0, 4, 8)
    assert [pt_amd.TILE_NOISE_DTYPE.fields[n][1] for n in ("noisy", "pixels", "max_err")] == [0, 4, 8]
    A = pt_amd.Adaptive
    assert ctypes.sizeof(A) == 48
    assert [getattr(A, n).offset for n, _ in A._fields_] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert [n for n, _ in A._fields_] == ["tile_w", "tile_h", "min_frames", "step_frames", "max_frames", "tol", "floor",
                                          "noisy_fraction"]
    a = A(8, 4, 2, 3, 9, 0.5, 0.25, 0.125)
    assert (a.tile_w, a.tile_h, a.min_frames, a.step_frames, a.max_frames, a.tol, a.floor, a.noisy_fraction) == \
        (8, 4, 2, 3, 9, 0.5, 0.25, 0.125)


# ---------------------------------------------------------------------------------------------
# 11. null arguments
# ---------------------------------------------------------------------------------------------
def test_null_scene_is_invalid():
    lib = pt_amd.load_library()
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    buf, sq = np.zeros(8 * 8 * 3, np.float32), np.zeros(8 * 8 * 3, np.float32)
    fr, out = np.full(4, 4, np.uint32), np.zeros(4, pt_amd.TILE_NOISE_DTYPE)
    ad = pt_amd.Adaptive(4, 4, 2, 1, 4, 0.5, 0.05, 0.05)
    assert lib.pt_render_moments(None, _p(meta), None, 0, 1, 1, 8, 0, _p(buf), _p(sq), None) == -1
    assert b"null" in lib.pt_last_error()
    assert lib.pt_render_moments_async(None, _p(meta), None, 0, 1, 1, 8, 0, _p(buf), _p(sq), 8, None, None) == -1
    assert lib.pt_noise_tiles(None, _p(buf), _p(sq), 8, 8, 4, 4, _p(fr), 0.5, 0.05, _p(out)) == -1
    assert lib.pt_noise_tiles_async(None, _p(buf), _p(sq), 8, 8, 8, 4, 4, _p(fr), 0.5, 0.05, _p(out), None) == -1
    assert lib.pt_tile_mean_async(None, _p(buf), 8, 8, 8, 4, 4, _p(fr), _p(sq), None) == -1
    assert lib.pt_render_adaptive(None, _p(meta), None, ctypes.byref(ad), 0, 8, 0, _p(buf), _p(sq), _p(fr), None, None,
                                  None, None) == -1
    assert b"null" in lib.pt_last_error()


def test_null_arguments_and_malformed_parameters_before_the_scene_is_looked_at():
    """With a scene argument that is not NULL (a zeroed buffer, in a child process, where a call that
    did look at it ends as a failed test): NULL meta, destination, m2, frames or pt_adaptive, and a
    malformed pt_adaptive or tile grid, answer PT_ERR_INVALID."""
    code = (
        "import ctypes, sys\n"
        "sys.path.insert(0, sys.argv[1])\n"
        "import numpy as np, pt_amd\n"
        "lib = pt_amd.load_library()\n"
        "meta = np.zeros(48, np.float32); meta[0] = meta[1] = 8\n"
        "buf = np.zeros(8 * 8 * 3, np.float32); sq = buf.copy(); fr = np.full(4, 4, np.uint32)\n"
        "out = np.zeros(4, pt_amd.TILE_NOISE_DTYPE)\n"
        "p = lambda a: a.ctypes.data_as(ctypes.c_void_p)\n"
        "scene = ctypes.create_string_buffer(1 << 16)\n"
        "sp = ctypes.cast(scene, ctypes.c_void_p)\n"
        "err = lambda: lib.pt_last_error().decode()\n"
        "for m, d, q in ((None, p(buf), p(sq)), (p(meta), None, p(sq)), (p(meta), p(buf), None)):\n"
        "    assert lib.pt_render_moments(sp, m, None, 0, 1, 1, 8, 0, d, q, None) == -1 and 'null' in err()\n"
        "    assert lib.pt_render_moments_async(sp, m, None, 0, 1, 1, 8, 0, d, q, 8, None, None) == -1 and 'null' in err()\n"
        "for a, q, f, o in ((None, p(sq), p(fr), p(out)), (p(buf), None, p(fr), p(out)), (p(buf), p(sq), None, p(out)),\n"
        "                   (p(buf), p(sq), p(fr), None)):\n"
        "    assert lib.pt_noise_tiles(sp, a, q, 8, 8, 4, 4, f, 0.5, 0.05, o) == -1 and 'null' in err()\n"
        "    assert lib.pt_noise_tiles_async(sp, a, q, 8, 8, 8, 4, 4, f, 0.5, 0.05, o, None) == -1 and 'null' in err()\n"
        "for a, f, o in ((None, p(fr), p(sq)), (p(buf), None, p(sq)), (p(buf), p(fr), None)):\n"
        "    assert lib.pt_tile_mean_async(sp, a, 8, 8, 8, 4, 4, f, o, None) == -1 and 'null' in err()\n"
        "ad = pt_amd.Adaptive(4, 4, 2, 1, 4, 0.5, 0.05, 0.05)\n"
        "adp = ctypes.byref(ad)\n"
        "for m, a, acc, f in ((None, adp, p(buf), p(fr)), (p(meta), None, p(buf), p(fr)), (p(meta), adp, None, p(fr)),\n"
        "                     (p(meta), adp, p(buf), None)):\n"
        "    assert lib.pt_render_adaptive(sp, m, None, a, 0, 8, 0, acc, p(sq), f, None, None, None, None) == -1\n"
        "    assert 'null' in err()\n"
        "inf, nan = float('inf'), float('nan')\n"
        "bad = [((0, 4, 2, 1, 4, 0.5, 0.05, 0.05), 'tile_w'), ((4, 0, 2, 1, 4, 0.5, 0.05, 0.05), 'tile_h'),\n"
        "       ((4, 4, 1, 1, 4, 0.5, 0.05, 0.05), 'min_frames'), ((4, 4, 2, 0, 4, 0.5, 0.05, 0.05), 'step_frames'),\n"
        "       ((4, 4, 5, 1, 4, 0.5, 0.05, 0.05), 'max_frames'), ((4, 4, 2, 1, 4, 0.0, 0.05, 0.05), 'tol'),\n"
        "       ((4, 4, 2, 1, 4, nan, 0.05, 0.05), 'tol'), ((4, 4, 2, 1, 4, inf, 0.05, 0.05), 'tol'),\n"
        "       ((4, 4, 2, 1, 4, 0.5, -1.0, 0.05), 'floor'), ((4, 4, 2, 1, 4, 0.5, nan, 0.05), 'floor'),\n"
        "       ((4, 4, 2, 1, 4, 0.5, 0.05, 1.0), 'noisy_fraction'), ((4, 4, 2, 1, 4, 0.5, 0.05, -0.1), 'noisy_fraction'),\n"
        "       ((4, 4, 2, 1, 4, 0.5, 0.05, nan), 'noisy_fraction')]\n"
        "for fields, name in bad:\n"
        "    a = pt_amd.Adaptive(*fields)\n"
        "    rc = lib.pt_render_adaptive(sp, p(meta), None, ctypes.byref(a), 0, 8, 0, p(buf), p(sq), p(fr), None, None, None, None)\n"
        "    assert rc == -1 and name in err(), (fields, err())\n"
        "rc = lib.pt_render_adaptive(sp, p(meta), None, adp, (1 << 24) - 3, 8, 0, p(buf), p(sq), p(fr), None, None, None, None)\n"
        "assert rc == -1 and '2^24' in err()\n"
        "for w, h, pitch, tw, th, tol, floor in ((0, 8, 8, 4, 4, .5, .05), (8, 0, 8, 4, 4, .5, .05), (8, 8, 7, 4, 4, .5, .05),\n"
        "                                        (8, 8, 8, 0, 4, .5, .05), (8, 8, 8, 4, 0, .5, .05), (8, 8, 8, 4, 4, 0., .05),\n"
        "                                        (8, 8, 8, 4, 4, .5, nan), (40000, 8, 40000, 4, 4, .5, .05)):\n"
        "    assert lib.pt_noise_tiles_async(sp, p(buf), p(sq), w, h, pitch, tw, th, p(fr), tol, floor, p(out), None) == -1\n"
        "    assert 'null' not in err()\n"
        "assert lib.pt_tile_mean_async(sp, p(buf), 8, 8, 7, 4, 4, p(fr), p(sq), None) == -1 and 'row_pitch' in err()\n"
    )
    r = subprocess.run([sys.executable, "-c", code, PKG], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------------------------
# 12. malformed parameters, on the host
# ---------------------------------------------------------------------------------------------
class _NoDevice:
    """A Scene without a device: a check that let the call through would reach the library with a
    NULL scene (PT_ERR_INVALID too, but with another message: the tests look at it)."""
    _lib = None
    _h = None


def _scene():
    s = _NoDevice()
    s._lib = pt_amd.load_library()
    return s


GOOD = dict(tile=(8, 8), min_frames=4, step_frames=4, max_frames=16, tol=0.5, floor=0.05, noisy_fraction=0.05)
BAD_ADAPTIVE = [
    ("tile", (8,)), ("tile", (8, 8, 8)), ("tile", 8), ("tile", (0, 8)), ("tile", (8, 0)), ("tile", (8.0, 8)),
    ("tile", (-1, 8)), ("tile", (True, 8)), ("tile", ("8", 8)), ("tile", (1 << 32, 8)),
    ("min_frames", 1), ("min_frames", 0), ("min_frames", -4), ("min_frames", 4.0), ("min_frames", "4"),
    ("min_frames", True), ("min_frames", None),
    ("step_frames", 0), ("step_frames", -1), ("step_frames", 1.5), ("step_frames", None),
    ("max_frames", 3), ("max_frames", 0), ("max_frames", 16.0), ("max_frames", 1 << 32),
    ("tol", 0), ("tol", -0.5), ("tol", float("nan")), ("tol", float("inf")), ("tol", "0.5"), ("tol", None), ("tol", True),
    ("floor", 0.0), ("floor", -1), ("floor", float("nan")), ("floor", float("-inf")), ("floor", [0.05]),
    ("noisy_fraction", 1.0), ("noisy_fraction", -0.01), ("noisy_fraction", float("nan")), ("noisy_fraction", 2),
    ("noisy_fraction", "0"), ("noisy_fraction", None),
]


@pytest.mark.parametrize("field,value", BAD_ADAPTIVE, ids=[f"{f}={v!r}" for f, v in BAD_ADAPTIVE])
def test_malformed_adaptive_parameters_are_rejected_on_the_host(field, value):
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    with pytest.raises(pt_amd.PtError) as e:
        pt_amd.Scene.render_adaptive(_scene(), meta, **{**GOOD, field: value})
    name = {"tile": "tile"}.get(field, field)
    assert e.value.code == -1 and name in str(e.value), str(e.value)


def test_frame_range_past_2_24_is_rejected_on_the_host():
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    for frame0 in ((1 << 24) - 15, 1 << 24, -1, 0.5):
        with pytest.raises(pt_amd.PtError) as e:
            pt_amd.Scene.render_adaptive(_scene(), meta, frame0=frame0, **GOOD)
        assert e.value.code == -1 and "frame0" in str(e.value)
    with pytest.raises(pt_amd.PtError) as e:  # the last frame 2^24 - 1 is allowed: the call reaches the (NULL) scene
        pt_amd.Scene.render_adaptive(_scene(), meta, frame0=(1 << 24) - 16, **GOOD)
    assert "null" in str(e.value)


@pytest.mark.parametrize("tile", [(8,), 8, (0, 8), (8, 0), (8.0, 8), (1, 2, 3), ("a", 1)], ids=repr)
def test_malformed_tiles_are_rejected_on_the_host(tile):
    s = _scene()
    acc = np.zeros((8, 8, 3), np.float32)
    for call in (lambda: pt_amd.Scene.noise_tiles(s, acc, acc, tile, np.ones(1, np.uint32), 0.5, 0.05),
                 lambda: pt_amd.Scene.noise_tiles_async(s, 1, 1, 8, 8, tile, 1, 0.5, 0.05, 1),
                 lambda: pt_amd.Scene.tile_mean_async(s, 1, 8, 8, tile, 1, 1)):
        with pytest.raises(pt_amd.PtError) as e:
            call()
        assert e.value.code == -1 and "tile" in str(e.value)


def test_malformed_noise_arguments_are_rejected_on_the_host():
    s = _scene()
    acc = np.zeros((8, 8, 3), np.float32)
    fr = np.full((2, 2), 4, np.uint32)
    for kw, name in ((dict(tol=0.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(floor=-1.0), "floor"),
                     (dict(floor="x"), "floor")):
        args = {"tol": 0.5, "floor": 0.05, **kw}
        with pytest.raises(pt_amd.PtError) as e:
            pt_amd.Scene.noise_tiles(s, acc, acc, (4, 4), fr, args["tol"], args["floor"])
        assert e.value.code == -1 and name in str(e.value)
    with pytest.raises(pt_amd.PtError) as e:  # one count per tile
        pt_amd.Scene.noise_tiles(s, acc, acc, (4, 4), np.ones(3, np.uint32), 0.5, 0.05)
    assert e.value.code == -1 and "frames" in str(e.value)
    with pytest.raises(pt_amd.PtError) as e:
        pt_amd.Scene.noise_tiles(s, acc, np.zeros((8, 4, 3), np.float32), (4, 4), fr, 0.5, 0.05)
    assert e.value.code == -1 and "m2" in str(e.value)
    with pytest.raises(pt_amd.PtError) as e:
        pt_amd.Scene.noise_tiles_async(s, 1, 1, 8, 8, (4, 4), 1, 0.5, 0.05, 1, row_pitch=-1)
    assert e.value.code == -1 and "row_pitch" in str(e.value)


# ---------------------------------------------------------------------------------------------
# 13. pt_selftest_tile_rects
# ---------------------------------------------------------------------------------------------
def check_rects(mask):
    mask = np.asarray(mask) != 0
    r = pt_amd.tile_rects(mask)
    cover = np.zeros(mask.shape, np.int32)
    for x, y, w, h in r.astype(int):
        assert w >= 1 and h >= 1 and x + w <= mask.shape[1] and y + h <= mask.shape[0]
        cover[y:y + h, x:x + w] += 1
    assert cover.max(initial=0) <= 1  # pairwise disjoint
    assert np.array_equal(cover == 1, mask)  # the union is the mask
    assert len(r) <= int(mask.sum())
    assert np.array_equal(pt_amd.tile_rects(mask), r)  # the same input, the same output
    assert np.array_equal(r, ar.tile_rects(mask))  # the documented order
    return r


@pytest.mark.parametrize("shape", [(3, 5), (7, 9)], ids=["5x3", "9x7"])
def test_tile_rects_random_masks(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for density in (0.2, 0.5, 0.8):
        for _ in range(20):
            check_rects(rng.random(shape) < density)


def test_tile_rects_special_masks():
    assert check_rects(np.ones((3, 5))).tolist() == [[0, 0, 5, 3]]
    assert check_rects(np.zeros((3, 5))).shape == (0, 4)
    board = np.indices((3, 5)).sum(0) % 2
    assert len(check_rects(board)) == int(board.sum())  # one per tile
    ell = np.array([[1, 0, 0], [1, 0, 0], [1, 1, 1]])
    assert check_rects(ell).tolist() == [[0, 0, 1, 2], [0, 2, 3, 1]]
    assert check_rects(np.ones((1, 1))).tolist() == [[0, 0, 1, 1]]


def test_tile_rects_golden():
    """Written out by hand: two runs in a row; a run that keeps its columns extends its rectangle; one
    that changes them closes it; a rectangle interrupted for a row does not reopen."""
    mask = np.array([[1, 1, 0, 1, 0],
                     [1, 1, 0, 1, 1],
                     [0, 1, 1, 0, 1],
                     [1, 1, 0, 0, 1],
                     [1, 1, 0, 0, 0],
                     [0, 0, 0, 0, 1]])
    want = [[0, 0, 2, 2], [3, 0, 1, 1], [3, 1, 2, 1], [1, 2, 2, 1], [4, 2, 1, 2], [0, 3, 2, 2], [4, 5, 1, 1]]
    assert check_rects(mask).tolist() == want


def test_tile_rects_small_cap_reports_the_count():
    lib = pt_amd.load_library()
    mask = np.ascontiguousarray(np.indices((3, 5)).sum(0) % 2, dtype=np.uint8)  # 7 rectangles
    n = ctypes.c_size_t(0)
    out = np.full((7, 4), 99, np.uint32)
    assert lib.pt_selftest_tile_rects(_p(mask), 5, 3, _p(out), 3, ctypes.byref(n)) == -1
    assert n.value == 7
    assert np.all(out[3:] == 99)  # nothing past cap
    assert lib.pt_selftest_tile_rects(_p(mask), 5, 3, None, 0, ctypes.byref(n)) == -1 and n.value == 7
    assert lib.pt_selftest_tile_rects(_p(mask), 5, 3, _p(out), 7, ctypes.byref(n)) == 0 and n.value == 7
    assert np.array_equal(out, ar.tile_rects(mask))
    assert lib.pt_selftest_tile_rects(None, 5, 3, _p(out), 7, ctypes.byref(n)) == -1
    assert lib.pt_selftest_tile_rects(_p(mask), 5, 3, _p(out), 7, None) == -1
    assert lib.pt_selftest_tile_rects(_p(mask), 0, 3, _p(out), 7, ctypes.byref(n)) == -1
