"""Window renders (pt_render_window, pt_render_window_async, pt_frame_window), the checks that need
no GPU: the symbols exist, null arguments and malformed windows are rejected before any device
call, the ABI version stays, and the CLI refuses a malformed --window."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pt_amd
from conftest import PKG, SCENES

WINDOW_FNS = ("pt_render_window", "pt_render_window_async", "pt_frame_window")
INI = os.path.join(SCENES, "scene_files", "final", "cornell_box_full_lighting.ini")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_library_exports_the_window_functions():
    lib = ctypes.CDLL(pt_amd.lib_path())
    assert [f for f in WINDOW_FNS if not hasattr(lib, f)] == []
    header = open(os.path.join(os.path.dirname(PKG), "include", "pt_hip.h")).read()
    for f in WINDOW_FNS:
        assert f + "(" in header
    assert "} pt_window;" in header


def test_abi_version_unchanged():
    assert pt_amd.abi_version() == 3 == pt_amd.ABI_VERSION


def test_window_struct_matches_header():
    assert ctypes.sizeof(pt_amd.Window) == 16
    w = pt_amd.Window(1, 2, 3, 4)
    assert (w.x0, w.y0, w.w, w.h) == (1, 2, 3, 4)


def test_null_scene_is_invalid():
    lib = pt_amd.load_library()
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    buf = np.zeros(8 * 8 * 3, np.float32)
    win = pt_amd.Window(0, 0, 2, 2)
    for m in (_p(meta), None):
        assert lib.pt_render_window(None, m, ctypes.byref(win), 0, 1, 1, 8, 0, _p(buf), None) == -1
        assert b"null" in lib.pt_last_error()
        assert lib.pt_render_window_async(None, m, ctypes.byref(win), 0, 1, 1, 8, 0, _p(buf), 2, None, None) == -1
        assert lib.pt_frame_window(None, m, ctypes.byref(win), 0, 8, _p(buf)) == -1
        assert lib.pt_render_window(None, m, None, 0, 1, 1, 8, 0, _p(buf), None) == -1


def test_null_meta_or_destination_is_invalid():
    """With a scene argument that is not NULL: the calls must answer PT_ERR_INVALID for a NULL meta
    or destination before they look at the scene.  No scene exists without a GPU, so a zeroed buffer
    stands in for one — in a child process, where a call that did look at it ends as a failed test."""
    code = (
        "import ctypes, sys\n"
        "sys.path.insert(0, sys.argv[1])\n"
        "import numpy as np, pt_amd\n"
        "lib = pt_amd.load_library()\n"
        "meta = np.zeros(48, np.float32); meta[0] = meta[1] = 8\n"
        "buf = np.zeros(8 * 8 * 3, np.float32)\n"
        "p = lambda a: a.ctypes.data_as(ctypes.c_void_p)\n"
        "win = ctypes.byref(pt_amd.Window(0, 0, 2, 2))\n"
        "scene = ctypes.create_string_buffer(1 << 16)\n"
        "sp = ctypes.cast(scene, ctypes.c_void_p)\n"
        "for m, d in ((None, p(buf)), (p(meta), None)):\n"
        "    assert lib.pt_render_window(sp, m, win, 0, 1, 1, 8, 0, d, None) == -1\n"
        "    assert lib.pt_render_window(sp, m, None, 0, 1, 1, 8, 0, d, None) == -1\n"
        "    assert lib.pt_render_window_async(sp, m, win, 0, 1, 1, 8, 0, d, 2, None, None) == -1\n"
        "    assert lib.pt_frame_window(sp, m, win, 0, 8, d) == -1\n"
        "    assert b'null' in lib.pt_last_error()\n"
    )
    r = subprocess.run([sys.executable, "-c", code, PKG], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


class _NoDevice:
    """A Scene without a device: a window check that let the call through would reach pt_render_window
    with a NULL scene (PT_ERR_INVALID too, but with another message: the tests look at it)."""
    _lib = None
    _h = None


BAD_WINDOWS = [(1, 2), (1, 2, 3), (1, 2, 3, 4, 5), (), (-1, 0, 4, 4), (0, -3, 4, 4), (0, 0, -4, 4), (0, 0, 4, -1),
               (0.5, 0, 4, 4), (0, 0, 4.0, 4), ("0", 0, 4, 4), (0, 0, 4, None), (True, 0, 4, 4), 7, "abcd",
               (0, 0, 1 << 32, 4)]


@pytest.mark.parametrize("window", BAD_WINDOWS, ids=[repr(w) for w in BAD_WINDOWS])
def test_malformed_windows_are_rejected_on_the_host(window):
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    s = _NoDevice()
    s._lib = pt_amd.load_library()
    for call in (lambda: pt_amd.Scene.render(s, meta, 0, 1, window=window),
                 lambda: pt_amd.Scene.frame(s, meta, 0, window=window),
                 lambda: pt_amd.Scene.render_async(s, meta, 0, 1, 1, 8, 0, 0, window=window, row_pitch=8)):
        with pytest.raises(pt_amd.PtError) as e:
            call()
        assert e.value.code == -1 and "window" in str(e.value)


@pytest.mark.parametrize("pitch", [-1, 2.5, "8", 1 << 32])
def test_malformed_row_pitch_is_rejected_on_the_host(pitch):
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    s = _NoDevice()
    s._lib = pt_amd.load_library()
    with pytest.raises(pt_amd.PtError) as e:
        pt_amd.Scene.render_async(s, meta, 0, 1, 1, 8, 0, 0, window=(0, 0, 4, 4), row_pitch=pitch)
    assert e.value.code == -1 and "row_pitch" in str(e.value)


@pytest.mark.parametrize("tile", [(16,), (0, 4), (4, -1), (4.5, 4), 16, (4, 4, 4)])
def test_render_tiled_rejects_malformed_tiles(tile):
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    with pytest.raises(pt_amd.PtError) as e:
        pt_amd.render_tiled(_NoDevice(), meta, 0, 1, tile=tile)
    assert e.value.code == -1 and "tile" in str(e.value)


def test_good_window_is_converted():
    w = pt_amd._lib._window((5, np.int64(3), np.uint8(19), 7))
    assert (w.x0, w.y0, w.w, w.h) == (5, 3, 19, 7)
    assert pt_amd._lib._window(None) is None


@pytest.mark.parametrize("arg", ["1,2", "1,2,3,x", "1,2,0,4", "-1,2,3,4", "1.5,2,3,4", ""])
def test_cli_rejects_a_malformed_window(arg, tmp_path):
    """pt-render.js --window 1,2: a usage message and a non-zero exit before any scene is loaded or
    device touched (no GPU here, and no output written)."""
    r = subprocess.run(["node", os.path.join(PKG, "node", "bin", "pt-render.js"), INI, "--web-root", SCENES,
                        "--out-root", str(tmp_path), "--window", arg], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "usage" in r.stderr and "--window x0,y0,w,h" in r.stderr
    assert os.listdir(tmp_path) == []


def test_node_exports_the_window_entry_points():
    code = ("const h = require(process.argv[1]);"
            "if (typeof h.check_window !== 'function') throw Error('check_window');"
            "if (typeof h.native().renderWindow !== 'function') throw Error('renderWindow');"
            "const many = [1, 2, [0, 0, 1, 1], 0, 1, 1, 8, 0, new Float32Array(3), false, 10, 11];"
            "for (const n of [11, 12, 8, 0]) {"
            "  let terr = null; try { h.native().renderWindow(...many.slice(0, n)); } catch (e) { terr = e.constructor.name; }"
            "  if (terr !== 'TypeError') throw Error('renderWindow with ' + n + ' arguments: ' + terr); }"
            "let t9 = null; try { h.native().render(1, 2, 0, 1, 1, 8, 0, new Float32Array(3), false, 9, 10, 11); }"
            " catch (e) { t9 = e.constructor.name; } if (t9 !== 'TypeError') throw Error('render: ' + t9);"
            "if (String(h.check_window([5, 3, 19, 7])) !== '5,3,19,7' || h.check_window(undefined) !== null) throw Error('ok');"
            "for (const w of [[1, 2], [0, 0, 0, 1], [0, 0, 1.5, 1], [-1, 0, 1, 1], 'x', [0, 0, 1, '1']]) {"
            "  let bad = false; try { h.check_window(w); } catch (e) { bad = /window must be/.test(e.message); }"
            "  if (!bad) throw Error('accepted ' + JSON.stringify(w)); }")
    r = subprocess.run(["node", "-e", code, os.path.join(PKG, "node")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
