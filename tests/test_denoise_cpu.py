"""Guide buffers and the denoiser: the checks that need no GPU.  The symbols and the struct match the
header, null and malformed arguments are rejected before any device call, the CLI rejects a malformed
--denoise, the numpy reference's restated camera ray is the oracle's, and the specified filter (the
reference alone) lowers the error of a 16-frame image."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_ref as dr
import oracle
import pt_amd
from conftest import PKG, SCENES

NEW_FNS = ("pt_render_features", "pt_render_features_async", "pt_denoise_defaults", "pt_denoise", "pt_denoise_async",
           "pt_render_denoised_image")
INI = os.path.join(SCENES, "scene_files", "final", "cornell_box_full_lighting.ini")


# ---------------------------------------------------------------------------------------------
# 1. symbols, header, struct
# ---------------------------------------------------------------------------------------------
def test_library_exports_the_new_functions():
    lib = ctypes.CDLL(pt_amd.lib_path())
    assert [f for f in NEW_FNS if not hasattr(lib, f)] == []
    header = open(os.path.join(os.path.dirname(PKG), "include", "pt_hip.h")).read()
    for f in NEW_FNS:
        assert f + "(" in header
    assert "} pt_denoise_params;" in header
    assert "#define PT_ABI_VERSION 3" in header
    assert pt_amd.abi_version() == 3 == pt_amd.ABI_VERSION


def test_struct_matches_the_header_and_defaults():
    P = pt_amd.DenoiseParams
    assert ctypes.sizeof(P) == 20
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("iters", 0), ("sigma_n", 4), ("sigma_a", 8),
                                                                  ("sigma_z", 12), ("sigma_l", 16)]
    d = pt_amd.denoise_defaults()
    F = np.float32
    assert (d.iters, F(d.sigma_n), F(d.sigma_a), F(d.sigma_z), F(d.sigma_l)) == (4, F(0.5), F(0.3), F(0.1), F(4.0))
    assert dr.DEFAULTS == dict(iters=4, sigma_n=0.5, sigma_a=0.3, sigma_z=0.1, sigma_l=4.0)
    pt_amd.load_library().pt_denoise_defaults(None)  # NULL: nothing to write


def test_denoise_lds_option_takes_0_to_4():
    pt_amd.reset_options()
    try:
        for v in range(5):
            pt_amd.set_option("denoise_lds", v)
            assert pt_amd.get_option("denoise_lds") == str(v)
        for bad in ("5", "-1", "x", "", "1.5"):
            with pytest.raises(pt_amd.PtError) as e:
                pt_amd.set_option("denoise_lds", bad)
            assert e.value.code == -1
    finally:
        pt_amd.reset_options()


# ---------------------------------------------------------------------------------------------
# 2. null and malformed arguments, before any device call
# ---------------------------------------------------------------------------------------------
def test_null_and_malformed_arguments_are_invalid_before_any_device_use():
    """In a child process, with a scene argument that is a zeroed buffer (a call that looked at it, or at
    a device, would not answer PT_ERR_INVALID with these messages)."""
    code = (
        "import ctypes, sys\n"
        "sys.path.insert(0, sys.argv[1])\n"
        "import numpy as np, pt_amd\n"
        "lib = pt_amd.load_library()\n"
        "meta = np.zeros(48, np.float32); meta[0] = meta[1] = 8\n"
        "buf = np.zeros(8 * 8 * 4, np.float32); sq = buf.copy(); g = buf.copy(); a = buf.copy(); out = buf.copy()\n"
        "fr = np.full(4, 4, np.uint32); img = np.zeros(8 * 8 * 4, np.uint8)\n"
        "p = lambda x: x.ctypes.data_as(ctypes.c_void_p)\n"
        "scene = ctypes.create_string_buffer(1 << 16)\n"
        "sp = ctypes.cast(scene, ctypes.c_void_p)\n"
        "err = lambda: lib.pt_last_error().decode()\n"
        "W = pt_amd.Window\n"
        "# NULL scene\n"
        "assert lib.pt_render_features(None, p(meta), None, 0, 1, 1, p(g), p(a), None) == -1 and 'null' in err()\n"
        "assert lib.pt_render_features_async(None, p(meta), None, 0, 1, 1, p(g), p(a), 8, None, None) == -1 and 'null' in err()\n"
        "assert lib.pt_denoise(None, p(buf), p(sq), 8, 8, 4, 4, p(fr), p(g), p(a), 1, None, p(out), None) == -1 and 'null' in err()\n"
        "assert lib.pt_denoise_async(None, p(buf), p(sq), 8, 8, 8, 4, 4, p(fr), p(g), p(a), 1, None, p(out), None, None) == -1\n"
        "assert 'null' in err()\n"
        "assert lib.pt_render_denoised_image(None, p(meta), 0, 4, 1, 8, 0, 2, None, p(img), None) == -1 and 'null' in err()\n"
        "# NULL arguments\n"
        "for m, x, y in ((None, p(g), p(a)), (p(meta), None, p(a)), (p(meta), p(g), None)):\n"
        "    assert lib.pt_render_features(sp, m, None, 0, 1, 1, x, y, None) == -1 and 'null' in err()\n"
        "    assert lib.pt_render_features_async(sp, m, None, 0, 1, 1, x, y, 8, None, None) == -1 and 'null' in err()\n"
        "good = [p(buf), p(sq), p(fr), p(g), p(a), p(out)]\n"
        "for k in range(6):\n"
        "    v = list(good); v[k] = None\n"
        "    assert lib.pt_denoise(sp, v[0], v[1], 8, 8, 4, 4, v[2], v[3], v[4], 1, None, v[5], None) == -1 and 'null' in err()\n"
        "    assert lib.pt_denoise_async(sp, v[0], v[1], 8, 8, 8, 4, 4, v[2], v[3], v[4], 1, None, v[5], None, None) == -1\n"
        "    assert 'null' in err()\n"
        "assert lib.pt_render_denoised_image(sp, None, 0, 4, 1, 8, 0, 2, None, p(img), None) == -1 and 'null' in err()\n"
        "assert lib.pt_render_denoised_image(sp, p(meta), 0, 4, 1, 8, 0, 2, None, None, None) == -1 and 'null' in err()\n"
        "# malformed parameters\n"
        "inf, nan = float('inf'), float('nan')\n"
        "bad = [((0, .5, .3, .1, 4.), 'iters'), ((6, .5, .3, .1, 4.), 'iters'), ((4, 0., .3, .1, 4.), 'sigma_n'),\n"
        "       ((4, nan, .3, .1, 4.), 'sigma_n'), ((4, .5, -1., .1, 4.), 'sigma_a'), ((4, .5, inf, .1, 4.), 'sigma_a'),\n"
        "       ((4, .5, .3, 0., 4.), 'sigma_z'), ((4, .5, .3, nan, 4.), 'sigma_z'), ((4, .5, .3, .1, -4.), 'sigma_l'),\n"
        "       ((4, .5, .3, .1, inf), 'sigma_l')]\n"
        "for fields, name in bad:\n"
        "    q = ctypes.byref(pt_amd.DenoiseParams(*fields))\n"
        "    assert lib.pt_denoise(sp, *good[:2], 8, 8, 4, 4, *good[2:5], 1, q, good[5], None) == -1 and name in err(), (fields, err())\n"
        "    assert lib.pt_denoise_async(sp, *good[:2], 8, 8, 8, 4, 4, *good[2:5], 1, q, good[5], None, None) == -1 and name in err()\n"
        "    assert lib.pt_render_denoised_image(sp, p(meta), 0, 4, 1, 8, 0, 2, q, p(img), None) == -1 and name in err()\n"
        "assert lib.pt_denoise(sp, *good[:2], 8, 8, 4, 4, *good[2:5], 0, None, good[5], None) == -1 and 'feature_frames' in err()\n"
        "assert lib.pt_denoise_async(sp, *good[:2], 8, 8, 8, 4, 4, *good[2:5], 0, None, good[5], None, None) == -1\n"
        "assert 'feature_frames' in err()\n"
        "assert lib.pt_render_denoised_image(sp, p(meta), 0, 4, 1, 8, 0, 0, None, p(img), None) == -1 and 'feature_frames' in err()\n"
        "assert lib.pt_render_denoised_image(sp, p(meta), 0, 1, 1, 8, 0, 2, None, p(img), None) == -1 and 'nframes' in err()\n"
        "# row pitch, grid, window\n"
        "assert lib.pt_denoise_async(sp, *good[:2], 8, 8, 7, 4, 4, *good[2:5], 1, None, good[5], None, None) == -1\n"
        "assert 'row_pitch' in err()\n"
        "for w, h, tw, th in ((0, 8, 4, 4), (8, 0, 4, 4), (8, 8, 0, 4), (8, 8, 4, 0), (40000, 8, 4, 4)):\n"
        "    assert lib.pt_denoise_async(sp, *good[:2], w, h, max(w, 1), tw, th, *good[2:5], 1, None, good[5], None, None) == -1\n"
        "    assert 'null' not in err()\n"
        "win = W(2, 2, 5, 5)\n"
        "assert lib.pt_render_features_async(sp, p(meta), ctypes.byref(win), 0, 1, 1, p(g), p(a), 4, None, None) == -1\n"
        "assert 'row_pitch' in err()\n"
        "assert lib.pt_render_features_async(sp, p(meta), None, 0, 1, 1, p(g), p(a), 7, None, None) == -1 and 'row_pitch' in err()\n"
        "for bw in (W(4, 0, 5, 2), W(0, 7, 2, 2), W(0, 0, 0, 2), W(0, 0, 2, 0)):\n"
        "    assert lib.pt_render_features(sp, p(meta), ctypes.byref(bw), 0, 1, 1, p(g), p(a), None) == -1 and 'window' in err()\n"
        "    assert lib.pt_render_features_async(sp, p(meta), ctypes.byref(bw), 0, 1, 1, p(g), p(a), 8, None, None) == -1\n"
        "    assert 'window' in err()\n"
        "assert lib.pt_render_features_async(sp, p(meta), None, (1 << 24) - 1, 2, 1, p(g), p(a), 8, None, None) == -1\n"
        "assert '2^24' in err()\n"
    )
    r = subprocess.run([sys.executable, "-c", code, PKG], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


class _NoDevice:
    _lib = None
    _h = None


def _scene():
    s = _NoDevice()
    s._lib = pt_amd.load_library()
    return s


BAD_PARAMS = [dict(iters=0), dict(iters=6), dict(iters=2.0), dict(iters=-1), dict(sigma_n=0), dict(sigma_a=float("nan")),
              dict(sigma_z=-0.1), dict(sigma_l=float("inf")), dict(sigma_l="4"), dict(sigma_q=1.0), 5,
              pt_amd.DenoiseParams(0, 0.5, 0.3, 0.1, 4.0), pt_amd.DenoiseParams(4, 0.5, 0.0, 0.1, 4.0)]


@pytest.mark.parametrize("params", BAD_PARAMS, ids=[repr(b)[:40] for b in BAD_PARAMS])
def test_malformed_parameters_are_rejected_on_the_host(params):
    acc = np.zeros((8, 8, 3), np.float32)
    g = np.zeros((8, 8, 4), np.float32)
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    for call in (lambda: pt_amd.Scene.denoise(_scene(), acc, acc, g, g, 2, 4, params=params),
                 lambda: pt_amd.Scene.denoise_async(_scene(), 1, 1, 8, 8, (8, 8), 1, 1, 1, 2, 1, params=params),
                 lambda: pt_amd.Scene.render_denoised(_scene(), meta, 0, 4, params=params)):
        with pytest.raises(pt_amd.PtError) as e:
            call()
        assert e.value.code == -1 and "null" not in str(e.value)


def test_malformed_buffers_and_counts_are_rejected_on_the_host():
    s = _scene()
    acc = np.zeros((8, 8, 3), np.float32)
    g = np.zeros((8, 8, 4), np.float32)
    meta = np.zeros(48, np.float32)
    meta[0], meta[1] = 8, 8
    cases = [(lambda: pt_amd.Scene.denoise(s, acc, acc, g, g, 0, 4), "feature_frames"),
             (lambda: pt_amd.Scene.denoise(s, acc, acc, g[:4], g, 2, 4), "geo"),
             (lambda: pt_amd.Scene.denoise(s, acc, acc[:4], g, g, 2, 4), "m2"),
             (lambda: pt_amd.Scene.denoise(s, acc, acc, g, g, 2, [4, 4]), "frames"),
             (lambda: pt_amd.Scene.denoise(s, acc, acc, g, g, 2, [4, 4, 4], tile=(4, 4)), "frames"),
             (lambda: pt_amd.Scene.denoise(s, acc, acc, g, g, 2, 4, tile=(0, 4)), "tile"),
             (lambda: pt_amd.Scene.denoise_async(s, 1, 1, 8, 8, (8, 8), 1, 1, 1, 2, 1, row_pitch=-1), "row_pitch"),
             (lambda: pt_amd.Scene.render_denoised(s, meta, 0, 1), "nframes"),
             (lambda: pt_amd.Scene.render_denoised(s, meta, 0, 4, feature_frames=0), "feature_frames"),
             (lambda: pt_amd.Scene.render_features_async(s, meta, 0, 1, 1, 16, 16, row_pitch=1.5), "row_pitch"),
             (lambda: pt_amd.Scene.render_features(s, meta, 0, 1, window=(0, 0, 4)), "window")]
    for call, name in cases:
        with pytest.raises(pt_amd.PtError) as e:
            call()
        assert e.value.code == -1 and name in str(e.value), (name, str(e.value))
    with pytest.raises(ValueError):
        pt_amd.Scene.render_features(s, meta, 0, 1, geo=np.zeros((8, 8, 3), np.float32))


# ---------------------------------------------------------------------------------------------
# 3. the CLI
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--denoise", "x"], ["--denoise", "6"], ["--denoise", "0"], ["--denoise", "2", "--feature-frames", "0"],
                                   ["--denoise", "--feature-frames", "1.5"], ["--denoise", "2", "--window", "0,0,4,4"],
                                   ["--denoise", "2", "--counters", "1"]],
                         ids=lambda e: " ".join(e))
def test_cli_rejects_a_malformed_denoise(extra):
    r = subprocess.run(["node", os.path.join(PKG, "node", "bin", "pt-render.js"), INI, "--web-root", SCENES] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert r.stderr.startswith("usage: pt-render.js") and "--denoise" in r.stderr


def test_program_entry_rejects_what_denoise_cannot_honour():
    """denoise is one device call for the whole image: every option it could only ignore is an Error,
    raised before a scene is created (so without a device)."""
    script = r"""
const host = require(process.argv[1]);
(async () => {
    const s = host.load_scene_from_ini(process.argv[2], { web_root: process.argv[3], quiet: true });
    const out = {};
    for (const [k, v] of Object.entries({ imageOnly: true, chunk: 2, counters: true, window: [0, 0, 2, 2], rects: [[0, 0, 2, 2]],
                                          onFrames: () => 0, devices: [0, 1] })) {
        try {
            await host.programEntry(s.screenDimension, s.primitive_data, s.camera_data, s.scene_description, { denoise: true, [k]: v });
            out[k] = null;
        } catch (e) { out[k] = e.message; }
    }
    console.log(JSON.stringify(out));
})().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
"""
    import json
    r = subprocess.run(["node", "-e", script, os.path.join(PKG, "node"), INI, SCENES], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(out) == {"imageOnly", "chunk", "counters", "window", "rects", "onFrames", "devices"}
    for k, msg in out.items():
        assert msg and msg.startswith("denoise: not with"), (k, msg)


# ---------------------------------------------------------------------------------------------
# 4. the reference itself: the restated primary ray is the oracle's
# ---------------------------------------------------------------------------------------------
def _hits(packed, scene, w, h):
    p = packed[scene]
    return p, dr.first_hits(scene, p, w, h)


def test_restated_primary_hits_are_the_oracles(packed):
    """Every pixel whose restated first hit is an emitter holds exactly that Ke in the oracle's frame
    (depth 0: L = Ke): the restated ray and the oracle's reach the same triangle."""
    W, H = 40, 24
    p, fh = _hits(packed, "CornellBox", W, H)
    rad, _ = oracle.frame(p.triangle_data, p.bvh_data, p.meta_for(W, H), 0, 8)
    emitters = misses = 0
    for y in range(H):
        for x in range(W):
            n, t, a, emits, _ = fh.hit(x, y, 0)
            if n is None:
                misses += 1
                assert np.all(rad[y, x] == 0)
            elif emits:
                emitters += 1
                assert rad[y, x].tobytes() == np.asarray(a, np.float32).tobytes(), (x, y)
    assert emitters >= 1 and misses >= 1


# ---------------------------------------------------------------------------------------------
# 5. quality of the specified filter (numpy reference alone)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Sphere"])
def test_reference_filter_halves_the_relative_mse(packed, scene):
    W = H = 64
    p, fh = _hits(packed, scene, W, H)
    meta = p.meta_for(W, H)
    frames = [oracle.frame(p.triangle_data, p.bvh_data, meta, k, 8)[0] for k in range(16)]
    acc = np.zeros((H, W, 3), np.float32)
    m2 = np.zeros((H, W, 3), np.float32)
    for L in frames:
        c = np.where(L >= 0, L, 0).astype(np.float32)
        acc = acc + c
        m2 = m2 + c * c
    geo, alb, _ = fh.features((0, 0, W, H), 0, 4, 1)
    ref, _ = oracle.render(p.triangle_data, p.bvh_data, meta, 1000, 512, 1, 8)
    ref = ref / np.float32(512)
    out, var = dr.denoise(acc, m2, 16, geo, alb, 4)
    noisy, den = dr.rel_mse(acc / np.float32(16), ref), dr.rel_mse(out, ref)
    print(f"{scene}: relMSE noisy {noisy:.4f} denoised (defaults, 4 passes) {den:.4f}")
    assert np.all(np.isfinite(out)) and np.all(var >= 0)
    assert den <= 0.5 * noisy, (noisy, den)
