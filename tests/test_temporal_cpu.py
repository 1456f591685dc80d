"""Temporal accumulation: the checks that need no GPU.  The symbols and the struct match the header, null,
mixed, aliasing and malformed arguments are rejected before any device call, the CLI rejects a malformed
--temporal, the reference's vectorised fmaf is libm's, and the specified step (the numpy reference alone)
reproduces a plain render under a static camera and lowers the error along an orbit."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as ar
import cam_cases as cc
import denoise_ref as dr
import oracle
import pt_amd
import temporal_ref as tr
from conftest import PKG, SCENES

NEW_FNS = ("pt_temporal_defaults", "pt_reproject", "pt_reproject_async", "pt_denoise_mean", "pt_denoise_mean_async",
           "pt_history_create", "pt_history_reset", "pt_history_destroy", "pt_history_step")
INI = os.path.join(SCENES, "scene_files", "final", "cornell_box_full_lighting.ini")
F = np.float32
DEPTH = 8


# ---------------------------------------------------------------------------------------------
# 1. symbols, header, struct
# ---------------------------------------------------------------------------------------------
def test_library_exports_the_new_functions():
    lib = ctypes.CDLL(pt_amd.lib_path())
    assert [f for f in NEW_FNS if not hasattr(lib, f)] == []
    header = open(os.path.join(os.path.dirname(PKG), "include", "pt_hip.h")).read()
    for f in NEW_FNS:
        assert f + "(" in header
    assert "} pt_temporal_params;" in header and "typedef struct pt_history pt_history;" in header
    assert "#define PT_ABI_VERSION 3" in header
    assert pt_amd.abi_version() == 3 == pt_amd.ABI_VERSION


def test_struct_matches_the_header_and_defaults():
    P = pt_amd.TemporalParams
    assert ctypes.sizeof(P) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("alpha", 0), ("normal_min", 4), ("depth_tol", 8),
                                                                  ("max_history", 12)]
    d = pt_amd.temporal_defaults()
    assert (F(d.alpha), F(d.normal_min), F(d.depth_tol), F(d.max_history)) == (F(0.2), F(0.9), F(0.1), F(64.0))
    assert tr.DEFAULTS == dict(alpha=0.2, normal_min=0.9, depth_tol=0.1, max_history=64.0)
    pt_amd.load_library().pt_temporal_defaults(None)  # NULL: nothing to write


# ---------------------------------------------------------------------------------------------
# 2. null, mixed, aliasing and malformed arguments, before any device call
# ---------------------------------------------------------------------------------------------
def test_invalid_arguments_are_rejected_before_any_device_use():
    """In a child process, with a scene argument that is a zeroed buffer (a call that looked at it, or at
    a device, would not answer PT_ERR_INVALID with these messages)."""
    code = (
        "import ctypes, sys\n"
        "sys.path.insert(0, sys.argv[1])\n"
        "import numpy as np, pt_amd\n"
        "lib = pt_amd.load_library()\n"
        "meta = np.zeros(48, np.float32); meta[0] = meta[1] = 8\n"
        "m9 = meta.copy(); m9[0] = 9\n"
        "mk = lambda k: np.zeros(8 * 8 * k, np.float32)\n"
        "acc, sq, g, a, out, var = mk(3), mk(3), mk(4), mk(4), mk(3), mk(1)\n"
        "prev = [mk(4) for _ in range(3)]; new = [mk(4) for _ in range(3)]; img = np.zeros(8 * 8 * 4, np.uint8)\n"
        "p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)\n"
        "scene = ctypes.create_string_buffer(1 << 16)\n"
        "sp = ctypes.cast(scene, ctypes.c_void_p)\n"
        "err = lambda: lib.pt_last_error().decode()\n"
        "def rp(s=sp, acc=acc, sq=sq, n=2, g=g, a=a, mc=meta, mp=meta, prev=prev, w=8, h=8, pitch=8, prm=None, new=new):\n"
        "    q = None if prm is None else ctypes.byref(pt_amd.TemporalParams(*prm))\n"
        "    r1 = lib.pt_reproject_async(s, p(acc), p(sq), n, p(g), p(a), p(mc), p(mp), *(p(x) for x in prev), w, h, pitch, q,\n"
        "                                *(p(x) for x in new), p(out), p(var), None)\n"
        "    e1 = err()\n"
        "    r2 = lib.pt_reproject(s, p(acc), p(sq), n, p(g), p(a), p(mc), p(mp), *(p(x) for x in prev), w, h, q,\n"
        "                          *(p(x) for x in new), p(out), p(var))\n"
        "    return r1, e1, r2, err()\n"
        "def bad(word, **kw):\n"
        "    r1, e1, r2, e2 = rp(**kw)\n"
        "    assert r1 == -1 and word in e1, (kw.keys(), e1)\n"
        "    assert r2 == -1 and word in e2, (kw.keys(), e2)\n"
        "# NULL arguments\n"
        "bad('null', s=None)\n"
        "for k in ('acc', 'sq', 'g', 'a', 'mc'):\n"
        "    bad('null', **{k: None})\n"
        "for k in range(3):\n"
        "    v = list(new); v[k] = None\n"
        "    bad('null', new=v)\n"
        "# a mixed history set\n"
        "bad('all NULL or all given', mp=None)\n"
        "for k in range(3):\n"
        "    v = list(prev); v[k] = None\n"
        "    bad('all NULL or all given', prev=v)\n"
        "bad('all NULL or all given', prev=[None] * 3)\n"
        "# aliasing\n"
        "for k in range(3):\n"
        "    for l in range(3):\n"
        "        v = list(new); v[l] = prev[k]\n"
        "        bad('alias', new=v)\n"
        "bad('alias', new=[new[0], new[0], new[2]])\n"
        "# W, H\n"
        "bad('meta_cur', mc=m9)\n"
        "bad('meta_prev', mp=m9)\n"
        "bad('meta_cur', w=7, pitch=8)\n"
        "bad('n must', n=0)\n"
        "r = lib.pt_reproject_async(sp, p(acc), p(sq), 2, p(g), p(a), p(meta), None, None, None, None, 8, 8, 7, None,\n"
        "                           *(p(x) for x in new), None, None, None)\n"
        "assert r == -1 and 'row_pitch' in err()\n"
        "# parameters\n"
        "inf, nan = float('inf'), float('nan')\n"
        "for prm, name in (((0., .9, .1, 64.), 'alpha'), ((1.5, .9, .1, 64.), 'alpha'), ((-.2, .9, .1, 64.), 'alpha'),\n"
        "                  ((nan, .9, .1, 64.), 'alpha'), ((.2, nan, .1, 64.), 'normal_min'), ((.2, inf, .1, 64.), 'normal_min'),\n"
        "                  ((.2, .9, 0., 64.), 'depth_tol'), ((.2, .9, -1., 64.), 'depth_tol'), ((.2, .9, inf, 64.), 'depth_tol'),\n"
        "                  ((.2, .9, .1, .5), 'max_history'), ((.2, .9, .1, nan), 'max_history'), ((.2, .9, .1, inf), 'max_history')):\n"
        "    bad(name, prm=prm)\n"
        "# pt_denoise_mean\n"
        "good = [p(acc), p(var), p(g), p(a), p(out)]\n"
        "assert lib.pt_denoise_mean(None, *good[:2], 8, 8, *good[2:4], 1, None, good[4], None) == -1 and 'null' in err()\n"
        "for k in range(5):\n"
        "    v = list(good); v[k] = None\n"
        "    assert lib.pt_denoise_mean(sp, *v[:2], 8, 8, *v[2:4], 1, None, v[4], None) == -1 and 'null' in err()\n"
        "    assert lib.pt_denoise_mean_async(sp, *v[:2], 8, 8, 8, *v[2:4], 1, None, v[4], None, None) == -1 and 'null' in err()\n"
        "q = ctypes.byref(pt_amd.DenoiseParams(6, .5, .3, .1, 4.))\n"
        "assert lib.pt_denoise_mean(sp, *good[:2], 8, 8, *good[2:4], 1, q, good[4], None) == -1 and 'iters' in err()\n"
        "assert lib.pt_denoise_mean_async(sp, *good[:2], 8, 8, 8, *good[2:4], 1, q, good[4], None, None) == -1 and 'iters' in err()\n"
        "assert lib.pt_denoise_mean(sp, *good[:2], 8, 8, *good[2:4], 0, None, good[4], None) == -1 and 'feature_frames' in err()\n"
        "assert lib.pt_denoise_mean_async(sp, *good[:2], 8, 8, 7, *good[2:4], 1, None, good[4], None, None) == -1\n"
        "assert 'row_pitch' in err()\n"
        "# pt_history\n"
        "hd = ctypes.c_void_p()\n"
        "assert lib.pt_history_create(None, 8, 8, ctypes.byref(hd)) == -1 and 'null' in err()\n"
        "assert lib.pt_history_create(sp, 8, 8, None) == -1 and 'null' in err()\n"
        "assert lib.pt_history_create(sp, 0, 8, ctypes.byref(hd)) == -1 and 'w and h' in err()\n"
        "assert lib.pt_history_reset(None) == -1 and 'null' in err()\n"
        "assert lib.pt_history_step(None, p(meta), 0, 2, 1, 8, 0, 1, None, None, None, None, None, None, None) == -1\n"
        "assert 'null' in err()\n"
        "lib.pt_history_destroy(None)\n"
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


BAD_PARAMS = [dict(alpha=0), dict(alpha=1.5), dict(alpha=float("nan")), dict(normal_min=float("inf")), dict(depth_tol=0),
              dict(depth_tol=-0.1), dict(max_history=0.5), dict(max_history="64"), dict(beta=1.0), 5,
              pt_amd.TemporalParams(0.0, 0.9, 0.1, 64.0), pt_amd.TemporalParams(0.2, 0.9, 0.1, 0.0)]


@pytest.mark.parametrize("params", BAD_PARAMS, ids=[repr(b)[:40] for b in BAD_PARAMS])
def test_malformed_parameters_are_rejected_on_the_host(params):
    acc = np.zeros((8, 8, 3), F)
    g = np.zeros((8, 8, 4), F)
    meta = np.zeros(48, F)
    meta[0], meta[1] = 8, 8
    for call in (lambda: pt_amd.Scene.reproject(_scene(), acc, acc, 2, g, g, meta, params=params),
                 lambda: pt_amd.Scene.reproject_async(_scene(), 1, 1, 2, 1, 1, meta, 8, 8, 1, 1, 1, params=params)):
        with pytest.raises(pt_amd.PtError) as e:
            call()
        assert e.value.code == -1 and "null" not in str(e.value)


def test_malformed_buffers_are_rejected_on_the_host():
    s = _scene()
    acc = np.zeros((8, 8, 3), F)
    g = np.zeros((8, 8, 4), F)
    v = np.zeros((8, 8), F)
    meta = np.zeros(48, F)
    meta[0], meta[1] = 8, 8
    prev = dict(meta=meta, hist=g, mom=g, gbuf=g[:4])
    cases = [(lambda: pt_amd.Scene.reproject(s, acc, acc[:4], 2, g, g, meta), "m2"),
             (lambda: pt_amd.Scene.reproject(s, acc, acc, 2, g[:4], g, meta), "geo"),
             (lambda: pt_amd.Scene.reproject(s, acc, acc, 0, g, g, meta), "n must"),
             (lambda: pt_amd.Scene.reproject(s, acc, acc, 2, g, g, meta[:40]), "meta"),
             (lambda: pt_amd.Scene.reproject(s, acc, acc, 2, g, g, meta, prev=prev), "prev"),
             (lambda: pt_amd.Scene.denoise_mean(s, acc, v[:4], g, g, 2), "var"),
             (lambda: pt_amd.Scene.denoise_mean(s, acc, v, g, g[:4], 2), "alb"),
             (lambda: pt_amd.Scene.denoise_mean(s, acc, v, g, g, 0), "feature_frames"),
             (lambda: pt_amd.Scene.denoise_mean(s, acc, v, g, g, 2, params=dict(iters=6)), "iters"),
             (lambda: pt_amd.Scene.denoise_mean_async(s, 1, 1, 8, 8, 1, 1, 2, 1, row_pitch=-1), "row_pitch")]
    for call, name in cases:
        with pytest.raises(pt_amd.PtError) as e:
            call()
        assert e.value.code == -1 and name in str(e.value), (name, str(e.value))


# ---------------------------------------------------------------------------------------------
# 3. the CLI
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--turntable", "4", "--temporal", "x"], ["--turntable", "4", "--temporal", "0"],
                                   ["--turntable", "4", "--temporal", "1.5"], ["--turntable", "4", "--temporal", "-0.2"],
                                   ["--temporal"], ["--temporal", "0.2"],
                                   ["--turntable", "4", "--temporal", "--window", "0,0,4,4"],
                                   ["--turntable", "4", "--temporal", "--counters", "1"]],
                         ids=lambda e: " ".join(e))
def test_cli_rejects_a_malformed_temporal(extra):
    r = subprocess.run(["node", os.path.join(PKG, "node", "bin", "pt-render.js"), INI, "--web-root", SCENES] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert r.stderr.startswith("usage: pt-render.js") and "--temporal" in r.stderr


# ---------------------------------------------------------------------------------------------
# 4. the reference itself
# ---------------------------------------------------------------------------------------------
def test_vectorised_fmaf_is_libms():
    """Random triples, half of them with c within a few ulps of -a * b (the cancellation a double-rounded
    sum gets wrong)."""
    rng = np.random.default_rng(7)
    n = 20000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F)
    b = rng.standard_normal(n).astype(F)
    c = (-a * b * (1 + rng.integers(-3, 4, n) * F(2 ** -23))).astype(F)
    c[::2] = rng.standard_normal(n // 2).astype(F)
    got = tr.fmaf(a, b, c)
    ref = np.array([dr.fmaf(x, y, z) for x, y, z in zip(a, b, c)], F)
    assert got.dtype == F and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # cases the double-rounded (a * b + c in f64, then f32) sum gets wrong are among them
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    print("double rounding differs in", int((naive.view(np.uint32) != ref.view(np.uint32)).sum()), "of", n)


def ref_steps(p, metas, n, feature_frames, W, H, **params):
    """The reference's steps along metas: step k renders frames k * n .. k * n + n - 1 (oracle.frame) and its
    guides from the first feature_frames of them.  Every dict also holds the step's raw n-frame mean."""
    prev, out = None, []
    for k, meta in enumerate(metas):
        acc, m2 = ar.moments([oracle.frame(p.triangle_data, p.bvh_data, meta, k * n + i, DEPTH)[0] for i in range(n)])
        geo, alb, _ = dr.FirstHits(p.triangle_data, p.bvh_data, meta).features((0, 0, W, H), k * n, feature_frames, 1)
        prev = tr.reproject(acc, m2, n, geo, alb, meta, prev, **params)
        prev["raw"] = (acc / F(n)).astype(F)
        out.append(prev)
    return out


# measured with the reference (printed by the test): the largest |accumulated - plain| over the image — at
# pixels on an edge, where the mean depth or normal of a step's two jittered guide frames fails the tap test and
# the history starts again or, the own tap failing, is a neighbour's whose tap has a weight of 1e-5 — and over
# the pixels whose history never started again (N' = k at every step k: a pure rounding difference)
STATIC_MAX_DIFF = 0.5565
STATIC_MAX_DIFF_WHOLE = 2.74e-6


def test_reference_static_camera_is_the_plain_mean(packed):
    """Six steps of two frames under one camera, alpha so small that a = 1 / N' throughout: the
    accumulated mean is the running mean of frames 0..11, up to the rounding of the reprojected position
    (u = x only up to an ulp, so the own pixel's tap has weight 1 - eps) and of the incremental mean."""
    W, H, K, n = 32, 24, 6, 2
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    s = ref_steps(p, [meta] * K, n, n, W, H, alpha=0.01)
    ref, _ = oracle.render(p.triangle_data, p.bvh_data, meta, 0, K * n, 1, DEPTH)
    ref = ref / F(K * n)
    d = np.abs(s[-1]["out"].astype(np.float64) - ref)
    whole = np.all([np.abs(st["hist"][..., 3] - F(k + 1)) < 1e-3 for k, st in enumerate(s)], axis=0)
    print(f"static camera: max |diff| {d.max():.6g} (all), {d[whole].max():.6g} (N' = k at every step k, {whole.mean():.3f} "
          f"of the pixels), mean radiance {ref.mean():.4f}")
    # a pixel that misses the scene (a third of this image) has Z = 0 and N' = 1 at every step by the rule, and is
    # black in both images; of the pixels that hit, three quarters never start again — the others lie on an edge
    hit = np.all([st["gbuf"][..., 3] > 0 for st in s], axis=0)
    print(f"static camera: {hit.mean():.3f} of the pixels hit at every step; {whole[hit].mean():.3f} of those never start again")
    assert whole[hit].mean() > 0.7
    assert d.max() <= 4 * STATIC_MAX_DIFF
    assert d[whole].max() <= 4 * STATIC_MAX_DIFF_WHOLE


ORBIT_DEGREES = 2.0  # per step, about the focus: the first angle tried; 0.958 of the hit pixels end with N' >= 4
ORBIT_GAIN = 5.72    # measured with the reference (printed by the test): relMSE raw 0.3331 / accumulated 0.0583


def orbit_meta(k, W, H, degrees=ORBIT_DEGREES):
    a = math.radians(degrees * k)
    return cc.meta_from(cc.cam((3.6 * math.sin(a), 1.0, 3.6 * math.cos(a)), (0, 1, 0)), W, H)


def test_reference_orbit_lowers_the_relative_mse(packed):
    """Eight cameras on an orbit, two frames each on disjoint frame ranges, the defaults: the last step's
    accumulated mean against its own raw two-frame mean, both measured against 512 frames of the last camera."""
    W = H = 64
    p = packed["CornellBox"]
    metas = [orbit_meta(k, W, H) for k in range(8)]
    last = ref_steps(p, metas, 2, 2, W, H)[-1]
    ref, _ = oracle.render(p.triangle_data, p.bvh_data, metas[-1], 1000, 512, 1, DEPTH)
    ref = ref / F(512)
    hit = last["gbuf"][..., 3] > 0
    long = float((last["hist"][..., 3][hit] >= 4).mean())
    raw, acc = dr.rel_mse(last["raw"], ref), dr.rel_mse(last["out"], ref)
    print(f"orbit {ORBIT_DEGREES} deg: relMSE raw {raw:.4f} accumulated {acc:.4f} gain {raw / acc:.2f}; N' >= 4 at {long:.3f} "
          "of the hit pixels")
    assert np.all(np.isfinite(last["out"])) and np.all(last["var"] >= 0)
    assert long >= 0.8  # the gain is not the disoccluded pixels' alone
    assert raw / acc >= 0.5 * ORBIT_GAIN, (raw, acc)
