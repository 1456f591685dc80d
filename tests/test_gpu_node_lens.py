"""GPU: the lens cameras through the Node host.  sceneSetCamera + render of the N-API addon returns the bytes
of the Python binding (and so the reference's, test_gpu_lens.py); pt-render.js --camera thinlens --aperture
0.1 --window ... --counters 1 runs, and the accumulator it dumps is lens_ref's; --projection equirect is
what it was."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cam_cases as cc
import lens_ref as lr
import pt_amd
import radiance_ref as rr
from conftest import PKG, SCENES
from test_gpu_node_radiance import INI_TEXT
from test_gpu_parity import mismatch_report, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
CASE = lr.CASES[1]  # CornellBox, its own camera, thin lens of radius 0.3 focused at 3.6
RENDER_JS = os.path.join(PKG, "node", "bin", "pt-render.js")
JS = r"""
const fs = require('fs');
const host = require(process.argv[2]);
const [dir, out] = [process.argv[3], process.argv[4]];
const raw = (p) => { const b = fs.readFileSync(p); const a = new Uint8Array(b.length); a.set(b); return a.buffer; };
const f32 = (p) => new Float32Array(raw(p));
const pt = host.native();
const scene = pt.sceneCreate(f32(dir + '/triangle_data.f32'), f32(dir + '/bvh_data.f32'), 0);
const save = (name, ta) => fs.writeFileSync(out + '/' + name, Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength));
(async () => {
    try {
        const meta = f32(out + '/meta.f32'), n = meta[0] * meta[1];
        const errs = [];
        for (const cam of [{ model: 'fisheye' }, { model: 'thin_lens', lensRadius: -1, focusDistance: 1 }, { model: 'ortho', focusDistance: 0 }, 7]) {
            try { pt.sceneSetCamera(scene, cam); errs.push(''); } catch (e) { errs.push(String(e.message)); }
        }
        pt.sceneSetCamera(scene, { model: 'thin_lens', lensRadius: 0.3, focusDistance: 3.6 });
        const lens = new Float32Array(3 * n);
        await pt.render(scene, meta, 2, 3, 1, 8, 0, lens, false);
        pt.sceneSetCamera(scene, { model: 'ortho', focusDistance: 3.6 });
        const ortho = new Float32Array(3 * n);
        await pt.render(scene, meta, 2, 3, 1, 8, 0, ortho, false);
        pt.sceneSetCamera(scene, null);
        const pin = new Float32Array(3 * n);
        await pt.render(scene, meta, 2, 3, 1, 8, 0, pin, false);
        save('lens.bin', lens); save('ortho.bin', ortho); save('pin.bin', pin);
        console.log(JSON.stringify({ errs, listed: Object.keys(pt).includes('sceneSetCamera') }));
    } finally {
        pt.sceneDestroy(scene);
    }
})().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
"""


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("radiance_ref"))


def test_addon_equals_the_python_binding(packed, ptopts, ref):
    scene, _, cam = CASE
    p = packed[scene]
    meta, zero, _, _ = lr.reference(ref, packed, CASE)
    ozero = lr.reference(ref, packed, lr.CASES[2])[1]
    h, w = zero.shape[:2]
    with tempfile.TemporaryDirectory() as td:
        np.asarray(meta, F).tofile(os.path.join(td, "meta.f32"))
        js = os.path.join(td, "cam.js")
        with open(js, "w") as f:
            f.write(JS)
        r = subprocess.run(["node", js, os.path.join(PKG, "node"), p.dir, td], check=True, capture_output=True, text=True,
                           timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        lens, ortho, pin = (np.fromfile(os.path.join(td, n), F).reshape(h, w, 3) for n in ("lens.bin", "ortho.bin", "pin.bin"))
    assert all(info["errs"]) and "camera" in info["errs"][1] and "camera" in info["errs"][2] and not info["listed"]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        py_pin = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH)
        s.set_camera(*cam)
        py_lens = s.render(meta, lr.FRAME0, lr.NFRAMES, 1, lr.DEPTH)
    assert lens.tobytes() == py_lens.tobytes() and pin.tobytes() == py_pin.tobytes()
    assert same_bits(lens, zero), mismatch_report(lens, zero)
    assert same_bits(ortho, ozero), mismatch_report(ortho, ozero)


def test_pt_render_cli_camera(packed, ptopts, ref):
    """--camera thinlens --aperture 0.1 with a window and counters: the dumped accumulator is the reference's
    for the window (focus distance: the default, |focus - position| of the scene's camera), and `samples`
    counts its pixels; --camera with the rectangle list and --denoise runs; a bad model is a usage error."""
    win = (9, 6, 31, 17)
    with tempfile.TemporaryDirectory() as td:
        ini = os.path.join(td, "lens.ini")
        with open(ini, "w") as f:
            f.write(INI_TEXT.replace("equirect.png", "lens.png"))
        ps = pt_amd.load_scene(ini, web_root=SCENES)
        acc_f = os.path.join(td, "accum.bin")
        base = ["node", RENDER_JS, ini, "--web-root", SCENES, "--out-root", td, "--max-depth", "8"]
        r = subprocess.run(base + ["--camera", "thinlens", "--aperture", "0.1", "--window", ",".join(map(str, win)), "--counters", "1",
                                   "--dump-accum", acc_f], check=True, capture_output=True, text=True, timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        acc = np.fromfile(acc_f, F).reshape(win[3], win[2], 3)
        more = [subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
                for extra in (["--camera", "ortho", "--window", "0,0,8,8;20,10,9,5"], ["--camera", "equirect", "--denoise"])]
        bad = subprocess.run(base + ["--camera", "fisheye"], capture_output=True, text=True, timeout=120)
    assert [m.returncode for m in more] == [0, 0], [m.stderr for m in more]
    assert bad.returncode == 2 and "--camera" in bad.stderr
    cam = info["camera"]
    assert cam["model"] == "thin_lens" and cam["lensRadius"] == 0.1
    pos, focus = cc.camera("CornellBox", "xml")["pos"], cc.camera("CornellBox", "xml")["focus"]
    assert abs(cam["focusDistance"] - float(np.linalg.norm(np.subtract(focus, pos)))) <= 1e-9
    want, wcnt = lr.render(ref, ps, ps.meta, ("thin_lens", 0.1, cam["focusDistance"]), 0, 4, 8, window=win)
    assert same_bits(acc, want), mismatch_report(acc, want)
    assert (want.sum(axis=2) > 0).mean() >= 0.25
    assert info["counters"]["samples"] == 4 * win[2] * win[3] == wcnt["samples"]


def test_projection_is_unchanged(packed, ptopts, ref):
    """--projection equirect still goes through queryRadiance with its pixel-centre rays: the dump is there
    and --camera was not involved (tests/test_gpu_node_radiance.py pins its bits)."""
    with tempfile.TemporaryDirectory() as td:
        ini = os.path.join(td, "equirect.ini")
        with open(ini, "w") as f:
            f.write(INI_TEXT)
        rays_f = os.path.join(td, "rays.bin")
        r = subprocess.run(["node", RENDER_JS, ini, "--web-root", SCENES, "--out-root", td, "--projection", "equirect",
                            "--max-depth", "8", "--dump-rays", rays_f], check=True, capture_output=True, text=True, timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        both = subprocess.run(["node", RENDER_JS, ini, "--web-root", SCENES, "--out-root", td, "--projection", "equirect",
                               "--window", "0,0,8,8"], capture_output=True, text=True, timeout=120)
        assert os.path.getsize(rays_f) == 64 * 32 * 36
    assert info["projection"] == "equirect" and "camera" not in info
    assert both.returncode == 2 and "--projection" in both.stderr
