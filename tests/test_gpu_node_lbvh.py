"""GPU: scenes built on the device through the Node host.  sceneCreateMesh + sceneExportBvh of the N-API addon
return the bytes of the Python route (Scene.from_mesh(...).export_bvh(), and so the host builder's,
tests/test_gpu_lbvh.py), bvhBuildLbvh the same tree without a GPU; pt-render.js --bvh device renders the image
that the exported tree renders through the packed route."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pt_amd
from conftest import PKG, SCENES

pytestmark = pytest.mark.gpu

W, H = 40, 32
JS = r"""
const fs = require('fs');
const host = require(process.argv[2]);
const [dir, out] = [process.argv[3], process.argv[4]];
const f32 = (p) => { const b = fs.readFileSync(p); const a = new Uint8Array(b.length); a.set(b); return new Float32Array(a.buffer); };
const wr = (p, a) => fs.writeFileSync(p, Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const pt = host.native();
const tri = f32(dir + '/triangle_data.f32');
const scene = pt.sceneCreateMesh(tri);
const scene8 = pt.sceneCreateMesh(tri, { maxLeaf: 8, isolateEmitters: false }, 0);
const packed = pt.sceneCreate(tri, f32(dir + '/bvh_data.f32'), 0);
try {
    wr(out + '/dev.bin', pt.sceneExportBvh(scene));
    wr(out + '/dev8.bin', pt.sceneExportBvh(scene8));
    wr(out + '/host.bin', pt.bvhBuildLbvh(tri));
    wr(out + '/host8.bin', pt.bvhBuildLbvh(tri, { maxLeaf: 8, isolateEmitters: false }));
    let err = '', perr = '', oerr = '';
    try { pt.sceneExportBvh(packed); } catch (e) { err = String(e.message); }
    try { pt.sceneCreateMesh(tri, { maxLeaf: 9 }); } catch (e) { perr = String(e.message); }
    try { pt.sceneCreateMesh(tri, 4); } catch (e) { oerr = String(e.message); }
    console.log(JSON.stringify({ info: pt.sceneInfo(scene), err, perr, oerr }));
} finally {
    pt.sceneDestroy(scene);
    pt.sceneDestroy(scene8);
    pt.sceneDestroy(packed);
}
"""

INI_TEXT = """[IO]
    scene = /scene_assets/CornellBox-Glossy.xml
    output = out/device.png

[Settings]
    imageWidth = %d
    imageHeight = %d
    samplesPerPixel = 3
    pathContinuationProb = 0.9
    directLightingOnly = false
    numDirectLightingSamples = 1
""" % (W, H)


def test_addon_mesh_route_equals_the_python_binding(packed, ptopts):
    p = packed["CornellBox-Glossy"]
    tri = p.triangle_data
    with tempfile.TemporaryDirectory() as td:
        js = os.path.join(td, "m.js")
        with open(js, "w") as f:
            f.write(JS)
        r = subprocess.run(["node", js, os.path.join(PKG, "node"), p.dir, td], check=True, capture_output=True, text=True,
                           timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        got = {n: np.fromfile(os.path.join(td, n + ".bin"), np.uint32) for n in ("dev", "dev8", "host", "host8")}
    with pt_amd.Scene.from_mesh(tri) as s, pt_amd.Scene.from_mesh(tri, max_leaf=8, isolate_emitters=False) as s8:
        want, want8, py_info = s.export_bvh().view(np.uint32), s8.export_bvh().view(np.uint32), s.info
    assert np.array_equal(got["dev"], want) and np.array_equal(got["host"], want)
    assert np.array_equal(got["dev8"], want8) and np.array_equal(got["host8"], want8)
    assert len(want) != len(want8) or not np.array_equal(want, want8)  # the options reach the builder
    assert {k: info["info"][k] for k in ("nodes", "leaves", "leaf_refs", "max_leaf", "max_stack")} == \
           {k: py_info[k] for k in ("nodes", "leaves", "leaf_refs", "max_leaf", "max_stack")}
    assert "not made by pt_scene_create_mesh" in info["err"]
    assert "max_leaf" in info["perr"] and "build options" in info["oerr"]


def test_pt_render_cli_builds_on_the_device(ptopts):
    with tempfile.TemporaryDirectory() as td:
        ini = os.path.join(td, "device.ini")
        with open(ini, "w") as f:
            f.write(INI_TEXT)
        acc_file = os.path.join(td, "accum.f32")
        r = subprocess.run(["node", os.path.join(PKG, "node", "bin", "pt-render.js"), ini, "--web-root", SCENES, "--out-root", td,
                            "--bvh", "device", "--max-depth", "8", "--dump-accum", acc_file], check=True, capture_output=True,
                           text=True, timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        got = np.fromfile(acc_file, np.float32).reshape(H, W, 3)
        png = open(os.path.join(td, "out", "device.png"), "rb").read()
        ps = pt_amd.load_scene(ini, web_root=SCENES)
        # the image of the exported tree, through the packed route and the same pipeline
        with pt_amd.Scene.from_mesh(ps.triangle_data) as s:
            bvh = s.export_bvh()
        with pt_amd.Scene(ps.triangle_data, bvh) as s:
            want = s.render(ps.meta, 0, 3, 1, 8, pt_amd.MODE_AUTO)
        rgba = pt_amd.tonemap(want, 3)
        enc = os.path.join(td, "enc.js")
        with open(enc, "w") as f:
            f.write("const fs = require('fs'); const host = require(process.argv[2]);"
                    "const b = fs.readFileSync(process.argv[3]);"
                    "fs.writeFileSync(process.argv[4], host.encode_png(new Uint8ClampedArray(b), %d, %d));" % (W, H))
        np.asarray(rgba, np.uint8).tofile(os.path.join(td, "rgba.bin"))
        subprocess.run(["node", enc, os.path.join(PKG, "node"), os.path.join(td, "rgba.bin"), os.path.join(td, "want.png")],
                       check=True, capture_output=True, timeout=60)
        want_png = open(os.path.join(td, "want.png"), "rb").read()
    assert (info["width"], info["height"], info["spp"]) == (W, H, 3)
    assert want.any() and got.tobytes() == want.tobytes()
    assert png == want_png
