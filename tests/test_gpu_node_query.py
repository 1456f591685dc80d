"""GPU: the ray queries through the Node host.  queryHits and queryOccluded of the N-API addon return the
bytes of the Python binding (and so the oracle's, test_gpu_query.py) on CornellBox's batches; cameraRays
returns pt_camera_rays' rays; pt-render.js --pick prints the oracle's hit of a pixel's frame-0 camera ray,
for a pixel on the box and for one beside it."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import denoise_ref as dr
import oracle
import pt_amd
import query_ref as qr
from conftest import PKG, SCENES
from test_gpu_window import H, W

pytestmark = pytest.mark.gpu

JS = r"""
const fs = require('fs');
const host = require(process.argv[2]);
const [dir, out] = [process.argv[3], process.argv[4]];
const f32 = (p) => { const b = fs.readFileSync(p); const a = new Uint8Array(b.length); a.set(b); return new Float32Array(a.buffer); };
const pt = host.native();
const scene = pt.sceneCreate(f32(dir + '/triangle_data.f32'), f32(dir + '/bvh_data.f32'), 0);
try {
    const hits = host.queryHits(scene, f32(out + '/rays.f32'));
    const occ = host.queryOccluded(scene, f32(out + '/occ_rays.f32'));
    const cam = host.cameraRays(scene, f32(out + '/meta.f32'), 3);
    const win = host.cameraRays(scene, f32(out + '/meta.f32'), 3, [5, 3, 19, 7]);
    const none = host.queryHits(scene, new Float32Array(0));
    let err = '';
    try { host.queryHits(scene, new Float32Array(7)); } catch (e) { err = String(e.message); }
    let werr = '';
    try { host.cameraRays(scene, f32(out + '/meta.f32'), 3, [30, 0, 32768, 32768]); } catch (e) { werr = String(e.message); }
    fs.writeFileSync(out + '/hits.bin', Buffer.from(hits.buffer, hits.byteOffset, hits.byteLength));
    fs.writeFileSync(out + '/occ.bin', Buffer.from(occ.buffer, occ.byteOffset, occ.byteLength));
    fs.writeFileSync(out + '/cam.bin', Buffer.from(cam.buffer, cam.byteOffset, cam.byteLength));
    fs.writeFileSync(out + '/win.bin', Buffer.from(win.buffer, win.byteOffset, win.byteLength));
    console.log(JSON.stringify({ hits: hits.constructor.name, occ: occ.constructor.name, none: none.length, err, werr }));
} finally {
    pt.sceneDestroy(scene);
}
"""

INI_TEXT = """[IO]
    scene = /scene_assets/CornellBox.xml
    output = out/pick.png

[Settings]
    imageWidth = %d
    imageHeight = %d
    samplesPerPixel = 1
    pathContinuationProb = 0.9
    directLightingOnly = false
    numDirectLightingSamples = 1
""" % (W, H)


def test_addon_queries_equal_the_python_binding(packed, ptopts):
    scene = "CornellBox"
    p, b = packed[scene], qr.batch(scene, packed)
    meta = p.meta_for(W, H)
    with tempfile.TemporaryDirectory() as td:
        b.rays.tofile(os.path.join(td, "rays.f32"))
        b.occ_rays.tofile(os.path.join(td, "occ_rays.f32"))
        meta.astype(np.float32).tofile(os.path.join(td, "meta.f32"))
        js = os.path.join(td, "q.js")
        with open(js, "w") as f:
            f.write(JS)
        r = subprocess.run(["node", js, os.path.join(PKG, "node"), p.dir, td], check=True, capture_output=True, text=True,
                           timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        hits = np.fromfile(os.path.join(td, "hits.bin"), np.float32).reshape(-1, 8)
        occ = np.fromfile(os.path.join(td, "occ.bin"), np.uint8)
        cam = np.fromfile(os.path.join(td, "cam.bin"), np.float32)
        win = np.fromfile(os.path.join(td, "win.bin"), np.float32)
    assert info["hits"] == "Float32Array" and info["occ"] == "Uint8Array" and info["none"] == 0
    assert "queryHits(scene, Float32Array rays[8n])" in info["err"]
    assert "lie within the image" in info["werr"]  # refused before its 32 GB result would be allocated
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        py_hits, py_occ = s.query_hits(b.rays), s.query_occluded(b.occ_rays)
        py_cam, py_win = s.camera_rays(meta, 3), s.camera_rays(meta, 3, window=(5, 3, 19, 7))
    assert hits.tobytes() == py_hits.tobytes() and occ.tobytes() == py_occ.tobytes()
    assert cam.tobytes() == py_cam.tobytes() and win.tobytes() == py_win.tobytes()
    assert not qr.hits_mismatch(hits, b) and np.array_equal(occ, b.occ)
    assert py_hits[:, 3].max() > 0 and occ.any() and not occ.all()


def test_pt_render_cli_pick(packed, ptopts):
    """One pixel on the box and one beside it: the oracle's intersect of the pixel's frame-0 camera ray."""
    with tempfile.TemporaryDirectory() as td:
        ini = os.path.join(td, "pick.ini")
        with open(ini, "w") as f:
            f.write(INI_TEXT)
        ps = pt_amd.load_scene(ini, web_root=SCENES)
        seen = set()
        for x, y in ((20, 12), (1, 1)):
            r = subprocess.run(["node", os.path.join(PKG, "node", "bin", "pt-render.js"), ini, "--web-root", SCENES,
                                "--out-root", td, "--pick", f"{x},{y}"], check=True, capture_output=True, text=True, timeout=120)
            lines = r.stdout.strip().splitlines()
            assert len(lines) == 1
            info = json.loads(lines[0])
            o, d = dr.camera_ray(ps.meta, x, y, 0)
            ok, out, _ = oracle.intersect(ps.triangle_data, ps.bvh_data, o, d)
            want = qr.hit_record(out) if ok else qr.MISS
            assert info["pick"] == [x, y] and (info["width"], info["height"]) == (W, H)
            assert info["hit"] == ok and info["material"] == int(want[7:8].view(np.int32)[0])
            assert info["bits"] == want.view(np.uint32).tolist(), (info, want)
            assert np.float32(info["t"]) == want[3] and np.array_equal(np.array(info["p"], np.float32), want[0:3])
            assert np.array_equal(np.array(info["ray"]["d"], np.float32), d[:3])
            seen.add(ok)
        assert not os.path.exists(os.path.join(td, "out"))  # nothing rendered, nothing written
    assert seen == {True, False}
