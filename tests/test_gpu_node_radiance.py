"""GPU: the radiance queries through the Node host.  queryRadiance and cameraSeeds of the N-API addon return
the bytes of the Python binding (and so the reference's, test_gpu_radiance.py) on CornellBox's mixed
family; pt-render.js --projection equirect renders 64 x 32 x 4 spp through queryRadiance: the rays and
seeds it dumps are the ones its header documents, and its accumulator is radiance_ref's on them."""
import io
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
from PIL import Image

import oracle
import pt_amd
import radiance_ref as rr
from conftest import PKG, SCENES
from test_gpu_parity import mismatch_report, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
JS = r"""
const fs = require('fs');
const host = require(process.argv[2]);
const [dir, out] = [process.argv[3], process.argv[4]];
const raw = (p) => { const b = fs.readFileSync(p); const a = new Uint8Array(b.length); a.set(b); return a.buffer; };
const f32 = (p) => new Float32Array(raw(p)), u32 = (p) => new Uint32Array(raw(p));
const pt = host.native();
const scene = pt.sceneCreate(f32(dir + '/triangle_data.f32'), f32(dir + '/bvh_data.f32'), 0);
const save = (name, ta) => fs.writeFileSync(out + '/' + name, Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength));
try {
    const rays = f32(out + '/rays.f32'), seeds = u32(out + '/seeds.u32'), meta = f32(out + '/meta.f32');
    const three = host.queryRadiance(scene, rays, seeds, { nsamples: 3, maxDepth: 8, rr: meta[45], accum: f32(out + '/init.f32') });
    const one = host.queryRadiance(scene, rays, seeds, { maxDepth: 8, rr: meta[45] });
    const cs = host.cameraSeeds(scene, meta, 3), win = host.cameraSeeds(scene, meta, 3, [5, 3, 19, 7]);
    const none = host.queryRadiance(scene, new Float32Array(0), new Uint32Array(0));
    const unit = host.unitRays([0, 0, 0, 1, 2, 3], [3e20, -4e20, 0, 1e-20, 2e-20, -2e-20]);
    let err = '';
    try { host.queryRadiance(scene, rays, seeds.subarray(1)); } catch (e) { err = String(e.message); }
    let derr = '';
    try { host.queryRadiance(scene, rays, seeds, { maxDepth: -1 }); } catch (e) { derr = String(e.message); }
    save('three.bin', three); save('one.bin', one); save('cs.bin', cs); save('win.bin', win); save('unit.bin', unit);
    console.log(JSON.stringify({ three: three.constructor.name, cs: cs.constructor.name, none: none.length, err, derr }));
} finally {
    pt.sceneDestroy(scene);
}
"""

INI_TEXT = """[IO]
    scene = /scene_assets/CornellBox.xml
    output = out/equirect.png

[Settings]
    imageWidth = 64
    imageHeight = 32
    samplesPerPixel = 4
    pathContinuationProb = 0.9
    directLightingOnly = false
    numDirectLightingSamples = 1
"""


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("radiance_ref"))


def test_addon_equals_the_python_binding(packed, ptopts, ref):
    scene = "CornellBox"
    p, fam = packed[scene], rr.family(scene, packed, "mixed")
    meta = p.meta_for(40, 24)
    init = rr.initial_accum()
    with tempfile.TemporaryDirectory() as td:
        fam.rays.tofile(os.path.join(td, "rays.f32"))
        fam.seeds.tofile(os.path.join(td, "seeds.u32"))
        init.tofile(os.path.join(td, "init.f32"))
        meta.astype(F).tofile(os.path.join(td, "meta.f32"))
        js = os.path.join(td, "q.js")
        with open(js, "w") as f:
            f.write(JS)
        r = subprocess.run(["node", js, os.path.join(PKG, "node"), p.dir, td], check=True, capture_output=True, text=True,
                           timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        three, one = (np.fromfile(os.path.join(td, n), F).reshape(-1, 3) for n in ("three.bin", "one.bin"))
        cs, win = (np.fromfile(os.path.join(td, n), np.uint32) for n in ("cs.bin", "win.bin"))
        unit = np.fromfile(os.path.join(td, "unit.bin"), F).reshape(-1, 8)
    assert info["three"] == "Float32Array" and info["cs"] == "Uint32Array" and info["none"] == 0
    assert "queryRadiance(scene, Float32Array rays[8n], Uint32Array seeds[n]" in info["err"]
    assert "max_depth" in info["derr"]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        py_three = s.query_radiance(fam.rays, fam.seeds, 3, 8, float(meta[45]), out=init)
        py_one = s.query_radiance(fam.rays, fam.seeds, 1, 8, float(meta[45]))
        py_cs, py_win = s.camera_seeds(meta, frame=3), s.camera_seeds(meta, window=(5, 3, 19, 7), frame=3)
    assert three.tobytes() == py_three.tobytes() and one.tobytes() == py_one.tobytes()
    assert cs.tobytes() == py_cs.tobytes() and win.tobytes() == py_win.tobytes()
    want = rr.reference(ref, scene, packed, "mixed", 3, init=True)[0]
    assert same_bits(three, want), mismatch_report(three, want)
    assert (one > 0).any()
    py_unit = pt_amd.unit_rays([(0, 0, 0), (1, 2, 3)], [(3e20, -4e20, 0), (1e-20, 2e-20, -2e-20)])
    assert rr.admitted(unit).all() and np.allclose(unit[:, 4:7], py_unit[:, 4:7], rtol=0, atol=2e-7)
    assert np.array_equal(unit[:, :4], py_unit[:, :4])


def test_pt_render_cli_equirect(packed, ptopts, ref):
    """The dumped rays are the documented ones (pixel centres on the sphere about the camera, unit, seeds
    hash1u(hash1u(i * 16787))), the accumulator is the reference's on them, the PNG is its tone map."""
    with tempfile.TemporaryDirectory() as td:
        ini = os.path.join(td, "equirect.ini")
        with open(ini, "w") as f:
            f.write(INI_TEXT)
        ps = pt_amd.load_scene(ini, web_root=SCENES)
        rays_f, acc_f = os.path.join(td, "rays.bin"), os.path.join(td, "accum.bin")
        r = subprocess.run(["node", os.path.join(PKG, "node", "bin", "pt-render.js"), ini, "--web-root", SCENES, "--out-root", td,
                            "--projection", "equirect", "--max-depth", "8", "--dump-rays", rays_f, "--dump-accum", acc_f],
                           check=True, capture_output=True, text=True, timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        W, H, n = 64, 32, 64 * 32
        raw = np.fromfile(rays_f, np.uint8)
        rays, seeds = raw[:32 * n].view(F).reshape(n, 8), raw[32 * n:].view(np.uint32)
        acc = np.fromfile(acc_f, F).reshape(n, 3)
        with open(os.path.join(td, "out", "equirect.png"), "rb") as f:
            png = f.read()
        bad = subprocess.run(["node", os.path.join(PKG, "node", "bin", "pt-render.js"), ini, "--web-root", SCENES,
                              "--projection", "fisheye"], capture_output=True, text=True, timeout=120)
    assert (info["projection"], info["width"], info["height"], info["spp"]) == ("equirect", W, H, 4)
    assert bad.returncode == 2 and "--projection" in bad.stderr
    assert seeds.shape == (n,) and rr.admitted(rays).all()
    m = np.asarray(ps.meta, np.float64)
    M, P = m[28:44], m[4:7]
    R, U, L = M[0:3], M[4:7], -M[8:11]
    y, x = np.divmod(np.arange(n), W)
    phi, th = ((x + 0.5) / W - 0.5) * 2 * np.pi, (0.5 - (y + 0.5) / H) * np.pi
    d = np.cos(th)[:, None] * (np.sin(phi)[:, None] * R + np.cos(phi)[:, None] * L) + np.sin(th)[:, None] * U
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert np.allclose(rays[:, 4:7], d, rtol=0, atol=3e-7) and np.array_equal(rays[:, 0:3], np.tile(P.astype(F), (n, 1)))
    assert np.isposinf(rays[:, 3]).all()
    assert seeds.tolist() == [oracle.hash1u(oracle.hash1u((i * 16787) & 0xFFFFFFFF)) for i in range(n)]
    want, adm, _, _ = rr.radiance(ref, ps, rays, seeds, 4, 8, float(ps.meta[45]), ps.meta[46] > 0)
    assert adm.all() and same_bits(acc, want), mismatch_report(acc, want)
    # not black: the camera stands 2.6 in front of the box's 2 x 2 opening, which fills about 0.5 of the
    # sphere's 4 pi steradians (4 %); at least a quarter of that gathers light
    assert float((acc > 0).any(axis=1).mean()) >= 0.01
    rgba = pt_amd.tonemap(acc.reshape(H, W, 3), 4)
    image = np.asarray(Image.open(io.BytesIO(png)).convert("RGBA"))
    assert np.array_equal(image, np.asarray(rgba).reshape(H, W, 4))
