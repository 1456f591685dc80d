"""GPU: the irradiance gathers through the Node host.  gather and gatherRays of the N-API addon return the
bytes of the Python binding (and so the reference's, test_gpu_gather.py) on CornellBox's points in both
modes; pt-render.js --probe prints 27 finite numbers, the scaled sums of the same call through Python, and
--irradiance three."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import gather_ref as gr
import pt_amd
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
    const meta = f32(out + '/meta.f32'), seeds = u32(out + '/seeds.u32');
    for (const mode of ['cosine', 'sh9']) {
        const points = host.gatherPoints(f32(out + '/p_' + mode + '.f32'), f32(out + '/n.f32'), seeds);
        save('points_' + mode + '.bin', points);
        const first = host.gather(scene, points, { nsamples: 2, mode, maxDepth: 8, rr: meta[45], accum: f32(out + '/init_' + mode + '.f32') });
        const three = host.gather(scene, points, { nsamples: 1, sample0: 2, mode, maxDepth: 8, rr: meta[45], accum: first });
        const r = host.gatherRays(scene, points, 1, mode);
        save('three_' + mode + '.bin', three); save('rays_' + mode + '.bin', r.rays); save('seeds_' + mode + '.bin', r.seeds);
    }
    const none = host.gather(scene, new Float32Array(0), { nsamples: 3 });
    let err = '';
    try { host.gather(scene, new Float32Array(7), { nsamples: 1 }); } catch (e) { err = String(e.message); }
    let derr = '';
    try { host.gather(scene, new Float32Array(8), { nsamples: 1, maxDepth: -1 }); } catch (e) { derr = String(e.message); }
    let merr = '';
    try { host.gather(scene, new Float32Array(8), { nsamples: 1, mode: 'sh4' }); } catch (e) { merr = String(e.message); }
    console.log(JSON.stringify({ none: none.length, err, derr, merr }));
} finally {
    pt.sceneDestroy(scene);
}
"""

INI_TEXT = """[IO]
    scene = /scene_assets/CornellBox.xml
    output = out/gather.png

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
    return gr.build(tmp_path_factory.mktemp("gather_ref"))


def test_addon_equals_the_python_binding(packed, ptopts, ref):
    scene = "CornellBox"
    p = packed[scene]
    meta = p.meta_for(40, 24)
    pts = {m: gr.points(scene, packed, m) for m in gr.MODES}
    with tempfile.TemporaryDirectory() as td:
        for m in gr.MODES:
            pts[m].p.tofile(os.path.join(td, f"p_{m}.f32"))
            gr.initial_accum(gr.N, gr.width(m)).tofile(os.path.join(td, f"init_{m}.f32"))
        pts["cosine"].n.tofile(os.path.join(td, "n.f32"))
        pts["cosine"].seeds.tofile(os.path.join(td, "seeds.u32"))
        meta.astype(F).tofile(os.path.join(td, "meta.f32"))
        js = os.path.join(td, "g.js")
        with open(js, "w") as f:
            f.write(JS)
        r = subprocess.run(["node", js, os.path.join(PKG, "node"), p.dir, td], check=True, capture_output=True, text=True,
                           timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        got = {m: {k: np.fromfile(os.path.join(td, f"{k}_{m}.bin"), np.uint32 if k == "seeds" else F)
                   for k in ("points", "three", "rays", "seeds")} for m in gr.MODES}
    assert info["none"] == 0 and "gather(scene, Float32Array points[8n]" in info["err"]
    assert "max_depth" in info["derr"] and "sh4" in info["merr"]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for m in gr.MODES:
            g, w = pts[m], gr.width(m)
            assert got[m]["points"].tobytes() == g.packed.tobytes()
            py = s.gather(g.p, g.n, g.seeds, 3, mode=m, max_depth=8, rr=float(meta[45]), out=gr.initial_accum(gr.N, w))
            py_rays, py_seeds = s.gather_rays(g.p, g.n, g.seeds, 1, m)
            three = got[m]["three"].reshape(-1, w)
            assert three.tobytes() == py.tobytes(), m
            assert got[m]["rays"].tobytes() == py_rays.tobytes() and got[m]["seeds"].tobytes() == py_seeds.tobytes(), m
            want = gr.reference(ref, scene, packed, m, 3, init=True)[0]
            assert same_bits(three, want), (m, mismatch_report(three, want))


def test_pt_render_cli_probe_and_irradiance(packed, ptopts):
    """--probe prints 27 finite numbers: 4 pi / N times the sums of the same point, seed and samples through
    the Python binding; --irradiance three, pi / N times its sums; a malformed point is a usage error."""
    cli = ["node", os.path.join(PKG, "node", "bin", "pt-render.js")]
    with tempfile.TemporaryDirectory() as td:
        ini = os.path.join(td, "gather.ini")
        with open(ini, "w") as f:
            f.write(INI_TEXT)
        ps = pt_amd.load_scene(ini, web_root=SCENES)
        base = cli + [ini, "--web-root", SCENES, "--max-depth", "8", "--samples", "64", "--seed", "7"]
        probe = subprocess.run(base + ["--probe", "0,0.5,0"], check=True, capture_output=True, text=True, timeout=120)
        irr = subprocess.run(base + ["--irradiance", "0,0,0,0,2,0"], check=True, capture_output=True, text=True, timeout=120)
        bad = subprocess.run(base + ["--probe", "0,0.5"], capture_output=True, text=True, timeout=120)
    pinfo, iinfo = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (probe, irr))
    assert bad.returncode == 2 and "--probe" in bad.stderr
    sh9, e = np.array(pinfo["sh9"], np.float64), np.array(iinfo["irradiance"], np.float64)
    assert sh9.shape == (27,) and np.isfinite(sh9).all() and pinfo["samples"] == 64
    assert e.shape == (3,) and np.isfinite(e).all()
    rrp = float(ps.meta[45])
    with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
        py9 = s.gather([(0, 0.5, 0)], None, [7], 64, mode="sh9", max_depth=8, rr=rrp)[0]
        pye = s.gather([(0, 0, 0)], [(0, 2, 0)], [7], 64, max_depth=8, rr=rrp)[0]
    assert np.array_equal(sh9, py9.astype(np.float64) * (4 * np.pi / 64))
    assert np.array_equal(e, pye.astype(np.float64) * (np.pi / 64))
    # not black: the probe floats in the middle of the lit box, so the constant term of every channel is positive
    assert (sh9[0::9] > 0).all()
