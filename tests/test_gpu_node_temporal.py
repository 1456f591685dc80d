"""GPU: temporal accumulation through the Node host.  The N-API calls (reproject, denoiseMean, historyCreate,
historyStep, historyReset, historyDestroy) give the Python binding's bytes, and pt-render.js --turntable 4
--temporal writes a contact sheet whose tiles are History.step's rgba for the same cameras and frames."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cam_cases as cc
import pt_amd
from conftest import PKG, SCENES
from test_gpu_temporal import DEPTH, FF, H, N, SEQUENCES, W, render_inputs

pytestmark = pytest.mark.gpu

F = np.float32
RENDER_JS = os.path.join(PKG, "node", "bin", "pt-render.js")
PARAMS = dict(alpha=0.3, normal_min=0.8, depth_tol=0.2, max_history=8.0)
JS = r"""
const fs = require('fs');
const host = require(process.argv[2]);
const [dir, out] = [process.argv[3], process.argv[4]];
const raw = (p) => { const b = fs.readFileSync(p); const a = new Uint8Array(b.length); a.set(b); return a.buffer; };
const f32 = (p) => new Float32Array(raw(p));
const put = (name, ta) => fs.writeFileSync(out + '/' + name, Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength));
const spec = JSON.parse(fs.readFileSync(out + '/spec.json', 'utf8'));
const pt = host.native();
const scene = pt.sceneCreate(f32(dir + '/triangle_data.f32'), f32(dir + '/bvh_data.f32'), 0);
let history = null;
try {
    const metas = f32(out + '/metas.f32');
    const params = { alpha: spec.params.alpha, normalMin: spec.params.normal_min, depthTol: spec.params.depth_tol, maxHistory: spec.params.max_history };
    let prev = null;
    for (let k = 0; k < spec.steps; ++k) {
        const meta = metas.slice(48 * k, 48 * k + 48);
        const step = { accum: f32(`${out}/acc${k}.f32`), m2: f32(`${out}/m2${k}.f32`), n: spec.n, geo: f32(`${out}/geo${k}.f32`),
                       alb: f32(`${out}/alb${k}.f32`), meta };
        prev = host.reproject(scene, step, prev, params);
        for (const key of ['hist', 'mom', 'gbuf', 'out', 'var']) put(`r${k}_${key}.f32`, prev[key]);
        const d = host.denoiseMean(scene, prev.out, prev.var, spec.w, spec.h, step.geo, step.alb, { featureFrames: spec.ff, iters: 2 });
        put(`d${k}_out.f32`, d.out);
        put(`d${k}_var.f32`, d.var);
    }
    history = host.historyCreate(scene, spec.w, spec.h);
    const run = (k, tag, denoise) => {
        const r = host.historyStep(history, metas.slice(48 * k, 48 * k + 48), { frame0: k * spec.n, nframes: spec.n, maxDepth: spec.depth,
            featureFrames: spec.ff, params, denoise });
        for (const key of ['mean', 'var', 'rgba', 'historyLen']) put(`${tag}${k}_${key}.bin`, r[key]);
    };
    for (let k = 0; k < spec.steps; ++k) run(k, 'h', { iters: 2 });
    host.historyReset(history);
    run(0, 'z', null);
    let refused = '';
    try { host.reproject(scene, { accum: new Float32Array(3), m2: new Float32Array(3), n: 1, geo: new Float32Array(4), alb: new Float32Array(4), meta: metas.slice(0, 48) }); }
    catch (e) { refused = String(e.message); }
    let badParams = '';
    try { host.historyStep(history, metas.slice(0, 48), { nframes: spec.n, params: { alpha: 2 } }); } catch (e) { badParams = String(e.message); }
    host.historyDestroy(history);
    let destroyed = '';
    try { host.historyReset(history); } catch (e) { destroyed = String(e.message); }
    history = null;
    console.log(JSON.stringify({ refused, badParams, destroyed, listed: Object.keys(pt).includes('historyStep') }));
} finally {
    if (history) host.historyDestroy(history);
    pt.sceneDestroy(scene);
}
"""
META_JS = r"""
const fs = require('fs');
const host = require(process.argv[2]);
const s = host.load_scene_from_ini(process.argv[3], { web_root: process.argv[4], quiet: true });
const cams = host.turntable_cameras(s.camera_data, +process.argv[6]);
const metas = new Float32Array(48 * cams.length);
cams.forEach((c, k) => metas.set(host.make_meta(s.screenDimension, c, s.scene_description, 0), 48 * k));
fs.writeFileSync(process.argv[5], Buffer.from(metas.buffer));
"""
INI_TEXT = """[IO]
    scene = /scene_assets/CornellBox.xml
    output = out/temporal.png

[Settings]
    imageWidth = %d
    imageHeight = %d
    samplesPerPixel = %d
    pathContinuationProb = 0.9
    directLightingOnly = false
    numDirectLightingSamples = 1
"""


def test_addon_equals_the_python_binding(packed, ptopts):
    p = packed["CornellBox"]
    metas = [cc.meta_from(c, W, H) for c in SEQUENCES["yaw"]]
    spec = dict(w=W, h=H, n=N, ff=FF, depth=DEPTH, steps=len(metas), params=PARAMS)
    with tempfile.TemporaryDirectory() as td, pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        np.concatenate(metas).astype(F).tofile(os.path.join(td, "metas.f32"))
        with open(os.path.join(td, "spec.json"), "w") as f:
            json.dump(spec, f)
        want, prev = [], None
        for k, meta in enumerate(metas):
            acc, m2, geo, alb = render_inputs(s, meta, k)
            for name, a in (("acc", acc), ("m2", m2), ("geo", geo), ("alb", alb)):
                a.tofile(os.path.join(td, f"{name}{k}.f32"))
            prev = s.reproject(acc, m2, N, geo, alb, meta, prev=prev, params=PARAMS)
            want.append((prev, s.denoise_mean(prev["out"], prev["var"], geo, alb, FF, params=dict(iters=2))))
        with pt_amd.History(s, W, H) as hist:
            hsteps = [hist.step(meta, k * N, N, 1, DEPTH, feature_frames=FF, params=PARAMS, denoise=dict(iters=2))
                      for k, meta in enumerate(metas)]
            hist.reset()
            first = hist.step(metas[0], 0, N, 1, DEPTH, feature_frames=FF, params=PARAMS)
        js = os.path.join(td, "temporal.js")
        with open(js, "w") as f:
            f.write(JS)
        r = subprocess.run(["node", js, os.path.join(PKG, "node"), p.dir, td], check=True, capture_output=True, text=True, timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        read = lambda name: open(os.path.join(td, name), "rb").read()  # noqa: E731
        for k, (rp, dn) in enumerate(want):
            for key in ("hist", "mom", "gbuf", "out", "var"):
                assert read(f"r{k}_{key}.f32") == rp[key].tobytes(), (k, key)
            assert read(f"d{k}_out.f32") == dn[0].tobytes() and read(f"d{k}_var.f32") == dn[1].tobytes(), k
        for tag, steps in (("h", hsteps), ("z", [first])):
            for k, st in enumerate(steps):
                for key, name in (("mean", "mean"), ("var", "var"), ("rgba", "rgba"), ("history_len", "historyLen")):
                    assert read(f"{tag}{k}_{name}.bin") == st[key].tobytes(), (tag, k, key)
    assert want[2][0]["hist"][..., 3].max() == 3 and hsteps[2]["rgba"][..., :3].max() > 0
    assert "reproject(scene" in info["refused"] and "alpha" in info["badParams"] and "destroyed" in info["destroyed"]
    assert not info["listed"]


@pytest.mark.parametrize("extra", [[], ["0.5", "--denoise", "2", "--feature-frames", "2"]], ids=["plain", "alpha-denoise"])
def test_pt_render_cli_turntable_temporal(packed, ptopts, extra):
    from PIL import Image
    w, h, spp, n = 40, 24, 2, 4
    with tempfile.TemporaryDirectory() as td:
        ini = os.path.join(td, "temporal.ini")
        with open(ini, "w") as f:
            f.write(INI_TEXT % (w, h, spp))
        r = subprocess.run(["node", RENDER_JS, ini, "--web-root", SCENES, "--out-root", td, "--max-depth", str(DEPTH), "--turntable",
                            str(n), "--temporal"] + extra, check=True, capture_output=True, text=True, timeout=300)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        img = np.array(Image.open(info["output"]))
        js, mf = os.path.join(td, "metas.js"), os.path.join(td, "metas.f32")
        with open(js, "w") as f:
            f.write(META_JS)
        subprocess.run(["node", js, os.path.join(PKG, "node"), ini, SCENES, mf, str(n)], check=True, capture_output=True, timeout=120)
        metas = np.fromfile(mf, F).reshape(n, 48)
        ps = pt_amd.load_scene(ini, web_root=SCENES)
    assert (info["width"], info["height"], info["turntable"], info["tile"], info["spp"]) == (2 * w, 2 * h, n, [w, h], spp)
    assert info["dsts"] == [[0, 0], [w, 0], [0, h], [w, h]]
    assert img.shape == (2 * h, 2 * w, 4)
    ff = 2
    with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s, pt_amd.History(s, w, h) as hist:
        steps = [hist.step(metas[k], k * spp, spp, 1, DEPTH, feature_frames=ff, params=dict(alpha=0.5) if extra else None,
                           denoise=dict(iters=2) if extra else None) for k in range(n)]
        raw = s.render_image(metas[0], 0, spp, 1, DEPTH)
    assert np.array_equal(metas[0], ps.meta)  # step 0 is the scene's camera
    for k, (x, y) in enumerate(info["dsts"]):
        assert np.ascontiguousarray(img[y:y + h, x:x + w]).tobytes() == steps[k]["rgba"].tobytes(), k
    print("longest history per view:", [float(st["history_len"].max()) for st in steps])
    if not extra:  # a first step is the plain image of its frames
        assert steps[0]["rgba"].tobytes() == raw.tobytes()
