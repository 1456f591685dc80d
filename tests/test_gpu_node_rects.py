"""GPU: the Node host's rectangle lists — the addon's renderRects against Python's render_rects, and
pt-render.js --window with several rectangles."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pt_amd
from conftest import PKG, SCENES
from test_gpu_rects import L1, cut, start
from test_gpu_window import DEPTH, H, W

pytestmark = pytest.mark.gpu

INI = os.path.join(SCENES, "scene_files", "final", "cornell_box_full_lighting.ini")

NODE_SCRIPT = r"""
const fs = require('fs');
const host = require(process.argv[1]);
(async () => {
    const [dir, out] = [process.argv[2], process.argv[3]];
    const f32 = (name) => { const b = fs.readFileSync(`${dir}/${name}`); return new Float32Array(b.buffer, b.byteOffset, b.length / 4).slice(); };
    const pt = host.native();
    const scene = pt.sceneCreate(f32('triangle_data.f32'), f32('bvh_data.f32'), 0);
    const meta = f32('meta.f32');
    const rects = %s;
    const result = {};
    for (const [mode, name] of [[1, 'megakernel'], [2, 'wavefront']]) {
        const accum = f32('init.f32');
        result[name] = await pt.renderRects(scene, meta, null, rects, 3, 3, 4, %d, mode, accum, true);
        fs.writeFileSync(`${out}/${name}.f32`, Buffer.from(accum.buffer));
    }
    const frame = %s, inner = %s;
    const facc = new Float32Array(frame[2] * frame[3] * 3);
    result.framed = await pt.renderRects(scene, meta, frame, inner, 3, 3, 4, %d, 0, facc, false);
    fs.writeFileSync(`${out}/framed.f32`, Buffer.from(facc.buffer));
    const bad = [];
    for (const list of [[[5, 3, 19, 7], [13, 9, 17, 11]], [[30, 20, 11, 2]]]) {
        try { await pt.renderRects(scene, meta, null, list, 0, 1, 1, 4, 0, f32('init.f32'), false); bad.push(null); }
        catch (e) { bad.push(e.message); }
    }
    const types = [];
    for (const args of [[scene, meta, null, [], 0, 1, 1, 4, 0, f32('init.f32')], [scene, meta, null, [[1, 2, 3]], 0, 1, 1, 4, 0, f32('init.f32')],
                        [scene, meta, [0, 0, 4, 4], [[0, 0, 1, 1]], 0, 1, 1, 4, 0, f32('init.f32')], [scene, meta, null]]) {
        try { pt.renderRects(...args); types.push(null); } catch (e) { types.push(e.constructor.name); }
    }
    pt.sceneDestroy(scene);
    fs.writeFileSync(out + '/result.json', JSON.stringify({ result, bad, types }));
})().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
"""


def test_render_rects_equals_python(packed):
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    init = start(W, H)
    frame, inner = (4, 2, 30, 20), [(5, 3, 19, 7), (13, 10, 17, 10)]
    with tempfile.TemporaryDirectory() as td:
        for name, a in (("triangle_data.f32", p.triangle_data), ("bvh_data.f32", p.bvh_data), ("meta.f32", meta),
                        ("init.f32", init)):
            np.asarray(a, np.float32).tofile(os.path.join(td, name))
        script = NODE_SCRIPT % (json.dumps([list(r) for r in L1]), DEPTH, json.dumps(list(frame)),
                                json.dumps([list(r) for r in inner]), DEPTH)
        subprocess.run(["node", "-e", script, os.path.join(PKG, "node"), td, td], check=True, capture_output=True, timeout=300)
        got = {n: np.fromfile(os.path.join(td, n + ".f32"), np.float32) for n in ("megakernel", "wavefront", "framed")}
        info = json.load(open(os.path.join(td, "result.json")))
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for name, mode in (("megakernel", pt_amd.MODE_MEGAKERNEL), ("wavefront", pt_amd.MODE_WAVEFRONT)):
            ref, cnt = s.render_rects(meta, L1, 3, 3, 4, DEPTH, mode, accum=init.copy(), counters=True)
            assert sum(float(cut(ref, r).sum() - cut(init, r).sum()) for r in L1) > 0  # the rectangles received light
            assert got[name].tobytes() == ref.tobytes(), name
            assert info["result"][name] == cnt
        fref = s.render_rects(meta, inner, 3, 3, 4, DEPTH, frame=frame)
    assert fref.mean() > 0 and got["framed"].tobytes() == fref.tobytes()
    assert info["result"]["framed"] is None
    assert all(m and "pt_hip error -1" in m for m in info["bad"]), info["bad"]
    assert "overlap" in info["bad"][0] and "outside" in info["bad"][1]
    assert info["types"] == ["TypeError"] * 4  # an empty list, a malformed rectangle, an accumulator of the wrong size, too few arguments


CLI = ["node", os.path.join(PKG, "node", "bin", "pt-render.js"), INI, "--web-root", SCENES, "--spp", "2", "--max-depth", "4"]


def run_cli(out_root, *extra):
    from PIL import Image
    r = subprocess.run(CLI + ["--out-root", out_root, *extra], check=True, capture_output=True, text=True, timeout=300)
    info = json.loads(r.stdout.strip().splitlines()[-1])
    return info, np.array(Image.open(info["output"]))


@pytest.fixture(scope="module")
def full_png(tmp_path_factory):
    return run_cli(str(tmp_path_factory.mktemp("full")))[1]


# under the light of the .ini's own image; then window A and its neighbour (dark there: the first pair is the one that counts)
@pytest.mark.parametrize("wins", [[(200, 40, 19, 7), (208, 50, 17, 10)], [(5, 3, 19, 7), (13, 10, 17, 10)]], ids=["lit", "A"])
def test_pt_render_cli_several_windows_png(full_png, tmp_path, wins):
    """pt-render.js --window "a;b": one renderRects call, a PNG of the image's size whose rectangles are
    the full PNG's and whose other pixels are black."""
    full = full_png
    info, img = run_cli(str(tmp_path), "--window", ";".join(",".join(map(str, w)) for w in wins))
    assert info["rects"] == [list(w) for w in wins] and info["window"] is None
    assert (info["width"], info["height"]) == (full.shape[1], full.shape[0])
    want = np.zeros_like(full)
    want[..., 3] = 255
    for x0, y0, w, h in wins:
        want[y0:y0 + h, x0:x0 + w] = full[y0:y0 + h, x0:x0 + w]
    if wins[0][0] == 200:
        assert all(full[y0:y0 + h, x0:x0 + w, :3].max() > 0 for x0, y0, w, h in wins)
    assert np.array_equal(img, want)
