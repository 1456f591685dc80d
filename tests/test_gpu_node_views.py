"""GPU: view-list renders through the Node host.  renderViews of the N-API addon (through node/index.js)
returns the bytes of the Python binding on the shared view sets (and so the reference's, test_gpu_views.py);
pt-render.js --turntable 4 --counters 1 writes a contact sheet whose first tile is the plain render and
whose tiles all see light; the combinations it refuses exit with the usage line."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pt_amd
import views_ref as vr
from conftest import PKG, SCENES
from test_gpu_node_radiance import INI_TEXT

pytestmark = pytest.mark.gpu

F = np.float32
RENDER_JS = os.path.join(PKG, "node", "bin", "pt-render.js")
JS = r"""
const fs = require('fs');
const host = require(process.argv[2]);
const [dir, out] = [process.argv[3], process.argv[4]];
const raw = (p) => { const b = fs.readFileSync(p); const a = new Uint8Array(b.length); a.set(b); return a.buffer; };
const f32 = (p) => new Float32Array(raw(p));
const pt = host.native();
const scene = pt.sceneCreate(f32(dir + '/triangle_data.f32'), f32(dir + '/bvh_data.f32'), 0);
(async () => {
    try {
        const spec = JSON.parse(fs.readFileSync(out + '/views.json', 'utf8'));
        const metas = f32(out + '/metas.f32');
        const views = spec.views.map((v, k) => Object.assign({}, v, { meta: metas.slice(48 * k, 48 * k + 48) }));
        pt.sceneSetCamera(scene, { model: 'ortho', focusDistance: 2 });  // not read: the views carry theirs
        const r = await host.renderViews(scene, views, { atlasW: spec.atlas[0], atlasH: spec.atlas[1], nframes: spec.nframes,
            maxDepth: spec.depth, accum: f32(out + '/init.f32'), counters: true });
        fs.writeFileSync(out + '/atlas.bin', Buffer.from(r.accum.buffer, r.accum.byteOffset, r.accum.byteLength));
        const packed = await host.renderViews(scene, views.map((v) => Object.assign({}, v, { dst: undefined })), { nframes: 1, maxDepth: spec.depth });
        let refused = '';
        try { await host.renderViews(scene, views.map((v) => Object.assign({}, v, { dst: [0, 0] })), { atlasW: spec.atlas[0], atlasH: spec.atlas[1], nframes: 1 }); }
        catch (e) { refused = String(e.message); }
        console.log(JSON.stringify({ counters: r.counters, packed: [packed.atlasW, packed.atlasH], dsts: packed.dsts, refused,
            listed: Object.keys(pt).includes('renderViews') }));
    } finally {
        pt.sceneDestroy(scene);
    }
})().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
"""
JS_MODEL = {None: None, "thin_lens": "thin_lens", "ortho": "ortho", "equirect": "equirect"}


@pytest.mark.parametrize("name", ("mixed5", "models4"))
def test_addon_equals_the_python_binding(packed, ptopts, name):
    scene, views, atlas = vr.views_of(name)
    p = packed[scene]
    init = vr.initial_atlas(atlas)
    spec = {"atlas": list(atlas), "nframes": vr.NFRAMES, "depth": vr.DEPTH, "views": [
        {"window": list(v["window"]), "dst": list(v["dst"]), "frame0": v["frame0"],
         "camera": None if v["camera"] is None else {"model": v["camera"][0], "lensRadius": v["camera"][1], "focusDistance": v["camera"][2]}}
        for v in views]}
    with tempfile.TemporaryDirectory() as td:
        np.concatenate([np.asarray(v["meta"], F) for v in views]).tofile(os.path.join(td, "metas.f32"))
        init.tofile(os.path.join(td, "init.f32"))
        with open(os.path.join(td, "views.json"), "w") as f:
            json.dump(spec, f)
        js = os.path.join(td, "views.js")
        with open(js, "w") as f:
            f.write(JS)
        r = subprocess.run(["node", js, os.path.join(PKG, "node"), p.dir, td], check=True, capture_output=True, text=True, timeout=120)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        got = np.fromfile(os.path.join(td, "atlas.bin"), F).reshape(atlas[1], atlas[0], 3)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        want, wcnt = s.render_views(views, vr.NFRAMES, 1, vr.DEPTH, atlas=atlas, accum=init.copy(), counters=True)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() != init.tobytes()
    assert info["counters"] == wcnt and not info["listed"]
    dsts, size = pt_amd.view_atlas([v["window"][2:] for v in views])
    assert info["packed"] == list(size) and info["dsts"] == [list(d) for d in dsts]  # the two packers agree
    assert "overlap" in info["refused"] and "views[0]" in info["refused"]


def test_pt_render_cli_turntable(packed, ptopts):
    """--turntable 4 --counters 1 with the accumulator dumped: a 2 x 2 sheet of 64 x 32 tiles; tile 0 is the plain
    render's dump; every tile sees light; --window, --denoise and --projection are refused with the usage line."""
    W, H, spp, n = 64, 32, 4, 4
    with tempfile.TemporaryDirectory() as td:
        ini = os.path.join(td, "turn.ini")
        with open(ini, "w") as f:
            f.write(INI_TEXT.replace("equirect.png", "turn.png"))
        sheet_f, plain_f, lens_f = (os.path.join(td, x) for x in ("sheet.bin", "plain.bin", "lens.bin"))
        base = ["node", RENDER_JS, ini, "--web-root", SCENES, "--out-root", td, "--max-depth", "8"]
        run = lambda extra, **kw: subprocess.run(base + extra, capture_output=True, text=True, timeout=120, **kw)  # noqa: E731
        r = run(["--turntable", "4", "--counters", "1", "--dump-accum", sheet_f], check=True)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        png = os.path.getsize(os.path.join(td, "out", "turn.png"))
        run(["--dump-accum", plain_f], check=True)
        row = run(["--turntable", "3,3", "--camera", "thinlens", "--aperture", "0.1", "--dump-accum", lens_f], check=True)
        row_info = json.loads(row.stdout.strip().splitlines()[-1])
        bad = [run(["--turntable", "4"] + extra) for extra in (["--window", "0,0,8,8"], ["--denoise"], ["--projection", "equirect"])]
        bad += [run(["--turntable", t]) for t in ("0", "x", "4,0", "1,2,3")]
        sheet = np.fromfile(sheet_f, F).reshape(2 * H, 2 * W, 3)
        plain = np.fromfile(plain_f, F).reshape(H, W, 3)
        lens = np.fromfile(lens_f, F).reshape(H, 3 * W, 3)
    assert png > 0 and (info["width"], info["height"], info["turntable"], info["tile"]) == (2 * W, 2 * H, n, [W, H])
    assert info["dsts"] == [[0, 0], [W, 0], [0, H], [W, H]]
    assert info["counters"]["samples"] == n * W * H * spp
    tiles = [sheet[y:y + H, x:x + W] for x, y in info["dsts"]]
    assert np.ascontiguousarray(tiles[0]).tobytes() == plain.tobytes()  # step 0 is the scene's camera
    shares = [float((t.sum(axis=2) > 0).mean()) for t in tiles]
    assert min(shares) >= 0.25, shares
    assert len({np.ascontiguousarray(t).tobytes() for t in tiles}) == n  # four different cameras
    assert (row_info["width"], row_info["height"]) == (3 * W, H) and row_info["camera"]["model"] == "thin_lens"
    assert min(float((lens[:, k * W:(k + 1) * W].sum(axis=2) > 0).mean()) for k in range(3)) >= 0.25
    for b in bad:
        assert b.returncode == 2 and "usage: pt-render.js <scene.ini> --turntable" in b.stderr, (b.returncode, b.stderr)
