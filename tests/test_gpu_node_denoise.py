"""GPU: pt-render.js --denoise.  The PNG of a 40x24, 8-frame CornellBox with 4 feature frames holds the
bytes of Scene.render_denoised for the scene the CLI loaded, and of the reference pipeline
(test_gpu_denoise.py: the oracle's frames, the reference's guides and filter, the oracle's tone map)."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
import pt_amd
from conftest import PKG, SCENES
from test_gpu_denoise import FEATURE_FRAMES, NFRAMES, oracle_passes
from test_gpu_window import DEPTH, H, W

pytestmark = pytest.mark.gpu

INI_TEXT = """[IO]
    scene = /scene_assets/CornellBox.xml
    output = out/denoised.png

[Settings]
    imageWidth = %d
    imageHeight = %d
    samplesPerPixel = %d
    pathContinuationProb = 0.9
    directLightingOnly = false
    numDirectLightingSamples = 1
""" % (W, H, NFRAMES)


def test_pt_render_cli_denoise_png(packed, ptopts):
    from PIL import Image
    want = oracle.tonemap(oracle_passes(packed, "defaults")[3][0], 1).reshape(H, W, 4)
    with tempfile.TemporaryDirectory() as td:
        ini = os.path.join(td, "denoise.ini")
        with open(ini, "w") as f:
            f.write(INI_TEXT)
        r = subprocess.run(["node", os.path.join(PKG, "node", "bin", "pt-render.js"), ini, "--web-root", SCENES, "--out-root", td,
                            "--max-depth", str(DEPTH), "--denoise", "--feature-frames", str(FEATURE_FRAMES)],
                           check=True, capture_output=True, text=True, timeout=300)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        img = np.array(Image.open(info["output"]))
        ps = pt_amd.load_scene(ini, web_root=SCENES)
    assert (info["width"], info["height"], info["spp"]) == (W, H, NFRAMES)
    assert info["denoise"] == {"iters": 0, "featureFrames": FEATURE_FRAMES}
    with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
        same = s.render_denoised(ps.meta, 0, NFRAMES, 1, DEPTH, feature_frames=FEATURE_FRAMES)
    assert img.shape == (H, W, 4) and img[..., :3].max() > 0
    assert img.tobytes() == same.tobytes()
    assert img.tobytes() == want.tobytes()
