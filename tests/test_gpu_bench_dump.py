"""bench.py as a program on the GPU: a plain run prints the headline line only (the roofline, the
GPU state and the CPU baseline are behind --full), and --dump-outputs writes the accumulator of the
last timed step, which is the C oracle's render of the same workload bit for bit (so the dump of
two builds can be compared value for value)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import bench
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH = 72, 40, 6, 8  # a small image, not a multiple of the 64-lane wave in either direction


def test_plain_run_line_and_dump(tmp_path):
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--width", str(W), "--height", str(H), "--spp", str(SPP), "--depth", str(DEPTH),
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = lines[0]
    assert out["metric"] == bench.metric_name("CornellBox", W, H, DEPTH) and out["unit"] == "Msamples/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["steps"] == 3 and out["warmup"] == 1
    # value = samples per step / ms_per_step; both are printed rounded to 3 decimals
    assert out["ms_per_step"] > 0 and out["value"] > 0
    rel = 0.0005 / out["ms_per_step"] + 0.0005 / out["value"] + 1e-6
    assert out["value"] == pytest.approx(W * H * SPP / out["ms_per_step"] / 1e3, rel=rel)
    assert not {"roofline", "gpu_state", "cpu_baseline"} & set(out)  # --full only

    assert os.listdir(d) == ["accumulator.npy"]
    got = np.load(d / "accumulator.npy")
    assert got.dtype == np.float32 and got.shape == (H, W, 3)
    with tempfile.TemporaryDirectory() as td:
        tri, bvh, meta = bench.pack_scene("CornellBox", td, W, H, SPP)
    ref, _ = oracle.render(tri, bvh, meta, 0, SPP, 1, DEPTH)
    bad = np.argwhere(got.view(np.uint32) != np.ascontiguousarray(ref, np.float32).view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} values differ from the oracle, first {bad[:4].tolist()}"
    assert float(got.mean()) > 0.0
