#!/usr/bin/env python3
"""What temporal accumulation costs (profiles/temporal_bench.jsonl): one JSON line per process
with
  * reproject_ms            k_reproject from pt_profile_read (HIP events around the launch) inside a history step
                            with a previous set (the second and later steps of a camera path: four taps per pixel),
                            and reproject_first_ms, the first step's (no taps),
  * step_ms / step_filtered_ms   a whole pt_history_step on the host's clock — the --frames-frame moments render, the
                            guide pass, k_reproject, [the a-trous filter,] the tone map and the copy of the RGBA image —
                            with the cameras alternating between two poses a --degrees turn apart,
  * render_ms_per_frame     the yardstick: two HIP events around a plain 16-frame render of the same image into a
                            device buffer, per frame (render_wall_ms_per_frame: the host's clock around the same call
                            and a synchronisation),
  * equivalent_frames_*     reproject_ms, and what a step adds to its own frames' render (step_ms - frames *
                            render_wall_ms_per_frame), in frames of this scene,
  * hbm_gbps, hbm_fraction  by the traffic model of 168 B per pixel (56 B of current inputs, 48 B of previous
                            planes — the four taps of a pixel and of its neighbours share lines —, 64 B written)
                            against --hbm-tbps (6.3: what a float4 copy attains on an MI355X).
The variants alternate inside a run (--runs runs: the median and every run); take three processes.

  python scripts/temporal_bench.py --scene CornellBox --size 1024
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES_PER_PIXEL = 56 + 48 + 64


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="CornellBox", help="a scene of scenes/scene_assets (without .xml)")
    ap.add_argument("--size", type=int, default=1024, help="the image is size x size")
    ap.add_argument("--frames", type=int, default=2, help="frames of a step's moments render")
    ap.add_argument("--feature-frames", type=int, default=2)
    ap.add_argument("--yardstick-frames", type=int, default=16)
    ap.add_argument("--degrees", type=float, default=2.0, help="the turn between the two alternating cameras")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    ap.add_argument("--label", default="")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "brown-cs2240-path-tracer_amd"))
    a = ap.parse_args()

    sys.path.insert(0, a.pkg)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch

    import pt_amd
    import scene_oracle as so

    xml = os.path.join(ROOT, "scenes", "scene_assets", a.scene + ".xml")
    packed = pt_amd.load_scene(xml, width=a.size, height=a.size)
    W = H = a.size
    npix = W * H
    with open(xml) as f:
        cam = so.load_scene_xml(f.read())[0]
    settings = {"samplesPerPixel": 16, "pathContinuationProb": 0.9, "directLightingOnly": False}

    def turned(deg):  # the scene's camera moved about its focus, about its up axis (y in these scenes)
        p, c, t = np.array(cam["pos"], float), np.array(cam["focus"], float), math.radians(deg)
        d = p - c
        q = c + np.array([d[0] * math.cos(t) + d[2] * math.sin(t), d[1], -d[0] * math.sin(t) + d[2] * math.cos(t)])
        return so.make_meta([W, H], {"pos": list(q), "focus": list(c), "up": list(cam["up"]), "heightangle": cam["heightangle"]},
                            settings)

    metas = [np.asarray(turned(0.0), np.float32), np.asarray(turned(a.degrees), np.float32)]
    lib = pt_amd.load_library()
    rgba = np.zeros((H, W, 4), np.uint8)
    dn = pt_amd.denoise_defaults()

    with pt_amd.Scene(packed.triangle_data, packed.bvh_data) as s, pt_amd.History(s, W, H) as hist:
        state = {"k": 0}

        def step(filtered):
            k = state["k"]
            state["k"] = k + 1
            m = metas[k & 1]
            rc = lib.pt_history_step(hist._h, m.ctypes.data_as(ctypes.c_void_p), (k * a.frames) % (1 << 20), a.frames, 1, a.depth,
                                     pt_amd.MODE_AUTO, a.feature_frames, None, ctypes.byref(dn) if filtered else None, None, None,
                                     rgba.ctypes.data_as(ctypes.c_void_p), None, None)
            if rc:
                raise RuntimeError(lib.pt_last_error().decode())

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        def kernel_ms(fn, name):
            s.profile_enable(True)
            fn()
            t = s.profile_read()
            s.profile_enable(False)
            assert t[name]["launches"] == 1
            return t[name]["total_ms"]

        scratch = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")

        def render():
            scratch.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            s.render_async(metas[0], 0, a.yardstick_frames, 1, a.depth, pt_amd.MODE_AUTO, scratch.data_ptr())
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.yardstick_frames, (time.perf_counter() - t0) * 1e3 / a.yardstick_frames

        for filtered in (False, True, False):  # warm-up of every kernel
            step(filtered)
        render()
        rp, rp_first, st, stf, rd, rdw = [], [], [], [], [], []
        for _ in range(a.runs):  # the variants alternate
            rp.append(kernel_ms(lambda: step(False), "k_reproject"))
            st.append(timed(lambda: step(False)))
            stf.append(timed(lambda: step(True)))
            ev, wall = render()
            rd.append(ev)
            rdw.append(wall)
            hist.reset()
            rp_first.append(kernel_ms(lambda: step(False), "k_reproject"))
            step(False)
        s.check()
        lit = float((rgba[..., :3].max(axis=2) > 0).mean())

    med = statistics.median
    r_ms, model_ms = med(rp), BYTES_PER_PIXEL * npix / (a.hbm_tbps * 1e12) * 1e3
    line = {
        "label": a.label, "scene": a.scene, "image": f"{W}x{H}", "depth": a.depth, "frames": a.frames,
        "feature_frames": a.feature_frames, "degrees": a.degrees, "runs": a.runs,
        "reproject_ms": r_ms, "reproject_ms_runs": rp, "reproject_first_ms": med(rp_first), "reproject_first_ms_runs": rp_first,
        "step_ms": med(st), "step_ms_runs": st, "step_filtered_ms": med(stf), "step_filtered_ms_runs": stf,
        "render_ms_per_frame": med(rd), "render_ms_per_frame_runs": rd,
        "render_wall_ms_per_frame": med(rdw), "render_wall_ms_per_frame_runs": rdw,
        "equivalent_frames_reproject": r_ms / med(rd),
        "equivalent_frames_step_overhead": (med(st) - a.frames * med(rdw)) / med(rdw),
        "equivalent_frames_step_filtered_overhead": (med(stf) - a.frames * med(rdw)) / med(rdw),
        "model_bytes": BYTES_PER_PIXEL * npix, "model_ms": model_ms, "hbm_gbps": BYTES_PER_PIXEL * npix / (r_ms * 1e-3) / 1e9,
        "hbm_fraction": model_ms / r_ms, "lit_fraction_last_image": lit,
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
