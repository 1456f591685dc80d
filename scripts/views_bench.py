#!/usr/bin/env python3
"""What a view list buys (profiles/views_bench.jsonl): the same N views of w x h pixels and F
frames rendered two ways on one build,

  list    one render_views_async call (pt_render_views_async)
  calls   N render_window_async calls queued on one stream into the same places of the atlas — the entry point
          that exists without the list, and therefore the yardstick

The N cameras stand on a turntable: the scene's own position rotated about the axis through its focus along its
up, step 0 the scene's camera (pt-render.js --turntable's rule); view v renders frames v * F .. v * F + F - 1.  Both
ways leave the same bytes in the atlas (atlas_sha256 of the two figures of a row agree).

Without --way the script runs every configuration (or --config NAME) both ways, ONE PROCESS PER FIGURE, and prints
one JSON line per configuration: per way the median of --runs calls after --warmup calls (wall clock around the
call(s) and a stream synchronisation), the spread max - min and every run, then calls / list.  With --way it is
that one process and prints its figure.

  --way profile   one view of the configuration's total paths (N w h F) under a thin lens, as a one-view list and as
                  set_camera + render_window_async: the generate kernels' busy time and share of the kernels' busy
                  time from pt_profile_read (k_wf_generate_views against k_wf_generate_cam, same slot count)

  python scripts/views_bench.py >> profiles/views_bench.jsonl
"""
import argparse
import hashlib
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# name -> (scene, N, w, h, F)
CONFIGS = {
    "cornell_cube6_128": ("CornellBox", 6, 128, 128, 16),
    "cornell_thumbs64_128": ("CornellBox", 64, 128, 128, 4),
    "cornell_pair2_1024": ("CornellBox", 2, 1024, 1024, 16),
    "glossy_thumbs64_128": ("CornellBox-Glossy", 64, 128, 128, 4),
    "glossy_cube6_256": ("CornellBox-Glossy", 6, 256, 256, 16),
    "boat_sheet16_240x135": ("MedievalBoat", 16, 240, 135, 4),
}
SETTINGS = {"samplesPerPixel": 16, "pathContinuationProb": 0.9, "directLightingOnly": False}


def turntable(cam, n):
    """n camera dicts: cam's position rotated about the axis through its focus along its up, in n equal steps."""
    P, C, U = (np.asarray(cam[k], np.float64) for k in ("pos", "focus", "up"))
    k, r = U / np.linalg.norm(U), P - C
    out = []
    for s in range(n):
        th = 2 * math.pi * s / n
        p = C + r * math.cos(th) + np.cross(k, r) * math.sin(th) + k * np.dot(k, r) * (1 - math.cos(th))
        out.append(dict(cam, pos=[float(v) for v in (P if s == 0 else p)]))
    return out


def scene_camera(scene):
    import scene_oracle as so
    with open(os.path.join(ROOT, "scenes", "scene_assets", scene + ".xml")) as f:
        x = so.load_scene_xml(f.read())[0]
    return {k: (list(x[k]) if k != "heightangle" else x[k]) for k in ("pos", "focus", "up", "heightangle")}


def figure(a):
    import scene_oracle as so
    sys.path.insert(0, a.pkg)
    import torch

    import pt_amd

    scene, n, w, h, frames = CONFIGS[a.config]
    ps = pt_amd.load_scene(os.path.join(ROOT, "scenes", "scene_assets", scene + ".xml"), width=w, height=h)
    cams = turntable(scene_camera(scene), n)
    st = torch.cuda.Stream()
    out = {"config": a.config, "way": a.way, "scene": scene, "views": n, "w": w, "h": h, "frames": frames, "depth": a.depth}
    with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
        if a.way == "profile":
            # one view of all the paths: a w x (h n) image of the scene's camera, thin lens
            W, H, cam = w, h * n, ("thin_lens", 0.05, 3.6)
            meta = so.make_meta([W, H], cams[0], SETTINGS)
            buf = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            view = [{"meta": meta, "camera": cam, "dst": (0, 0), "frame0": 0}]
            for name in ("views", "lens"):
                s.set_camera(*(cam if name == "lens" else ("pinhole",)))
                for k in range(a.warmup + 1):
                    if k == a.warmup:
                        s.profile_enable(True)
                    if name == "views":
                        s.render_views_async(view, frames, 1, a.depth, pt_amd.MODE_AUTO, buf.data_ptr(), atlas=(W, H),
                                             stream_ptr=st.cuda_stream)
                    else:
                        s.render_async(meta, 0, frames, 1, a.depth, pt_amd.MODE_AUTO, buf.data_ptr(), stream_ptr=st.cuda_stream)
                    st.synchronize()
                prof = s.profile_read()
                s.profile_enable(False)
                busy = sum(v["busy_ms"] for v in prof.values())
                out[name] = {"generate_busy_ms": prof["k_wf_generate"]["busy_ms"], "kernels_busy_ms": busy,
                             "generate_share": prof["k_wf_generate"]["busy_ms"] / busy,
                             "generate_launches": prof["k_wf_generate"]["launches"]}
            out["paths"] = W * H * frames
            s.check()
            return out
        metas = [so.make_meta([w, h], c, SETTINGS) for c in cams]
        dsts, (aw, ah) = pt_amd.view_atlas([(w, h)] * n)
        views = [{"meta": m, "dst": d, "frame0": v * frames} for v, (m, d) in enumerate(zip(metas, dsts))]
        atlas = torch.zeros((ah, aw, 3), dtype=torch.float32, device="cuda")
        base = atlas.data_ptr()
        torch.cuda.synchronize()

        def call():
            if a.way == "list":
                s.render_views_async(views, frames, 1, a.depth, pt_amd.MODE_AUTO, base, atlas=(aw, ah), stream_ptr=st.cuda_stream)
            else:
                for v in views:
                    x, y = v["dst"]
                    s.render_window_async(v["meta"], (0, 0, w, h), v["frame0"], frames, 1, a.depth, pt_amd.MODE_AUTO,
                                          base + 12 * (y * aw + x), row_pitch=aw, stream_ptr=st.cuda_stream)
            st.synchronize()

        for _ in range(a.warmup):
            call()
        atlas.zero_()
        torch.cuda.synchronize()
        call()
        out["atlas_sha256"] = hashlib.sha256(atlas.cpu().numpy().tobytes()).hexdigest()[:16]
        runs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            call()
            runs.append((time.perf_counter() - t0) * 1e3)
        s.check()
    out.update(median_ms=statistics.median(runs), spread_ms=max(runs) - min(runs), runs_ms=[round(r, 4) for r in runs],
               mpaths_per_s=n * w * h * frames / statistics.median(runs) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=list(CONFIGS))
    ap.add_argument("--way", choices=["list", "calls", "profile"])
    ap.add_argument("--depth", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", action="store_true", help="without --way: add the --way profile figure to every line")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "brown-cs2240-path-tracer_amd"))
    a = ap.parse_args()
    if a.way:
        if not a.config:
            ap.error("--way needs --config")
        print(json.dumps(figure(a)), flush=True)
        return
    for name in ([a.config] if a.config else list(CONFIGS)):
        line = {"config": name}
        for way in ["list", "calls"] + (["profile"] if a.profile else []):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", name, "--way", way, "--depth", str(a.depth),
                                "--runs", str(a.runs), "--warmup", str(a.warmup), "--pkg", a.pkg],
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:  # a failed figure ends the run: nothing more is started on the device
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{name} --way {way} failed with exit status {r.returncode}")
            line[way] = json.loads(r.stdout.strip().splitlines()[-1])
        for k in ("scene", "views", "w", "h", "frames", "depth"):
            line[k] = line["list"][k]
        line["same_bytes"] = line["list"]["atlas_sha256"] == line["calls"]["atlas_sha256"]
        line["calls_over_list"] = line["calls"]["median_ms"] / line["list"]["median_ms"]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
