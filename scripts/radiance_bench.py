#!/usr/bin/env python3
"""Paths per second of pt_query_radiance_async against the render route it shares (profiles/radiance_bench.jsonl;
DESIGN.md §5.11).  One process measures one of

  --what query    pt_query_radiance_async on the image's frame-0 camera rays and seeds (pt_camera_rays_async,
                  pt_camera_seeds_async), --samples samples per ray, all from device buffers
  --what render   pt_render_async of the same number of frames with option fuse_gen = 0: camera paths from
                  k_wf_generate, the route the query's k_wf_generate_rays replaces (run it with --pkg pointing at
                  the parent commit's package for the comparison DESIGN.md records)

and prints one JSON line: ms per call (median of --runs after one warm-up call, the spread max - min and every
run; wall clock around the call and a stream synchronisation), Mpaths/s = width * height * samples / median, and
from a further profiled call (pt_profile_read) the generate kernel's share of the kernels' busy time.

  python scripts/radiance_bench.py --what query --scene CornellBox --width 1024 --height 1024 --samples 16
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=["query", "render"], required=True)
    ap.add_argument("--scene", default="CornellBox", help="a scene of scenes/scene_assets (without .xml)")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "brown-cs2240-path-tracer_amd"))
    a = ap.parse_args()

    sys.path.insert(0, a.pkg)
    import torch

    import pt_amd

    ps = pt_amd.load_scene(os.path.join(ROOT, "scenes", "scene_assets", a.scene + ".xml"), width=a.width, height=a.height)
    meta, n = ps.meta, a.width * a.height
    st = torch.cuda.Stream()
    d_acc = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
        if a.what == "query":
            d_rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
            d_seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            s.camera_rays_async(meta, 0, d_rays.data_ptr(), stream_ptr=st.cuda_stream)
            s.camera_seeds_async(meta, 0, d_seeds.data_ptr(), stream_ptr=st.cuda_stream)

            def call():
                s.query_radiance_async(d_rays.data_ptr(), d_seeds.data_ptr(), n, d_acc.data_ptr(), a.samples, a.depth,
                                       float(meta[45]), bool(meta[46] > 0), stream_ptr=st.cuda_stream)
        else:
            pt_amd.set_option("fuse_gen", 0)
            torch.cuda.synchronize()

            def call():
                s.render_async(meta, 0, a.samples, 1, a.depth, pt_amd.MODE_AUTO, d_acc.data_ptr(), stream_ptr=st.cuda_stream)
        st.synchronize()
        call()
        st.synchronize()
        ms = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            call()
            st.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        s.check()
        s.profile_enable(True)
        call()
        st.synchronize()
        prof = s.profile_read()
        s.profile_enable(False)
    busy = {k: v["busy_ms"] for k, v in prof.items()}
    med = statistics.median(ms)
    print(json.dumps({"what": a.what, "label": a.label, "scene": a.scene, "width": a.width, "height": a.height,
                      "samples": a.samples, "depth": a.depth, "ms_median": med, "ms_spread": max(ms) - min(ms), "ms_runs": ms,
                      "mpaths_per_s": n * a.samples / med / 1e3, "kernel_busy_ms": busy,
                      "generate_share": busy.get("k_wf_generate", 0.0) / max(sum(busy.values()), 1e-9),
                      "accum_mean": float(d_acc.mean().item()), "build_id": pt_amd.build_id()}))


if __name__ == "__main__":
    main()
