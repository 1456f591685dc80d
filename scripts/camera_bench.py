#!/usr/bin/env python3
"""Cost of the lens cameras (pt_scene_set_camera) against the two routes there were before them
(profiles/camera_bench.jsonl).  One process measures one of

  --what thin_lens|ortho|equirect   pt_render_async under that model (thin lens: --aperture, --focus-distance)
  --what pinhole     baseline (a): the same tree's pinhole render with option fuse_gen = 0 — the same pipeline
                     shape (camera paths from a generate kernel), so the difference is the generate kernel
  --what host_rays   baseline (b): the only route to such an image without the feature — rays made on the host
                     (here: the frame-0 camera rays, read back once outside the timed region and standing in for any
                     host-made set), one upload of 32 B per ray and one pt_query_radiance_async(nsamples = 1) per
                     sample, the upload inside the timed region.  Runs on the parent commit's package with --pkg.

and prints one JSON line: ms per call (median of --runs after one warm-up call, the spread max - min and every
run; wall clock around the call and a stream synchronisation), Msamples/s = width * height * samples / median,
and from a further profiled call (pt_profile_read) the generate kernel's share of the kernels' busy time.

  python scripts/camera_bench.py --what thin_lens --scene CornellBox --width 1024 --height 1024 --samples 64
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=["thin_lens", "ortho", "equirect", "pinhole", "host_rays"], required=True)
    ap.add_argument("--scene", default="CornellBox", help="a scene of scenes/scene_assets (without .xml)")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--aperture", type=float, default=0.1)
    ap.add_argument("--focus-distance", type=float, default=3.6)
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
        if a.what == "host_rays":
            h_rays = torch.from_numpy(s.camera_rays(meta, 0).reshape(n, 8)).pin_memory()
            d_rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
            d_seeds = torch.zeros(n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            s.camera_seeds_async(meta, 0, d_seeds.data_ptr(), stream_ptr=st.cuda_stream)

            def call():
                with torch.cuda.stream(st):
                    for _ in range(a.samples):  # fresh directions per sample: one upload per sample
                        d_rays.copy_(h_rays, non_blocking=True)
                        s.query_radiance_async(d_rays.data_ptr(), d_seeds.data_ptr(), n, d_acc.data_ptr(), 1, a.depth,
                                               float(meta[45]), bool(meta[46] > 0), stream_ptr=st.cuda_stream)
        else:
            if a.what == "pinhole":
                pt_amd.set_option("fuse_gen", 0)
            else:
                s.set_camera(a.what, a.aperture, a.focus_distance)
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
                      "msamples_per_s": n * a.samples / med / 1e3, "kernel_busy_ms": busy,
                      "generate_share": busy.get("k_wf_generate", 0.0) / max(sum(busy.values()), 1e-9),
                      "upload_mb_per_call": (n * 32 * a.samples / 1e6) if a.what == "host_rays" else 0.0,
                      "accum_mean": float(d_acc.mean().item()), "build_id": pt_amd.build_id()}))


if __name__ == "__main__":
    main()
