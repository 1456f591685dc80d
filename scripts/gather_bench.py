#!/usr/bin/env python3
"""Paths per second of pt_gather_async against the radiance query it replaces (profiles/gather_throughput.jsonl;
DESIGN.md §5.13).  The points are the first hits of the image's frame-0 camera rays (pt_camera_rays_async +
pt_query_hits_async, misses dropped, the rest repeated up to --points), with their geometric normals and seeded
seeds: the same in every process.  One process does one of

  --what gather    pt_gather_async over --samples samples of every point, --mode cosine | sh9, from device buffers
  --what emit      pt_gather_rays_async for samples 0 .. --samples - 1: the rays and seeds of every sample, written
                   to --rays-file (numpy .npz, 36 B per path)
  --what baseline  pt_query_radiance_async(nsamples = 1) on the device-resident rays and seeds of --rays-file, one call
                   per sample: what a caller without pt_gather runs once the directions are on the device (run it with
                   --pkg pointing at the parent commit's package for the comparison DESIGN.md records).  Its sums are
                   the COSINE gather's, bit for bit: accum_sha256 of both lines agree.

and prints one JSON line: ms per call (median of --runs after one warm-up call, the spread max - min and every run;
wall clock around the call and a stream synchronisation), Mpaths/s = points * samples / median, and from a further
profiled call (pt_profile_read) the generate and accumulate kernels' shares of the kernels' busy time.

  python scripts/gather_bench.py --what gather --scene CornellBox --points 1048576 --samples 16
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def surface_points(pt_amd, torch, s, ps, side, count, st):
    """[count, 8] f32 gather points: hits of the side x side image's camera rays, seeds from a fixed generator."""
    n = side * side
    d_rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    d_hits = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s.camera_rays_async(ps.meta, 0, d_rays.data_ptr(), stream_ptr=st.cuda_stream)
    s.query_hits_async(d_rays.data_ptr(), n, d_hits.data_ptr(), stream_ptr=st.cuda_stream)
    st.synchronize()
    hits = d_hits.cpu().numpy()
    hits = hits[hits[:, 3] > 0]
    if len(hits) == 0:
        raise SystemExit("the camera sees nothing")
    idx = np.resize(np.arange(len(hits)), count)
    pts = np.zeros((count, 8), np.float32)
    pts[:, 0:3] = hits[idx, 0:3]
    pts[:, 4:7] = hits[idx, 4:7]
    pts.view(np.uint32)[:, 3] = np.random.default_rng(20261022).integers(0, 2 ** 32, count, dtype=np.uint32)
    return pts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=["gather", "emit", "baseline"], required=True)
    ap.add_argument("--mode", choices=["cosine", "sh9"], default="cosine")
    ap.add_argument("--scene", default="CornellBox", help="a scene of scenes/scene_assets (without .xml)")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--side", type=int, default=1024, help="the image whose camera rays find the points")
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--rays-file", default="")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "brown-cs2240-path-tracer_amd"))
    a = ap.parse_args()
    if a.what != "gather" and not a.rays_file:
        ap.error("--what emit and --what baseline need --rays-file")

    sys.path.insert(0, a.pkg)
    import torch

    import pt_amd

    ps = pt_amd.load_scene(os.path.join(ROOT, "scenes", "scene_assets", a.scene + ".xml"), width=a.side, height=a.side)
    n, rrp, direct = a.points, float(ps.meta[45]), bool(ps.meta[46] > 0)
    st = torch.cuda.Stream()
    with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
        if a.what == "emit":
            d_pts = torch.from_numpy(surface_points(pt_amd, torch, s, ps, a.side, n, st)).cuda()
            d_rays = torch.zeros((a.samples, n, 8), dtype=torch.float32, device="cuda")
            d_seeds = torch.zeros((a.samples, n), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for k in range(a.samples):
                s.gather_rays_async(d_pts.data_ptr(), n, k, d_rays[k].data_ptr(), d_seeds[k].data_ptr(), a.mode, st.cuda_stream)
            st.synchronize()
            s.check()
            np.savez(a.rays_file, rays=d_rays.cpu().numpy(), seeds=d_seeds.cpu().numpy())
            print(json.dumps({"what": "emit", "scene": a.scene, "points": n, "samples": a.samples, "file": a.rays_file}))
            return
        width = 27 if (a.what == "gather" and a.mode == "sh9") else 3
        d_acc = torch.zeros((n, width), dtype=torch.float32, device="cuda")
        if a.what == "gather":
            d_pts = torch.from_numpy(surface_points(pt_amd, torch, s, ps, a.side, n, st)).cuda()
            torch.cuda.synchronize()

            def call():
                s.gather_async(d_pts.data_ptr(), n, d_acc.data_ptr(), a.samples, 0, a.mode, a.depth, rrp, direct,
                               stream_ptr=st.cuda_stream)
        else:
            with np.load(a.rays_file if a.rays_file.endswith(".npz") else a.rays_file + ".npz") as z:
                if z["rays"].shape != (a.samples, n, 8):
                    raise SystemExit(f"{a.rays_file} holds {z['rays'].shape}, not ({a.samples}, {n}, 8)")
                d_rays, d_seeds = torch.from_numpy(z["rays"]).cuda(), torch.from_numpy(z["seeds"]).cuda()
            torch.cuda.synchronize()

            def call():
                for k in range(a.samples):
                    s.query_radiance_async(d_rays[k].data_ptr(), d_seeds[k].data_ptr(), n, d_acc.data_ptr(), 1, a.depth, rrp,
                                           direct, stream_ptr=st.cuda_stream)
        call()
        st.synchronize()
        first = hashlib.sha256(d_acc.cpu().numpy().tobytes()).hexdigest()  # the sums of one call into zeros
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
    total = max(sum(busy.values()), 1e-9)
    med = statistics.median(ms)
    print(json.dumps({"what": a.what, "mode": a.mode if a.what == "gather" else "cosine", "label": a.label, "scene": a.scene,
                      "points": n, "samples": a.samples, "depth": a.depth, "ms_median": med, "ms_spread": max(ms) - min(ms),
                      "ms_runs": ms, "mpaths_per_s": n * a.samples / med / 1e3, "kernel_busy_ms": busy,
                      "generate_share": busy.get("k_wf_generate", 0.0) / total, "accum_share": busy.get("k_wf_accum", 0.0) / total,
                      "accum_sha256": first, "build_id": pt_amd.build_id()}))


if __name__ == "__main__":
    main()
