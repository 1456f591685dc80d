#!/usr/bin/env python3
"""Scene-creation time and render throughput of scenes built on the device (pt_scene_create_mesh) against the
host route, on one GPU.  Writes profiles/lbvh_build.jsonl, one JSON line per scene:

  stages     the device time of the build by stage (HIP events around every launch, through pt_profile_read) and
             the sort's share of it; upload_bytes: the triangle_data a creation uploads from pageable memory.
  creation   wall time of Scene.from_mesh(triangle_data) against bvh_build(sah, isolate) + Scene(...), and the
             host builders alone (bvh_build_lbvh, bvh_build sah): medians of RUNS runs in this process, min and
             max recorded.  Condition (asserted at the end): the device route is faster at 100,000 and at
             1,000,000 triangles.
  render     Msamples/s at the sweep's settings (1024^2, 16 spp, depth 8; median of RUNS) on the LBVH tree at
             max_leaf 4 and 8 and on the SAH tree of the same mesh.  Recorded, not gated.

usage: build_bench.py [--scenes NAME,...] [--runs 5] [--out profiles/lbvh_build.jsonl] [--no-render]
scenes: CornellBox-Glossy, MedievalBoat, synthetic-N
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "brown-cs2240-path-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import pt_amd  # noqa: E402
import synth_scene  # noqa: E402

PACK_JS = os.path.join(ROOT, "brown-cs2240-path-tracer_amd", "node", "bin", "pt-pack.js")
W = H = 1024
SPP, DEPTH = 16, 8


def pack(name, td):
    """triangle_data and meta of a scene; the tree packed with it (the LBVH: the cheapest to make) is not used."""
    if name.startswith("synthetic-"):
        xml = synth_scene.write(int(name.split("-")[1]), os.path.join(td, "synth"))
    else:
        xml = os.path.join(ROOT, "scenes", "scene_assets", name + ".xml")
    out = os.path.join(td, "packed")
    subprocess.run(["node", PACK_JS, xml, out, "--bvh", "lbvh", "--width", str(W), "--height", str(H)], check=True,
                   capture_output=True)
    return np.fromfile(os.path.join(out, "triangle_data.f32"), np.float32), np.fromfile(os.path.join(out, "meta.f32"), np.float32)


def mesh_of(tri):
    nv, i0, m0 = int(tri[0]), int(tri[3]), int(tri[4])
    ke = tri[m0:m0 + 15 * int(tri[1])].reshape(-1, 15)[:, 12:15]
    return (tri[16:16 + 3 * nv].reshape(-1, 3).astype(np.float64), tri[i0:m0].reshape(-1, 4).astype(np.int32),
            ((ke[:, 0] + ke[:, 1]) + ke[:, 2] > 0).astype(np.uint8))


def timed(fn, runs):
    ts, last = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        last = fn()
        ts.append(time.perf_counter() - t0)
    return last, {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def stages(tri, runs):
    """The build's device time by stage (pt_build_params.profile, pt_profile_read: HIP events around every launch,
    a stage's launches summed): per stage the median over the runs, and the sort's share of their sum."""
    per = {}
    for _ in range(runs):
        with pt_amd.Scene.from_mesh(tri, profile=True) as s:
            for name, k in s.profile_read().items():
                per.setdefault(name, []).append(k["total_ms"])
    med = {name: statistics.median(v) for name, v in per.items()}
    return med, med["k_build_sort"] / sum(med.values())


def msamples(scene, meta, runs):
    scene.render(meta, 0, 1, 1, DEPTH, pt_amd.MODE_AUTO)  # buffers, first launch
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        scene.render(meta, 0, SPP, 1, DEPTH, pt_amd.MODE_AUTO)
        ts.append(time.perf_counter() - t0)
    rate = [W * H * SPP / t / 1e6 for t in ts]
    return {"median": statistics.median(rate), "min": min(rate), "max": max(rate)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="CornellBox-Glossy,MedievalBoat,synthetic-12500,synthetic-100000,synthetic-1000000")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbvh_build.jsonl"))
    ap.add_argument("--no-render", action="store_true")
    args = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as td:
        with pt_amd.Scene.from_mesh(pack("CornellBox-Glossy", td)[0]):
            pass  # the runtime and the code objects are loaded before anything is timed
    for name in args.scenes.split(","):
        with tempfile.TemporaryDirectory() as td:
            tri, meta = pack(name, td)
        verts, recs, flags = mesh_of(tri)
        row = {"scene": name, "triangles": int(len(recs)), "runs": args.runs, "upload_bytes": int(tri.nbytes)}

        def device():
            s = pt_amd.Scene.from_mesh(tri)
            s.close()

        def host():
            s = pt_amd.Scene(tri, pt_amd.bvh_build(verts, recs, sah=True, isolate=flags))
            s.close()
        _, row["create_device"] = timed(device, args.runs)
        _, row["create_host_sah"] = timed(host, args.runs)
        sah, row["host_bvh_build_sah"] = timed(lambda: pt_amd.bvh_build(verts, recs, sah=True, isolate=flags), args.runs)
        _, row["host_bvh_build_lbvh"] = timed(lambda: pt_amd.bvh_build_lbvh(tri), args.runs)
        row["host_over_device"] = row["create_host_sah"]["median_s"] / row["create_device"]["median_s"]
        row["stages_ms"], row["sort_share"] = stages(tri, args.runs)
        if not args.no_render:
            for max_leaf in (4, 8):
                with pt_amd.Scene.from_mesh(tri, max_leaf=max_leaf) as s:
                    row[f"msamples_lbvh{max_leaf}"] = msamples(s, meta, args.runs)
                    row[f"info_lbvh{max_leaf}"] = s.info
            with pt_amd.Scene(tri, sah) as s:
                row["msamples_sah"] = msamples(s, meta, args.runs)
                row["info_sah"] = s.info
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    for row in rows:
        if row["triangles"] >= 100000:
            assert row["host_over_device"] > 1.0, (row["scene"], row["host_over_device"])


if __name__ == "__main__":
    main()
