#!/usr/bin/env python3
"""Rays per second of the ray queries (profiles/query_bench.jsonl).  One process measures
one scene and prints one JSON line per ray set:
  camera       the image's frame-0 camera rays (pt_camera_rays), coherent, in pixel order
  incoherent   from every camera hit point, nudged 1e-3 along the normal that faces the camera, a uniform
               direction of the hemisphere around that normal, made on the host with a fixed seed
and per set, in Mrays/s from pt_profile_read (HIP events around the one launch):
  hits_refill1, hits_refill0   pt_query_hits_async with option query_refill = 1 and 0
  occl_refill1, occl_refill0   pt_query_occluded_async with tmax = +inf: hits minus this is what early exit
                               buys, and with refill off how much of that the idle lanes lose
  features (camera set only)   one frame of k_features over the same rays: the same closest hits, one
                               lane per pixel, the fast reciprocal, no refill — the yardstick
The settings alternate inside a run (--runs runs: the median, the spread max - min, and every run); take
three processes.  same_bits: both refill settings gave the same bytes, and with tmax = +inf the
occlusion bytes are the hits' "material >= 0".

  python scripts/query_bench.py --scene CornellBox --width 1024 --height 1024
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = (("hits_refill1", False, 1), ("hits_refill0", False, 0), ("occl_refill1", True, 1), ("occl_refill0", True, 0))


def hemisphere_rays(hits, cam_d, rng):
    """Rays leaving the hit points: [m, 8] f32 for the m hits among the records."""
    hit = hits[:, 7].view(np.int32) >= 0
    p, n, d = hits[hit, 0:3], hits[hit, 4:7].copy(), cam_d[hit]
    n[(n * d).sum(axis=1) > 0] *= -1  # the side the camera ray came from
    v = rng.standard_normal((len(p), 3)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[(v * n).sum(axis=1) < 0] *= -1
    rays = np.zeros((len(p), 8), np.float32)
    rays[:, 0:3] = p + np.float32(1e-3) * n
    rays[:, 3] = np.inf
    rays[:, 4:7] = v
    return rays


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="CornellBox", help="a scene of scenes/scene_assets (without .xml)")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--label", default="")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "brown-cs2240-path-tracer_amd"))
    a = ap.parse_args()

    sys.path.insert(0, a.pkg)
    import torch

    import pt_amd

    packed = pt_amd.load_scene(os.path.join(ROOT, "scenes", "scene_assets", a.scene + ".xml"), width=a.width, height=a.height)
    meta = np.asarray(packed.meta, np.float32)
    W, H = a.width, a.height

    with pt_amd.Scene(packed.triangle_data, packed.bvh_data) as s:
        def kernel_ms(fn, name):
            s.profile_enable(True)
            fn()
            torch.cuda.synchronize()
            t = s.profile_read()
            s.profile_enable(False)
            assert t[name]["launches"] == 1, t
            return t[name]["total_ms"]

        cam = s.camera_rays(meta, 0).reshape(-1, 8)
        sets = {"camera": cam, "incoherent": hemisphere_rays(s.query_hits(cam), cam[:, 4:7], np.random.default_rng(a.seed))}
        geo = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        alb = torch.zeros_like(geo)
        for name, rays in sets.items():
            n = len(rays)
            d_rays = torch.from_numpy(rays).cuda()
            d_hits = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
            d_occ = torch.zeros((n,), dtype=torch.uint8, device="cuda")

            def run(occluded, refill):
                pt_amd.set_option("query_refill", refill)
                if occluded:
                    return kernel_ms(lambda: s.query_occluded_async(d_rays.data_ptr(), n, d_occ.data_ptr()), "k_query_occluded")
                return kernel_ms(lambda: s.query_hits_async(d_rays.data_ptr(), n, d_hits.data_ptr()), "k_query_hits")

            def features():
                return kernel_ms(lambda: s.render_features_async(meta, 0, 1, 1, geo.data_ptr(), alb.data_ptr()), "k_features")

            # warm-up of every instance, and the bytes of every setting
            got = {}
            for key, occluded, refill in SETTINGS:
                run(occluded, refill)
                got[key] = (d_occ if occluded else d_hits).cpu().numpy().copy()
            same = bool(np.array_equal(got["hits_refill1"].view(np.uint32), got["hits_refill0"].view(np.uint32)) and
                        np.array_equal(got["occl_refill1"], got["occl_refill0"]) and
                        np.array_equal(got["occl_refill1"] != 0, got["hits_refill1"][:, 7].view(np.int32) >= 0))
            if name == "camera":
                features()
            ms = {key: [] for key, _, _ in SETTINGS}
            feat = []
            for _ in range(a.runs):
                for key, occluded, refill in SETTINGS:  # the settings alternate
                    ms[key].append(run(occluded, refill))
                if name == "camera":
                    feat.append(features())
            pt_amd.set_option("query_refill", None)
            s.check()

            def rate(v):
                r = [n / (x * 1e3) for x in v]  # Mrays/s
                return {"median": statistics.median(r), "spread": max(r) - min(r), "runs": r}

            line = {"label": a.label, "scene": a.scene, "image": f"{W}x{H}", "set": name, "rays": n,
                    "hit_share": float((got["hits_refill1"][:, 7].view(np.int32) >= 0).mean()), "runs": a.runs,
                    "mrays_per_s": {key: rate(v) for key, v in ms.items()}, "same_bits": same}
            if feat:
                line["mrays_per_s"]["features"] = rate(feat)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
