#!/usr/bin/env python3
"""What the adaptive driver costs (profiles/adaptive_driver.jsonl, profiles/rects_driver.jsonl;
DESIGN.md §5.8): one JSON line per run with
  * driver_wall_ms       pt_render_adaptive, wall clock of the blocking call (the median of --runs, and every run),
  * uniform_render_wall_ms_runs  Scene.render of round(mean spp) frames of the whole image, the same samples
                         spent uniformly,
  * per_pass             the driver's passes replayed from Python on device buffers, each timed with a
                         synchronisation after it: frames, rectangles, active tiles, render_ms, noise_ms.
                         A refinement pass is one render_rects_async over the pass's rectangles, as the
                         driver renders it; --per-rectangle renders one window call per rectangle instead
                         (what the driver did before it had the list call, and the only replay a library
                         without the list call can run).  The replay must end with the driver's tile_frames
                         (python_passes_same_tile_frames).

  python scripts/adaptive_driver.py --scene CornellBox --size 1024 --tile 64 --frames 16 16 256 --tol 0.05

--pkg DIR runs another build of the package (a directory that holds pt_amd/ and lib/), for A/B runs.
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
    ap.add_argument("--scene", default="CornellBox", help="a scene of scenes/scene_assets (without .xml)")
    ap.add_argument("--size", type=int, default=1024, help="the image is size x size")
    ap.add_argument("--tile", type=int, default=64, help="tiles are tile x tile")
    ap.add_argument("--frames", type=int, nargs=3, default=(16, 16, 256), metavar=("MIN", "STEP", "MAX"))
    ap.add_argument("--tol", type=float, default=0.05)
    ap.add_argument("--floor", type=float, default=0.05)
    ap.add_argument("--noisy-fraction", type=float, default=0.02)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--mode", choices=("auto", "megakernel", "wavefront"), default="auto")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--per-rectangle", action="store_true", help="replay a pass as one window render per rectangle")
    ap.add_argument("--label", default="", help="copied into the line (e.g. the build)")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "brown-cs2240-path-tracer_amd"))
    a = ap.parse_args()

    sys.path.insert(0, a.pkg)
    import torch

    import pt_amd

    xml = os.path.join(ROOT, "scenes", "scene_assets", a.scene + ".xml")
    packed = pt_amd.load_scene(xml, width=a.size, height=a.size)
    meta = np.asarray(packed.meta, np.float32)
    W = H = a.size
    tile = (a.tile, a.tile)
    lo, step, hi = a.frames
    mode = {"auto": pt_amd.MODE_AUTO, "megakernel": pt_amd.MODE_MEGAKERNEL, "wavefront": pt_amd.MODE_WAVEFRONT}[a.mode]
    per_rectangle = a.per_rectangle or not hasattr(pt_amd.Scene, "render_rects_async")
    tx, ty = -(-W // a.tile), -(-H // a.tile)

    def ms_since(t0):
        return (time.perf_counter() - t0) * 1e3

    with pt_amd.Scene(packed.triangle_data, packed.bvh_data) as s:
        def driver():
            return s.render_adaptive(meta, 0, a.depth, mode, tile=tile, min_frames=lo, step_frames=step, max_frames=hi,
                                     tol=a.tol, floor=a.floor, noisy_fraction=a.noisy_fraction, counters=False)
        r = driver()  # warm-up: allocations, the probe, the clocks
        driver_ms = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            r = driver()
            driver_ms.append(ms_since(t0))
        tile_frames = r["tile_frames"]
        pixels = np.minimum(a.tile, W - np.arange(tx) * a.tile)[None, :] * np.minimum(a.tile, H - np.arange(ty) * a.tile)[:, None]
        total = int((tile_frames.astype(np.int64) * pixels).sum())
        mean_spp = total / (W * H)

        s.render(meta, 0, max(1, round(mean_spp)), 1, a.depth, mode)
        uniform_ms = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            s.render(meta, 0, max(1, round(mean_spp)), 1, a.depth, mode)
            uniform_ms.append(ms_since(t0))

        # the driver's passes from Python, each with a synchronisation of its own
        def replay():
            acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            m2 = torch.zeros_like(acc)
            d_out = torch.zeros(tx * ty * 2, dtype=torch.float64, device="cuda")
            frames = np.full((ty, tx), lo, np.uint32)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.render_moments_async(meta, 0, lo, 1, a.depth, mode, acc.data_ptr(), m2.data_ptr())
            torch.cuda.synchronize()
            log = [{"pass": 0, "frames": lo, "rects": 1, "active_tiles": tx * ty, "render_ms": ms_since(t0)}]
            done = lo
            while True:
                d_fr = torch.from_numpy(frames.astype(np.int32)).cuda()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.noise_tiles_async(acc.data_ptr(), m2.data_ptr(), W, H, tile, d_fr.data_ptr(), a.tol, a.floor, d_out.data_ptr())
                torch.cuda.synchronize()
                log[-1]["noise_ms"] = ms_since(t0)
                noise = d_out.cpu().numpy().view(pt_amd.TILE_NOISE_DTYPE).reshape(ty, tx)
                limit = (a.noisy_fraction * noise["pixels"].astype(np.float64)).astype(np.uint32)
                active = (noise["noisy"] > limit) & (frames < hi)
                if not active.any():
                    return frames, log
                nf = min(step, hi - done)
                rects = [(int(x) * a.tile, int(y) * a.tile, min(int(w) * a.tile, W - int(x) * a.tile),
                          min(int(h) * a.tile, H - int(y) * a.tile)) for x, y, w, h in pt_amd.tile_rects(active)]
                t0 = time.perf_counter()
                if per_rectangle:
                    for x0, y0, w, h in rects:
                        o = 12 * (y0 * W + x0)
                        s.render_moments_async(meta, done, nf, 1, a.depth, mode, acc.data_ptr() + o, m2.data_ptr() + o,
                                               window=(x0, y0, w, h), row_pitch=W)
                else:
                    s.render_rects_async(meta, rects, done, nf, 1, a.depth, mode, acc.data_ptr(), m2.data_ptr(), row_pitch=W)
                torch.cuda.synchronize()
                log.append({"pass": len(log), "frames": nf, "rects": len(rects), "active_tiles": int(active.sum()),
                            "render_ms": ms_since(t0)})
                frames[active] += nf
                done += nf

        replay()  # warm-up
        frames, log = replay()
        s.check()

    hist = {str(k): int((tile_frames == k).sum()) for k in np.unique(tile_frames)}
    print(json.dumps({
        "label": a.label, "scene": a.scene, "image": f"{W}x{H}", "depth": a.depth, "mode": a.mode, "min_frames": lo,
        "step_frames": step, "max_frames": hi, "tol": a.tol, "floor": a.floor, "noisy_fraction": a.noisy_fraction,
        "tile": list(tile), "total_samples": total, "mean_spp": mean_spp, "passes": int(r["passes"]),
        "driver_wall_ms": statistics.median(driver_ms), "driver_wall_ms_runs": driver_ms,
        "uniform_render_wall_ms": statistics.median(uniform_ms), "uniform_render_wall_ms_runs": uniform_ms,
        "replay": "one window render per rectangle" if per_rectangle else "one list render per pass",
        "python_passes_render_ms_sum": sum(p["render_ms"] for p in log),
        "python_passes_noise_ms_sum": sum(p.get("noise_ms", 0.0) for p in log),
        "python_passes_same_tile_frames": bool(np.array_equal(frames, tile_frames)),
        "tile_frames_hist": hist, "tiles_at_max": int((tile_frames == hi).sum()), "tiles": tx * ty,
        "tile_frames": [int(v) for v in tile_frames.ravel()],
        "per_pass": log}))


if __name__ == "__main__":
    main()
