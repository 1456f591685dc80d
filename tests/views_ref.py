"""The reference of a view-list render (include/pt_hip.h pt_render_views), shared by
test_views_cpu.py, test_gpu_views.py and test_gpu_node_views.py: every view is its own window render —
lens_ref.render for a lens view, the same accumulation (radiance_ref.radiance, the oracle's own radiance())
over radiance_ref.camera_rays_seeds for a pinhole view (lens_ref.camera_ray restates the three lens models
only) — placed into the atlas; the counters are summed.  test_views_cpu.py pins the pinhole path against
oracle.render.

The view sets are the smallest shapes at which the slot map can go wrong; their cameras come from
cam_cases.py's catalogue and lens_ref.CASES, and every view carries light in >= 0.25 of its pixels
(test_views_cpu.py, on the oracle alone)."""
import numpy as np

import cam_cases as cc
import lens_ref as lr
import radiance_ref as rr

F = np.float32
NFRAMES, DEPTH = 3, 8
THIN = ("thin_lens", 0.3, 3.6)
ORTHO = ("ortho", 0.0, 3.6)
EQUI = ("equirect", 0.0, 1.0)


def V(camera, size=None, window=None, cam=None, frame0=lr.FRAME0, dst=None):
    return {"camera": camera, "size": size, "window": window, "cam": cam, "frame0": frame0, "dst": dst}


# name -> (scene, atlas (w, h) or None: packed by pt_amd.view_atlas, views)
SETS = {
    # five pinhole views, one image of another size (W, H, inv_w, inv_h, aspect differ between rows), one view
    # a single pixel, every border between views inside a 64-path batch and inside a wave, per-view frame0,
    # destinations with gaps between them and listed in an order that is not their atlas order
    "mixed5": ("CornellBox", (96, 64), [
        V("xml", (40, 32), (3, 2, 33, 27), frame0=2, dst=(60, 34)),
        V("oblique", (24, 16), (0, 0, 24, 16), frame0=0, dst=(1, 1)),
        V("inside_in", (40, 32), (0, 0, 1, 1), frame0=7, dst=(30, 20)),  # the one camera whose corner pixel sees light
        V("rolled", (40, 32), (7, 5, 13, 11), frame0=2, dst=(40, 3)),
        V("above", (40, 32), (1, 0, 39, 31), frame0=1000, dst=(2, 30)),
    ]),
    # all four models in one launch: the model switch diverges inside waves
    "models4": ("CornellBox", None, [V("xml"), V("xml", cam=THIN), V("oblique", cam=ORTHO), V("inside_in", cam=EQUI)]),
    "boat3": ("MedievalBoat", None, [V("rigging"), V("rigging", cam=("thin_lens", 0.05, lr.BOAT_FOCUS)), V("rolled_low")]),
    "glossy2": ("CornellBox-Glossy", None, [V("oblique", cam=THIN), V("inside_in", cam=EQUI)]),
    "sphere2": ("CornellBox-Sphere", None, [V("oblique", cam=ORTHO), V("inside_in")]),
    # the same meta twice, frames 0..2 and 3..5
    "twins": ("CornellBox", None, [V("xml", frame0=0), V("xml", frame0=3)]),
}
MIXED5_FIRST, MIXED5_NPIX = [0, 891, 1275, 1276, 1419], 2628


def views_of(name):
    """(scene, [view dicts for Scene.render_views, each with its dst], atlas (w, h)) of a set."""
    import pt_amd
    scene, atlas, spec = SETS[name]
    out = []
    for v in spec:
        size = v["size"] or cc.size_of(scene)
        meta = cc.meta_of(scene, v["camera"], size)
        out.append({"meta": meta, "window": v["window"] or (0, 0, size[0], size[1]), "camera": v["cam"], "frame0": v["frame0"],
                    "dst": v["dst"]})
    if atlas is None:
        dsts, atlas = pt_amd.view_atlas([v["window"][2:] for v in out])
        for v, d in zip(out, dsts):
            v["dst"] = d
    return scene, out, atlas


def view_frames(view, nframes, stride=1):
    """[(rays [h, w, 8], seeds [h, w], admitted [h, w]) per frame] of a view's window."""
    frames = []
    for k in range(nframes):
        f = view["frame0"] + k * stride
        if view["camera"] is None:
            rays, seeds = rr.camera_rays_seeds(view["meta"], f, view["window"])
            frames.append((rays, seeds, np.ones(seeds.shape, bool)))
        else:
            frames.append(lr.rays_seeds(view["meta"], view["camera"], f, view["window"]))
    return frames


def place(atlas, view):
    """The view's destination rectangle of atlas [h, w, 3] (a numpy view)."""
    (x, y), (_, _, w, h) = view["dst"], view["window"]
    return atlas[y:y + h, x:x + w]


def initial_atlas(atlas):
    return lr.initial_accum(atlas[1], atlas[0])


_REF = {}


def reference(lib, packed, name, nframes=NFRAMES, stride=1, depth=DEPTH):
    """The set's reference, computed once per process and shared (callers leave it unchanged): (atlas
    [ah, aw, 3] rendered onto initial_atlas, counters summed over the views, [tile from zeros per view])."""
    key = (name, nframes, stride, depth)
    if key not in _REF:
        scene, views, atlas = views_of(name)
        out = initial_atlas(atlas)
        total, tiles = {}, []
        for v in views:
            frames = view_frames(v, nframes, stride)
            onto, cnt = lr.accumulate(lib, packed[scene], v["meta"], frames, depth, place(out, v))
            place(out, v)[...] = onto
            tiles.append(lr.accumulate(lib, packed[scene], v["meta"], frames, depth, np.zeros_like(onto))[0])
            for k, c in cnt.items():
                total[k] = total.get(k, 0) + c
        _REF[key] = (out, total, tiles)
    return _REF[key]


def inside_mask(views, atlas):
    m = np.zeros((atlas[1], atlas[0]), bool)
    for v in views:
        (x, y), (_, _, w, h) = v["dst"], v["window"]
        m[y:y + h, x:x + w] = True
    return m
