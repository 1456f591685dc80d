"""Cameras the scenes never use (a helper module like tests/cond_scenes.py, not a conftest): the
catalogue tests/test_cam_cpu.py and tests/test_gpu_cam.py share.  The geometry is the `packed`
fixture's; only the 48-float meta block changes.

The four Cornell scenes share one camera (pos (0, 1, 3.6), focus (0, 1, 0), up (0, 1, 0), 45 degrees):
its look-at matrix is the identity plus a translation, so M[1], M[2], M[4], M[6], M[8], M[9] are +-0,
M[3] = M[7] = M[11] = 0 and pw = M[15]: a transposed 3 x 3 block, swapped fmaf operands, a dropped
pw / dw term or an ignored cam[3] in camera_ray (pt_device.h) would go unseen on the scenes that run
the bench pipeline.  CAMERAS names other viewpoints per scene; each becomes a meta through
scene_oracle.make_meta (meta_of) at SIZES.  PERTURBATIONS change single fields of the oblique
CornellBox meta that no scene varies.

kind:
  seeing   light in >= 0.25 of the pixels of the 3-frame render
  mixed    light in 0.05 .. 0.30 of them, and both hits and misses among frame 0's camera rays
  miss     every camera ray misses: no light, no shadow query, W * H extension queries per frame
  under    no light, but more extension queries than that (the boat's ocean seen from below)
The conditions are tests/test_cam_cpu.py's; the `lit` figures here are the oracle's, measured there
(3-frame render, depth 8).
"""
import os

import numpy as np

import scene_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "scenes", "scene_assets")

DEPTH = 8
SALT = 3
SETTINGS = {"samplesPerPixel": 16, "pathContinuationProb": 0.9, "directLightingOnly": False}  # pt-pack.js's for an XML
UP = (0.0, 1.0, 0.0)
CORNELL_POS, CORNELL_FOCUS = (0.0, 1.0, 3.6), (0.0, 1.0, 0.0)


def size_of(scene):
    return (24, 16) if scene == "MedievalBoat" else (40, 32)


def cam(pos, focus, up=UP, angle=45.0, kind="seeing"):
    return {"pos": tuple(map(float, pos)), "focus": tuple(map(float, focus)), "up": tuple(map(float, up)),
            "heightangle": float(angle), "kind": kind}


# name -> camera; "xml" is the scene file's own (None: read from it).  lit: 3-frame render.
CORNELL = {
    "xml": None,                                                                             # lit 0.659
    "oblique": cam((1.7, 2.3, 3.1), (-0.2, 0.6, -0.3)),                                      # 0.555
    "rolled": cam((0.4, 1.2, 3.3), (0, 1, 0), up=(0.6, 0.8, 0.1)),                           # 0.702
    "inside_out": cam((0.1, 1, -0.5), (0.3, 1.1, 4)),                                        # 0.354
    "inside_in": cam((0.2, 0.4, 0.6), (-0.3, 1.9, -0.4)),                                    # 1.000
    "behind": cam((0.3, 1.1, -4), (0, 1, 0)),                                                # 0.541
    "above": cam((0.05, 5, 0.1), (0, 0, 0), up=(0, 0, -1)),                                  # 0.513
    "side": cam((4, 1, 0.2), (0, 1, 0)),                                                     # 0.537
    "beside_wall": cam((0.999, 1, 0), (-1, 1.2, 0.1)),                                       # 0.917
    "in_tall_box": cam((-0.33, 0.6, -0.29), (0.5, 1, 1)),                                    # 0.995
    "tele3": cam(CORNELL_POS, (0, 1.95, 0), angle=3),                                        # 0.976
    "far_tele": cam((0, 1, 120), (0, 1, 0), angle=1.5),                                      # 0.320
    "wide170": cam((0, 1, 1.2), (0, 1, 0), angle=170, kind="mixed"),                         # 0.146
    "fov179": cam((0, 1, 0.9), (0, 1, 0), angle=179),
    "fov0.01": cam(CORNELL_POS, CORNELL_FOCUS, angle=0.01),
    "away": cam(CORNELL_POS, (0, 1, 8), kind="miss"),                                        # 0
}
SMALL = {"oblique": CORNELL["oblique"], "inside_in": CORNELL["inside_in"]}
BOAT = {
    "xml": None,                                                                             # 0.143, mixed
    "rigging": cam((1.32, 3.2, 1.96), (0.49, 2.07, 1.13), angle=60),                         # cond_scenes': 0.878
    "rolled_low": cam((-3, 0.6, 2.5), (0.2, 1.5, 0.1), up=(0.3, 0.9, -0.2), angle=50),       # 0.266
    # over the ocean's edge (the ocean is 20 x 20 around the boat): 320 of 384 camera rays hit
    "top_down": cam((6, 8, 0.2), (5.5, 0, 0.1), up=(0, 0, -1), angle=60, kind="mixed"),      # 0.151
    "away": cam((5, 5, 5), (10, 8, 10), angle=80, kind="miss"),
    "under": cam((2, -1.5, 2), (0, 2, 0), angle=80, kind="under"),
}
CAMERAS = {"CornellBox": CORNELL, "CornellBox-Glossy": SMALL, "CornellBox-Mirror": SMALL, "CornellBox-Sphere": SMALL,
           "MedievalBoat": BOAT}
XML_KIND = {"MedievalBoat": "mixed"}  # the other scenes' own cameras see

CASES = [(s, c) for s in CAMERAS for c in CAMERAS[s]]


def case_id(scene, name):
    return f"{scene}-{name}"


_XML = {}


def camera(scene, name):
    """The camera's dict (pos, focus, up, heightangle, kind); "xml": the scene file's."""
    c = CAMERAS[scene][name] if name != "xml" else None
    if c is None:
        if scene not in _XML:
            with open(os.path.join(ASSETS, scene + ".xml")) as f:
                x = so.load_scene_xml(f.read())[0]
            _XML[scene] = cam(x["pos"], x["focus"], x["up"], x["heightangle"], XML_KIND.get(scene, "seeing"))
        c = _XML[scene]
    return c


def meta_from(c, W, H):
    """scene_oracle.make_meta of a camera dict at W x H, the Node host's settings for an XML."""
    return so.make_meta([W, H], {"pos": list(c["pos"]), "focus": list(c["focus"]), "up": list(c["up"]),
                                 "heightangle": c["heightangle"]}, SETTINGS)


def meta_of(scene, name, size=None):
    W, H = size or size_of(scene)
    return meta_from(camera(scene, name), W, H)


def kind_of(scene, name):
    return camera(scene, name)["kind"]


# ---------------------------------------------------------------------------------------------
# perturbations of the oblique CornellBox meta: name -> (edit(meta) in place, expectation)
#   "changes"   the image differs from the oblique one's
#   "same"      it has the same bits (the kernels must not read the field, or read it the same way)
#   "dark"      every camera ray is non-finite: an all-miss image
# ---------------------------------------------------------------------------------------------
F = np.float32
UNUSED = list(range(11, 28)) + [44, 47]  # time, world_to_cam, samplesPerPixel, the pad


def _set(**kv):
    def edit(m):
        for k, v in kv.items():
            m[int(k[1:])] = v
    return edit


def _row4(m):
    m[28 + 3], m[28 + 7], m[28 + 11], m[28 + 15] = 0.05, -0.03, 0.02, 1.1


def _unused_nan(m):
    m[UNUSED] = np.nan


def _m_nan(m):
    m[28:44] = np.nan


PERTURBATIONS = {
    "focal0.25": (_set(m2=0.25), "changes"),
    "focal4": (_set(m2=4.0), "changes"),
    "cam3_0.5": (_set(m7=0.5), "changes"),
    "row4": (_row4, "changes"),
    "aspect2.5": (_set(m10=2.5), "changes"),
    "inv_wh": (_set(m8=1 / 64, m9=1 / 20), "changes"),
    "unused_nan": (_unused_nan, "same"),
    "direct0": (_set(m46=0.0), "same"),          # direct-only is meta[46] > 0
    "direct-0": (_set(m46=-0.0), "same"),
    "direct1e-30": (_set(m46=1e-30), "changes"),  # > 0: direct lighting only
    "rr0": (_set(m45=0.0), "changes"),
    "rr-0.5": (_set(m45=-0.5), "changes"),
    "rr1": (_set(m45=1.0), "changes"),
    "rr1.5": (_set(m45=1.5), "changes"),
    "rr_nan": (_set(m45=np.nan), "changes"),
    "rr1-ulp": (_set(m45=np.nextafter(F(1), F(0))), "changes"),
    "m_nan": (_m_nan, "dark"),
    "cam0_inf": (_set(m4=np.inf), "dark"),
}
# pairs whose images are the same: roulette never continues below 0, always from 1 on
RR_TWINS = [("rr0", "rr-0.5"), ("rr1", "rr1.5")]
NONFINITE = ["m_nan", "cam0_inf"]
PERT_SCENE = "CornellBox"


def perturbed(name):
    m = meta_of(PERT_SCENE, "oblique")
    PERTURBATIONS[name][0](m)
    return m


# ---------------------------------------------------------------------------------------------
# scene files with a catalogue camera, for the Node host
# ---------------------------------------------------------------------------------------------
def write_xml(scene, c, path):
    """A copy of the scene's XML at `path` (inside a scene_assets directory whose models/ the caller
    provides) with camera c written into it, %.17g so every double survives."""
    import re
    with open(os.path.join(ASSETS, scene + ".xml")) as f:
        xml = f.read()
    for tag in ("pos", "focus", "up"):
        xml, n = re.subn(r"<%s\b[^>]*/>" % tag, '<%s x="%.17g" y="%.17g" z="%.17g"/>' % ((tag,) + tuple(c[tag])), xml)
        assert n == 1, tag
    xml, n = re.subn(r"<heightangle\b[^>]*/>", '<heightangle v="%.17g"/>' % c["heightangle"], xml)
    assert n == 1
    with open(path, "w") as f:
        f.write(xml)
    return path


# up parallel to the view direction: make_meta raises; what the Node host does is recorded by
# tests/test_cam_cpu.py.  No parity case.
DEGENERATE_UP = cam((0, 4, 0), (0, 0, 0), up=(0, 1, 0))
