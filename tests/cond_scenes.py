"""Ill-conditioned copies of the test scenes (a helper module like scripts/synth_scene.py, not a
conftest): write(scene, variant, out_root) writes OBJ + MTL + scene XML that the Node host packs
like any scene, and returns the XML's path.  Vertex positions are transformed in float64 and written
with %.9g (every f32 survives that); the camera's pos and focus go through the same map, `up` and
the height angle stay (the boat's camera is another than its XML's, and `flat` has one of its own:
CAMERAS says why).  The packer drops the XML's translation (parse-obj.js, as the reference), and
the scenes' rotations are by 0 degrees, so the OBJ's positions are the scene's.

Variants (CASES lists which scene gets which):
  far3          + (1000, -2000, 500)
  far4          + (10000, -20000, 5000): some of the boat's triangles collapse after f32 rounding
  big           x 1.1e3
  bigfar        x 37, then + (3000, 100, -7000)
  small         x 1.1e-3: the sphere's triangles fall under the triangle test's det < 1e-8, the
                walls do not
  flat          y x 1e-3: every triangle a sliver with a near-y normal
  slivers       CornellBox + a fan of FAN_BLADES faces around a hub in front of the boxes, in the
                camera's view: well-shaped blades, between them needles whose shape factor
                |e1 x e2| / (|e1||e2|) steps from 1e-2 down to 1e-7, three triangles of collinear
                vertices and two with a repeated vertex position.  With the box's entries that is
                more than 64 distinct ones: no mailbox scene, and leaf_bvh=2 chunks its leaves.
  giant         CornellBox + one diffuse triangle far below the floor with edges of about 2^63
                (max |e1||e2| = 2^126: SceneView::fast_rcp is 0)
  nearly_giant  the same with edges of about 2^61 (2^122 < 2^124: fast_rcp stays 1)

What the Node packer needed: nothing special for collinear vertices; the two repeated-position
faces use three distinct vertex indices, two of them at equal positions, so that no face repeats an
index.  Appended faces name their vertices by negative (relative) indices, which the parser resolves
at the face's line, so no earlier face changes its meaning.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "scenes", "scene_assets")

# scene -> OBJ path below scene_assets (the MTL lies next to it)
MODELS = {
    "CornellBox": "models/CornellBox/CornellBox-Original.obj",
    "CornellBox-Glossy": "models/CornellBox/CornellBox-Glossy.obj",
    "CornellBox-Sphere": "models/CornellBox/CornellBox-Sphere.obj",
    "MedievalBoat": "models/MedievalBoat/MedievalBoat.obj",
}

# variant -> (scale per axis, translation after it)
TRANSFORMS = {
    "far3": ((1.0, 1.0, 1.0), (1000.0, -2000.0, 500.0)),
    "far4": ((1.0, 1.0, 1.0), (10000.0, -20000.0, 5000.0)),
    "big": ((1.1e3, 1.1e3, 1.1e3), (0.0, 0.0, 0.0)),
    "bigfar": ((37.0, 37.0, 37.0), (3000.0, 100.0, -7000.0)),
    "small": ((1.1e-3, 1.1e-3, 1.1e-3), (0.0, 0.0, 0.0)),
    "flat": ((1.0, 1e-3, 1.0), (0.0, 0.0, 0.0)),
    "slivers": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "giant": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "nearly_giant": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
}

# (variant, scene) pairs under test, in the issue's order
CASES = [
    ("far3", "CornellBox"), ("far3", "CornellBox-Glossy"), ("far3", "CornellBox-Sphere"), ("far3", "MedievalBoat"),
    ("far4", "CornellBox"), ("far4", "MedievalBoat"),
    ("big", "CornellBox-Glossy"), ("big", "MedievalBoat"),
    ("bigfar", "MedievalBoat"), ("bigfar", "CornellBox-Sphere"),
    ("small", "CornellBox"), ("small", "CornellBox-Sphere"),
    ("flat", "MedievalBoat"),
    ("slivers", "CornellBox"), ("giant", "CornellBox"), ("nearly_giant", "CornellBox"),
]


# Cameras that replace the scene XML's.  By scene: in the scene's own space, moved with the mesh like
# the XML's would be.  By (scene, variant): in the variant's space, used as it stands.
#
# MedievalBoat.xml's camera stands 8 units from a mast-high, 1.5-unit-wide boat over a mirror ocean
# under a small light: at 24 x 16 only 8 % of a frame's pixels carry light (14 % of a 3-frame
# render's) in the untransformed scene, far below the tests' condition that half of them do.  The
# boat variants therefore look at the lit side of the sail from inside the rigging (62 % of a frame,
# 88 % of the render).  `flat` cannot take that camera through its map: it would look along the
# flattened boat's plane from 3 mm above it and see it in under 1 % of the pixels; its camera stands
# above the pancake and looks down at it (57 % / 77 %).
CAMERAS = {
    "MedievalBoat": {"pos": (1.32, 3.2, 1.96), "focus": (0.49, 2.07, 1.13), "heightangle": 60},
    ("MedievalBoat", "flat"): {"pos": (0.56, 0.46, 2.01), "focus": (0.66, 0.0, 2.05), "heightangle": 45},
}


def case_id(variant, scene):
    return f"{scene}-{variant}"


# ---------------------------------------------------------------------------------------------
# appended faces
# ---------------------------------------------------------------------------------------------
FAN_HUB = np.array([0.05, 1.05, 0.78])
FAN_RADIUS = 0.55
FAN_GOOD = 28            # well-shaped blades
NEEDLE_SHAPES = [10.0 ** (-0.5 * k) for k in range(4, 15)]  # 1e-2, 3.2e-3, ... 1e-7: 11 needles
FAN_BLADES = FAN_GOOD + len(NEEDLE_SHAPES) + 3 + 2          # 44 faces
FAN_MATERIAL = "shortBox"                                   # white, diffuse


def fan_faces():
    """[(3 x 3 float64 positions, kind)] of the fan: slot j of FAN_BLADES equal sectors around the
    hub holds a blade in the plane through the hub whose normal is the view axis z tipped by 0.35 rad
    about the blade's own direction (a propeller, so the blades share no plane).  Two slots in
    three hold a well-shaped blade (0.8 of the sector wide), the others a needle (the sector's
    direction and one at the angle asin(shape) from it, both of the full radius), a collinear
    triangle (hub, mid-point, tip) or one whose last two vertices coincide."""
    kinds = ["good"] * FAN_GOOD + [("needle", s) for s in NEEDLE_SHAPES] + ["collinear"] * 3 + ["repeat"] * 2
    # interleave: every third slot a bad face while they last, so every neighbourhood mixes them
    good = [k for k in kinds if k == "good"]
    bad = [k for k in kinds if k != "good"]
    order = []
    while good or bad:
        for _ in range(2):
            if good:
                order.append(good.pop())
        if bad:
            order.append(bad.pop(0))
    assert len(order) == FAN_BLADES
    out = []
    for j, kind in enumerate(order):
        phi = 2.0 * np.pi * j / FAN_BLADES
        u = np.array([np.cos(phi), np.sin(phi), 0.0])          # the blade's direction, in the view plane
        w = np.array([-np.sin(phi), np.cos(phi), 0.0])
        side = np.cos(0.35) * w + np.sin(0.35) * np.array([0.0, 0.0, 1.0])  # in the tipped plane, normal to u
        tip = FAN_HUB + FAN_RADIUS * u

        def at(angle):
            return FAN_HUB + FAN_RADIUS * (np.cos(angle) * u + np.sin(angle) * side)
        if kind == "good":
            tri = [FAN_HUB, tip, at(0.8 * 2.0 * np.pi / FAN_BLADES)]
        elif kind == "collinear":
            tri = [FAN_HUB, FAN_HUB + 0.5 * FAN_RADIUS * u, tip]
        elif kind == "repeat":
            tri = [FAN_HUB, tip, tip]
        else:
            tri = [FAN_HUB, tip, at(np.arcsin(kind[1]))]
            kind = "needle"
        out.append((np.array(tri), kind))
    return out


GIANT_EDGE = {"giant": 2.0 ** 63, "nearly_giant": 2.0 ** 61}


def giant_face(variant):
    """One right triangle with legs of GIANT_EDGE along x and z, its corner at -edge / 4 in both, far
    below the floor (y = -edge / 64, so no path from inside the box's bounds is near it)."""
    e = GIANT_EDGE[variant]
    v0 = np.array([-0.25 * e, -e / 64.0, -0.25 * e])
    return np.array([v0, v0 + np.array([e, 0.0, 0.0]), v0 + np.array([0.0, 0.0, e])])


def _appended(variant):
    """OBJ text appended for the identity variants."""
    if variant == "slivers":
        faces = [t for t, _ in fan_faces()]
    elif variant in GIANT_EDGE:
        faces = [giant_face(variant)]
    else:
        return ""
    lines = ["", "g " + variant, "usemtl " + FAN_MATERIAL]
    for tri in faces:
        lines += ["v %.9g %.9g %.9g" % tuple(p) for p in tri]
        lines.append("f -3 -2 -1")
    return "\n".join(lines) + "\n"


# ---------------------------------------------------------------------------------------------
def transform(variant, p):
    s, t = TRANSFORMS[variant]
    return np.asarray(p, np.float64) * np.array(s) + np.array(t)


def _camera(xml, scene, variant):
    cam = CAMERAS.get((scene, variant)) or CAMERAS.get(scene)

    def move(m):
        tag, rest = m.group(1), m.group(2)
        if (scene, variant) in CAMERAS:
            q = cam[tag]  # given in the variant's own space
        else:
            p = cam[tag] if cam else [float(re.search(r'\b%s="([^"]*)"' % a, rest).group(1)) for a in "xyz"]
            q = transform(variant, p)
        return '<%s x="%.17g" y="%.17g" z="%.17g"/>' % (tag, q[0], q[1], q[2])
    out, n = re.subn(r"<(pos|focus)\b([^>]*)/>", move, xml)
    assert n == 2
    if cam:
        out, n = re.subn(r"<heightangle\b[^>]*/>", '<heightangle v="%g"/>' % cam["heightangle"], out)
        assert n == 1
    return out


def write(scene: str, variant: str, out_root: str) -> str:
    """OUT_ROOT/scene_assets/<scene>-<variant>.xml (+ the OBJ and MTL under its models/ path)."""
    rel = MODELS[scene]
    assets = os.path.join(out_root, "scene_assets")
    os.makedirs(os.path.join(assets, os.path.dirname(rel)), exist_ok=True)
    with open(os.path.join(ASSETS, rel)) as f:
        obj = f.read()

    def vertex(m):
        q = transform(variant, [float(x) for x in m.group(2).split()[:3]])
        return "%s%.9g %.9g %.9g" % (m.group(1), q[0], q[1], q[2])
    obj = re.sub(r"^(v\s+)([^\n#]*)", vertex, obj, flags=re.M)
    with open(os.path.join(assets, rel), "w") as f:
        f.write(obj.rstrip("\n") + "\n" + _appended(variant))
    with open(os.path.join(ASSETS, rel[:-3] + "mtl")) as f:
        mtl = f.read()
    with open(os.path.join(assets, rel[:-3] + "mtl"), "w") as f:
        f.write(mtl)
    with open(os.path.join(ASSETS, scene + ".xml")) as f:
        xml = _camera(f.read(), scene, variant)
    path = os.path.join(assets, case_id(variant, scene) + ".xml")
    with open(path, "w") as f:
        f.write(xml)
    return path


def pack(variant: str, scene: str, base: str, *extra):
    """The variant written under base/<case id> and packed by the Node host (conftest.Packed)."""
    from conftest import pack_with_node
    d = os.path.join(str(base), case_id(variant, scene))
    return pack_with_node(write(scene, variant, d), os.path.join(d, "packed" + "".join(extra).replace("-", "_")), *extra)


def size_of(scene: str):
    """(W, H) of the conditioned renders: the smallest sizes tests/test_gpu_parity.py's frame cases use."""
    return (24, 16) if scene == "MedievalBoat" else (40, 32)


DEPTH = 8


if __name__ == "__main__":
    import sys
    print(write(sys.argv[1], sys.argv[2], sys.argv[3]))
