"""Lights and materials the five test scenes never use (a helper module like tests/cond_scenes.py,
not a conftest).  Two kinds of input:

Light variants of CornellBox: OBJ + MTL + scene XML that the Node host packs like any scene
(write_light / pack_light).  The scenes under test all have one emissive object of two triangles:
Ntri = 2, inv_ntri = 0.5 exactly, header ranges 2..4 unused.  The variants change the number of
emissive triangles and of listed ranges:

  one_tri          the light's quad replaced by its first triangle                         Ntri 1
  fan3 fan5 fan7   the light replaced by a fan of 3 / 5 / 7 triangles in its footprint          3 5 7
  two_objects      light + l2                                                                    3
  four_objects     light + l2 + l3 + l4: all four header ranges used                            11
  five_objects     four_objects + l5, a fifth emissive object the packer does not list          11
  emitter_first    the light's section moved in front of the floor's: range 1 starts at the
                   first object                                                                  2
  listed_but_dark  two_objects with l2's Ke = (2, -3, 0.5): listed by the packer (some
                   component > 0), no emitter to the shader (the components' sum is < 0)        3

fan(c, u, v, n) is n triangles (c, c + cos a_j u + sin a_j v, c + cos a_(j+1) u + sin a_(j+1) v),
a_j = 2 pi j / max(n, 3).  The added emitters (EMITTERS) use Ns 10, illum 2, Kd 0.5, Ks 0 and have
their own usemtl section after the scene's faces; vertices are written with %.9g, faces as
f -3 -2 -1 (relative indices: no earlier face changes its meaning).  l5 is one triangle on the back
wall, right of l3 and above what the short box hides, where the camera sees it (on the floor in
front of the boxes it has no first-hit pixel at 40 x 32).

Material tables: patches of the 15-float material records (Ns Ni illum Ka Kd Ks Ke) in a packed
triangle_data, at tri[4] + 15 * object (apply).  Ke is left alone.  No parser is involved, so
non-finite values get through.  TABLES patches the packed five_objects variant (objects 0..6 =
OBJECTS), SPHERE_TABLES the packed CornellBox-Sphere (object 0 the mirror sphere, 1 the glass one).
`up` / `dn` are nextafter in f32.

    python tests/shade_scenes.py      searches all 2^32 seeds for those whose hash1(seed * 7 + 11) is
                                      exactly 1.0 (128 of them; HASH1_ONE_SEEDS holds eight)
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "scenes", "scene_assets")
MODEL = "models/CornellBox/CornellBox-Original"

W, H, DEPTH, SALT = 40, 32, 8, 3

LIGHT_VARIANTS = ["one_tri", "fan3", "fan5", "fan7", "two_objects", "four_objects", "five_objects", "emitter_first",
                  "listed_but_dark"]
# variant -> Ntri, and the number of header ranges in use
NTRI = {"one_tri": 1, "fan3": 3, "fan5": 5, "fan7": 7, "two_objects": 3, "four_objects": 11, "five_objects": 11,
        "emitter_first": 2, "listed_but_dark": 3}
RANGES = {"one_tri": 1, "fan3": 1, "fan5": 1, "fan7": 1, "two_objects": 2, "four_objects": 4, "five_objects": 4,
          "emitter_first": 1, "listed_but_dark": 2}
# CornellBox's objects in the packer's order (usemtl sections with faces); the light is object 7
OBJECTS = ["floor", "ceiling", "backWall", "rightWall", "leftWall", "shortBox", "tallBox"]
LIGHT_OBJECT = 7

ADDED = {"two_objects": ["l2"], "four_objects": ["l2", "l3", "l4"], "five_objects": ["l2", "l3", "l4", "l5"],
         "listed_but_dark": ["l2"]}
DARK_KE = (2, -3, 0.5)

# the light's footprint is x in [-0.24, 0.23], z in [-0.22, 0.16] at y = 1.98; u x v points down like the quad's normal
LIGHT_FAN = ((-0.005, 1.98, -0.03), (0, 0, -0.18), (0.18, 0, 0))


def fan(c, u, v, n):
    """[n, 3, 3] float64."""
    c, u, v = (np.asarray(x, np.float64) for x in (c, u, v))
    a = [2.0 * np.pi * j / max(n, 3) for j in range(n + 1)]
    return np.array([[c, c + np.cos(a[j]) * u + np.sin(a[j]) * v, c + np.cos(a[j + 1]) * u + np.sin(a[j + 1]) * v]
                     for j in range(n)])


def _faces(tris):
    lines = []
    for t in tris:
        lines += ["v %.9g %.9g %.9g" % tuple(p) for p in t]
        lines.append("f -3 -2 -1")
    return lines


def written_triangles(tris):
    """The triangles as the packer reads them back: %.9g text, parsed, rounded to f32."""
    return np.array([[[float("%.9g" % x) for x in p] for p in t] for t in tris]).astype(np.float32)


# name -> (Ke, its triangles): fans but for l5, one triangle on the back wall between l3 and the right wall,
# above what the short box hides, facing the camera like l3 (about 15 pixels of 40 x 32)
EMITTERS = {
    "l2": ((5, 9, 3), fan((-1.0, 1.0, 0.0), (0, .25, 0), (0, 0, -.25), 1)),      # left wall
    "l3": ((0, 0, 8), fan((0, 1.2, -1.03), (.3, 0, 0), (0, .3, 0), 3)),          # back wall
    "l4": ((12, 1, 1), fan((.98, 1.0, 0), (0, .25, 0), (0, 0, .25), 5)),         # right wall
    "l5": ((3, 3, 3), np.array([[[0.36, 0.75, -1.03], [0.98, 0.75, -1.03], [0.98, 1.95, -1.03]]])),
}


_LIGHT_SECTION = re.compile(r"((?:v[ \t][^\n]*\n){4})\s*g light\s*\nusemtl light\s*\nf -4 -3 -2 -1\s*$")


def light_obj(variant, obj):
    """CornellBox-Original.obj's text changed into the variant's."""
    m = _LIGHT_SECTION.search(obj)
    assert m, "the light's section is the OBJ's last"
    head, quad = obj[:m.start()], m.group(1)
    section = quad + "\ng light\nusemtl light\nf -4 -3 -2 -1\n"
    if variant == "one_tri":
        return head + quad + "\ng light\nusemtl light\nf -4 -3 -2\n"
    if variant.startswith("fan"):
        return head + "\n".join(["g light", "usemtl light"] + _faces(fan(*LIGHT_FAN, int(variant[3:])))) + "\n"
    if variant == "emitter_first":
        k = head.index("## Object floor")
        return head[:k] + section + "\n" + head[k:]
    lines = []
    for name in ADDED[variant]:
        lines += ["", "g " + name, "usemtl " + name] + _faces(EMITTERS[name][1])
    return head + section + "\n".join(lines) + "\n"


def light_mtl(variant, mtl):
    out = [mtl.rstrip("\n"), ""]
    for name in ADDED.get(variant, []):
        ke = DARK_KE if variant == "listed_but_dark" else EMITTERS[name][0]
        out += ["newmtl " + name, "  Ns 10", "  Ni 1", "  illum 2", "  Ka 0.5 0.5 0.5", "  Kd 0.5 0.5 0.5", "  Ks 0 0 0",
                "  Ke %g %g %g" % tuple(ke), ""]
    return "\n".join(out) + "\n"


def write_light(variant: str, out_root: str) -> str:
    """OUT_ROOT/scene_assets/CornellBox.xml (+ the OBJ and MTL under its models/ path)."""
    assets = os.path.join(out_root, "scene_assets")
    os.makedirs(os.path.join(assets, os.path.dirname(MODEL)), exist_ok=True)
    with open(os.path.join(ASSETS, MODEL + ".obj")) as f:
        obj = light_obj(variant, f.read())
    with open(os.path.join(assets, MODEL + ".obj"), "w") as f:
        f.write(obj)
    with open(os.path.join(ASSETS, MODEL + ".mtl")) as f:
        mtl = light_mtl(variant, f.read())
    with open(os.path.join(assets, MODEL + ".mtl"), "w") as f:
        f.write(mtl)
    with open(os.path.join(ASSETS, "CornellBox.xml")) as f:
        xml = f.read()
    path = os.path.join(assets, "CornellBox.xml")
    with open(path, "w") as f:
        f.write(xml)
    return path


def pack_light(variant: str, base):
    """The variant written under base/<variant> and packed by the Node host (conftest.Packed)."""
    from conftest import pack_with_node
    d = os.path.join(str(base), variant)
    return pack_with_node(write_light(variant, d), os.path.join(d, "packed"))


# ---------------------------------------------------------------------------------------------
# material tables
# ---------------------------------------------------------------------------------------------
F = np.float32
INF, NAN = F(np.inf), F(np.nan)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def dn(x):
    return np.nextafter(F(x), F(-np.inf))


def _row(**kw):
    """Fields of one object's patch: scalars Ns / illum, colours Kd / Ks as one number (all three
    channels) or three."""
    return {k: (tuple(v) if isinstance(v, tuple) else v) for k, v in kw.items()}


TABLES = {
    "phong_ns": [_row(Ks=.4, Ns=ns) for ns in (0, 1, 10, 17.5, dn(40), up(40), 500)],
    "ns40": [_row(Ns=40, Ks=0), _row(Ns=40, Ks=(.5, 0, 0)), _row(Ns=40, Ks=.5, Kd=0), _row(Ns=40, Ks=.3, Kd=1.5),
             _row(Ns=40, Ks=.9), _row(Ns=40, Ks=(.1, .2, .3)), _row(Ns=40, Ks=(0, 0, .7))],
    "mirror_edge": [_row(Ns=up(500)), _row(Ns=500, Ks=.5), _row(Ns=1e6), _row(Ns=INF), _row(Ns=10, illum=5),
                    _row(Ns=1000, Ks=.9), _row()],
    "glass": [_row(), _row(), _row(illum=7), _row(illum=7, Ns=1000), _row(illum=up(7)), _row(illum=7, Ks=.3, Ns=200),
              _row(illum=7)],
    "dark": [_row(Kd=0), _row(), _row(Ks=(.5, -.3, -.3), Ns=20), _row(Kd=(-.5, .5, .5)), _row(Kd=0, Ks=0), _row(),
             _row(Kd=(.9, 0, 0))],
    "wild": [_row(Ns=-1, Ks=.4), _row(Ns=NAN, Ks=.4), _row(Ns=-40, Ks=.2), _row(), _row(Ns=NAN), _row(illum=NAN),
             _row(Ns=3e38, Ks=.1)],
}

# the pools the random tables draw from: every value the tables above use
POOLS = {
    "Ns": [0, 1, 10, 17.5, 20, dn(40), 40, up(40), 200, 500, up(500), 1000, 1e6, INF, -1, -40, 3e38, NAN],
    "illum": [2, 5, 7, up(7), NAN],
    "Kd": [None, 0, 1.5, (-.5, .5, .5), (.9, 0, 0)],
    "Ks": [0, .1, .2, .3, .4, .5, .9, (.5, 0, 0), (.1, .2, .3), (0, 0, .7), (.5, -.3, -.3)],
}
# seeds whose tables keep the oracle's frame finite and lit (tests/test_shade_cpu.py's conditions; of the seeds
# 0..59, 25 do), among them those that draw the most negative and non-finite parameters
RANDOM_SEEDS = {"random0": 3, "random1": 9, "random2": 10, "random3": 24}


def random_table(seed):
    """Per object one draw of every field from POOLS (Kd None: unchanged)."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in OBJECTS:
        r = {k: POOLS[k][int(rng.integers(len(POOLS[k])))] for k in ("Ns", "illum", "Kd", "Ks")}
        rows.append({k: v for k, v in r.items() if v is not None})
    return rows


for _name, _seed in RANDOM_SEEDS.items():
    TABLES[_name] = random_table(_seed)

SPHERE_TABLES = {
    "s1": [_row(Ns=17.5, Ks=.95), _row(Ns=1000)],  # the second keeps its illum 7
    "s2": [_row(illum=7), _row(illum=2, Ns=40, Ks=.3)],
    "s3": [_row(illum=2, Ns=0, Ks=.5), _row(illum=2, Ns=0, Ks=.5)],
}

_OFFSET = {"Ns": 0, "illum": 2, "Kd": 6, "Ks": 9}


def apply(tri, rows):
    """A copy of the packed triangle_data with rows[i] patched into object i's material record."""
    tri = np.array(tri, np.float32)
    m0 = int(tri[4])
    for i, row in enumerate(rows):
        for k, v in row.items():
            o = m0 + 15 * i + _OFFSET[k]
            if k in ("Kd", "Ks"):
                tri[o:o + 3] = np.asarray(v, np.float32)  # one number: all three channels
            else:
                tri[o] = F(v)
    return tri


class Patched:
    """A conftest.Packed with another triangle_data (written to d when the layout harness needs files)."""

    def __init__(self, p, tri, d=None):
        self.triangle_data, self.bvh_data, self.meta, self.info = tri, p.bvh_data, p.meta, p.info
        self.meta_for = p.meta_for
        self.dir = d
        if d is not None:
            os.makedirs(d, exist_ok=True)
            tri.tofile(os.path.join(d, "triangle_data.f32"))
            p.bvh_data.tofile(os.path.join(d, "bvh_data.f32"))


def all_cases(lights, sphere, base=None):
    """name -> scene of everything under test: lights = {variant: Packed}, sphere = the packed
    CornellBox-Sphere.  base: a directory for the patched buffers' files (None: none written)."""
    out = dict(lights)
    for name, rows in TABLES.items():
        out[name] = Patched(lights["five_objects"], apply(lights["five_objects"].triangle_data, rows),
                            base and os.path.join(str(base), name))
    for name, rows in SPHERE_TABLES.items():
        out[name] = Patched(sphere, apply(sphere.triangle_data, rows), base and os.path.join(str(base), name))
    return out


CASES = LIGHT_VARIANTS + list(TABLES) + list(SPHERE_TABLES)

# ---------------------------------------------------------------------------------------------
# seeds whose hash1(seed * 7 + 11) is exactly 1.0f: sample_area_lights draws k = Ntri with them.
# hash1(n) = 1 - f32(mix(n) & 0x7fffffff) / 2^31 is 1.0 when the masked value is <= 64 (the
# quotient is then <= 2^-25, half an ulp below 1, and the tie rounds to even): 65 of 2^31 values.
# ---------------------------------------------------------------------------------------------
HASH1_ONE_SEEDS = [35246946, 73028306, 196800826, 203894572, 214545687, 226608965, 4175569787, 4240068968]


def hash1_masked(n):
    """mix(n) & 0x7fffffff for a uint32 array (hash.wgsl's integer hash, wrapping arithmetic)."""
    n = np.asarray(n, np.uint32)
    with np.errstate(over="ignore"):
        n = (n << np.uint32(13)) ^ n
        return (n * (n * n * np.uint32(15731) + np.uint32(789221)) + np.uint32(1376312589)) & np.uint32(0x7fffffff)


def search_hash1_one(limit=1 << 32, chunk=1 << 24):
    found = []
    for s0 in range(0, limit, chunk):
        seeds = np.arange(s0, min(s0 + chunk, limit), dtype=np.uint64).astype(np.uint32)
        with np.errstate(over="ignore"):
            u = hash1_masked(seeds * np.uint32(7) + np.uint32(11))
        found += [int(s) for s in seeds[u <= 64]]
    return found


if __name__ == "__main__":
    print(search_hash1_one())
