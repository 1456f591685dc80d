"""The scene re-encoder on the host (csrc/pt_scene_layout.cpp build_layout and plan_sections, run by
scripts/scene_layout_harness.cpp).  Most of what it decides — which leaves get chunks, the pre-resolved
table, the leaf remainders — changes the kernels' speed and not the image, so the bit-exact GPU suite
cannot see a slip there.  tests/golden/scene_layout.txt holds the harness's output ("== case", then its
lines: per array its length, element size and FNV-1a digest, the scalars, the device section plan) as
build_layout gave it while it stood inside the C ABI file; every line must match, no tolerance.  The
malformed inputs are CornellBox's buffers with one edit each; their code and message are recorded the
same way.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ALL_SCENES, SCENES, pack_with_node

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_layout.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# case id -> (scene, tree, harness arguments)
VALID = {s: (s, "reference", []) for s in ALL_SCENES}
VALID.update({
    "MedievalBoat-sah": ("MedievalBoat", "sah", []),
    "CornellBox-Glossy-sah": ("CornellBox-Glossy", "sah", []),
    "CornellBox-uid_reverse": ("CornellBox", "reference", ["uid_reverse"]),
    "CornellBox-Glossy-leaf_skip=0": ("CornellBox-Glossy", "reference", ["leaf_skip=0"]),
    "MedievalBoat-leaf_bvh=0": ("MedievalBoat", "reference", ["leaf_bvh=0"]),
    "MedievalBoat-leaf_bvh=64": ("MedievalBoat", "reference", ["leaf_bvh=64"]),
})


def _first_leaf(bvh):
    """Offset of the first leaf child a walk from the root (bvh[6]) meets."""
    stack = [6]
    while stack:
        q = stack.pop()
        for side in (0, 1):
            c = int(bvh[q + 2 + side])
            if bvh[c] == 1.0:
                return c
            stack.append(c)
    raise AssertionError("no leaf")


def _edit(f):
    def make(tri, bvh):
        tri, bvh = tri.copy(), bvh.copy()
        return f(tri, bvh) or (tri, bvh)
    return make


def _set(buf, idx, val):
    def f(tri, bvh):
        (tri if buf == "tri" else bvh)[idx] = val
    return _edit(f)


def _leaf_set(field, val):
    def f(tri, bvh):
        bvh[_first_leaf(bvh) + field] = val(tri, bvh) if callable(val) else val
    return _edit(f)


def _no_lights(tri, bvh):
    tri[8:16] = -1.0


# case id -> (tri, bvh) -> (tri, bvh): CornellBox's buffers with one edit
MALFORMED = {
    "triangle_data-15-floats": _edit(lambda tri, bvh: (tri[:15], bvh)),
    "bvh_data-22-floats": _edit(lambda tri, bvh: (tri, bvh[:22])),
    "vertex-count-not-integral": _edit(lambda tri, bvh: tri.__setitem__(0, tri[0] + 0.5)),
    "vertex-section-past-end": _edit(lambda tri, bvh: tri.__setitem__(2, float(len(tri) - 3))),
    "material-section-past-end": _edit(lambda tri, bvh: tri.__setitem__(4, float(len(tri) - 14))),
    "root-is-leaf": _set("bvh", 6, 1.0),
    "child-pointer-past-end": _edit(lambda tri, bvh: bvh.__setitem__(6 + 2, float(len(bvh) - 16))),
    "leaf-count-not-multiple-of-4": _leaf_set(4, lambda tri, bvh: bvh[_first_leaf(bvh) + 4] + 1.0),
    "leaf-entry-vertex-0": _leaf_set(17, 0.0),
    "leaf-entry-material-is-object-count": _leaf_set(17 + 3, lambda tri, bvh: tri[1]),
    "child-pointer-back-to-root": _edit(lambda tri, bvh: bvh.__setitem__(6 + 2, 6.0)),
    "no-emissive-ranges": _edit(_no_lights),
}


def read_golden():
    cases, cur = {}, None
    with open(GOLDEN) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("== "):
                cur = cases.setdefault(line[3:], [])
            elif line:
                cur.append(line)
    return cases


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    assert os.path.exists(HIPCC) or shutil.which("hipcc"), "no hipcc"
    exe = str(tmp_path_factory.mktemp("layout") / "scene_layout_harness")
    csrc = os.path.join(ROOT, "brown-cs2240-path-tracer_amd", "csrc")
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                    "-ffp-contract=off", "-I", csrc, os.path.join(ROOT, "scripts", "scene_layout_harness.cpp"),
                    *[os.path.join(csrc, n) for n in ("pt_scene_layout.cpp", "pt_leafbvh.cpp", "pt_leafskip.cpp")],
                    "-o", exe], check=True, capture_output=True)

    def run(d, *args):
        return subprocess.run([exe, os.path.join(d, "triangle_data.f32"), os.path.join(d, "bvh_data.f32"), *args],
                              check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def sah_packed(tmp_path_factory):
    base = tmp_path_factory.mktemp("layout_sah")
    return {s: pack_with_node(os.path.join(SCENES, "scene_assets", s + ".xml"), str(base / s), "--bvh", "sah")
            for s in ("MedievalBoat", "CornellBox-Glossy")}


@pytest.fixture(scope="module")
def golden():
    return read_golden()


def test_golden_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(list(VALID) + list(MALFORMED))


@pytest.mark.parametrize("case", list(VALID))
def test_layout_matches_the_recorded_one(harness, packed, sah_packed, golden, case):
    scene, tree, args = VALID[case]
    got = harness((sah_packed if tree == "sah" else packed)[scene].dir, *args)
    want = golden[case]
    assert got[0] == "rc 0" and len(want) > 20
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not bad, f"{len(bad)} lines differ; first (got, recorded): {bad[:3]}"


@pytest.mark.parametrize("case", list(MALFORMED))
def test_malformed_input_is_refused_as_recorded(harness, packed, golden, tmp_path, case):
    p = packed["CornellBox"]
    tri, bvh = MALFORMED[case](p.triangle_data, p.bvh_data)
    np.asarray(tri, np.float32).tofile(str(tmp_path / "triangle_data.f32"))
    np.asarray(bvh, np.float32).tofile(str(tmp_path / "bvh_data.f32"))
    got = harness(str(tmp_path))
    assert got == golden[case]
    assert got[0] == "rc -2" and got[1] != "msg []"  # PT_ERR_SCENE with a reason
    if case == "child-pointer-back-to-root":
        assert "not a tree" in got[1]
