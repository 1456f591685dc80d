"""Ill-conditioned geometry on the host (tests/cond_scenes.py: scenes far from the origin, scaled,
flattened, with needles and degenerate faces, with one giant triangle), without a GPU:

- the re-encoder accepts every variant and sets the two scene-derived flags as the variants intend
  (SceneView::fast_rcp off only for `giant`; `slivers` is no mailbox scene, the moved and scaled
  CornellBox still is);
- the leaf chunks' skip rules (scripts/leafbvh_harness.cpp with its rays scaled to the leaf: uniform,
  aimed, grazing and surface-leaving families; the cone check and the second check) lose no hit of
  the sequential loop on the largest leaf of every boat variant and on the `slivers` fan's leaf;
- the oracle's renders of the variants, which tests/test_gpu_cond.py compares the kernels with, are
  worth comparing: at least half the pixels of the 3-frame render carry light (a pixel counts when
  its three channels are finite and not all zero; the accumulating render is the image the project
  delivers, one frame is a sample of it), and `small` makes the sphere's triangles fall under the
  triangle test's det < 1e-8: its image differs from the unscaled scene's where the sphere stood.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cond_scenes as cs
import oracle
from test_scene_layout import harness as layout_harness  # noqa: F401  (the fixture, built as there)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
IDS = [cs.case_id(v, s) for v, s in cs.CASES]


@pytest.fixture(scope="module")
def cond(tmp_path_factory):
    base = tmp_path_factory.mktemp("cond")
    return {cs.case_id(v, s): cs.pack(v, s, base) for v, s in cs.CASES}


# ---------------------------------------------------------------------------------------------
# layout facts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,scene", cs.CASES, ids=IDS)
def test_layout_flags(layout_harness, cond, variant, scene):  # noqa: F811
    out = layout_harness(cond[cs.case_id(variant, scene)].dir)
    assert out[0] == "rc 0", out[:2]
    line = [ln for ln in out if ln.startswith("leaf_min ")]
    assert len(line) == 1, out
    f = dict(zip(line[0].split()[0::2], line[0].split()[1::2]))
    assert f["fast_rcp"] == ("0" if variant == "giant" else "1"), line
    if variant == "slivers":
        assert f["mailbox"] == "0", line
    if scene == "CornellBox" and variant in ("far3", "far4", "small"):
        assert f["mailbox"] == "1", line


# ---------------------------------------------------------------------------------------------
# chunk rules
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_harness(tmp_path_factory):
    assert os.path.exists(HIPCC) or shutil.which("hipcc"), "no hipcc"
    exe = str(tmp_path_factory.mktemp("cond_leafbvh") / "leafbvh_harness")
    csrc = os.path.join(ROOT, "brown-cs2240-path-tracer_amd", "csrc")
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17",
                    "-ffp-contract=off", "-I", csrc, os.path.join(ROOT, "scripts", "leafbvh_harness.cpp"),
                    os.path.join(csrc, "pt_leafbvh.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def leaves_of(bvh):
    """[(entries, offset)] of the leaves a walk from the root meets."""
    out, stack = [], [6]
    while stack:
        q = stack.pop()
        for side in (0, 1):
            c = int(bvh[q + 2 + side])
            if bvh[c] == 1.0:
                out.append((int(bvh[c + 4]) // 4, c))
            else:
                stack.append(c)
    return out


def leaf_records(p, c, n):
    """The leaf at offset c as 48-byte Tri records (v0, e1 = v1 - v0, e2 = v2 - v0 in f32), and its
    entries' 1-based vertex numbers."""
    t, b = p.triangle_data, p.bvh_data
    vs = int(t[2])
    ent = b[c + 17: c + 17 + 4 * n].reshape(n, 4)[:, :3].astype(np.int64)
    idx = (ent - 1) * 3
    v = [np.stack([t[vs + idx[:, k] + a] for a in range(3)], axis=1) for k in range(3)]
    rec = np.zeros((n, 12), np.float32)
    rec[:, 0:3] = v[0]
    rec[:, 3:6] = (v[1] - v[0]).astype(np.float32)
    rec[:, 6:9] = (v[2] - v[0]).astype(np.float32)
    return rec, ent


CORNELL_VERTICES = 72  # CornellBox-Original.obj's; the fan's come after them

CHUNK_CASES = [cs.case_id(v, s) for v, s in cs.CASES if s == "MedievalBoat" or v == "slivers"]


@pytest.mark.parametrize("chunking", [("8", "0"), ("16", "16")], ids=["traversal-8", "pass-16-merged"])
@pytest.mark.parametrize("case", CHUNK_CASES)
def test_chunk_rules_on_conditioned_leaves(chunk_harness, cond, tmp_path, case, chunking):
    p = cond[case]
    leaves = leaves_of(p.bvh_data)
    if case.endswith("slivers"):  # the leaf with the most fan faces
        def fan_count(leaf):
            return int((leaf_records(p, leaf[1], leaf[0])[1].min(axis=1) > CORNELL_VERTICES).sum())
        n, c = max(leaves, key=fan_count)
        rec, ent = leaf_records(p, c, n)
        fan = ent.min(axis=1) > CORNELL_VERTICES
        area = np.linalg.norm(np.cross(rec[:, 3:6].astype(np.float64), rec[:, 6:9].astype(np.float64)), axis=1)
        # it mixes well-shaped faces with needles and exact degenerates
        assert fan.sum() >= 8 and (area[fan] == 0).any() and (area[fan] > 1e-3).any(), (n, fan.sum(), area[fan])
    else:
        n, c = max(leaves)
        assert n == 7327
        rec, _ = leaf_records(p, c, n)
    leaf = str(tmp_path / "leaf.bin")
    rec.tofile(leaf)
    r = subprocess.run([chunk_harness, leaf, *chunking, "scaled"], capture_output=True, text=True, timeout=600)
    counts = [int(m) for m in re.findall(r"mismatches (\d+)", r.stdout)]
    assert len(counts) == 8, r.stdout + r.stderr      # 4 ray families x (cone check, second check)
    assert counts == [0] * 8 and r.returncode == 0, r.stdout
    # the aimed and the grazing rays do hit the leaf
    hit = {int(f): int(h) for f, h in re.findall(r"family (\d) cone check: (\d+) of 2000 rays hit", r.stdout)}
    assert hit[1] >= 250 and hit[2] >= 250, r.stdout


# ---------------------------------------------------------------------------------------------
# the oracle's images of the variants
# ---------------------------------------------------------------------------------------------
_RENDERS = {}


def oracle_render(p, key, scene):
    if key not in _RENDERS:
        W, H = cs.size_of(scene)
        _RENDERS[key] = oracle.render(p.triangle_data, p.bvh_data, p.meta_for(W, H), 0, 3, 1, cs.DEPTH)[0]
    return _RENDERS[key]


def lit(img):
    return np.isfinite(img).all(axis=-1) & (img != 0).any(axis=-1)


@pytest.mark.parametrize("variant,scene", cs.CASES, ids=IDS)
def test_oracle_render_carries_light(cond, variant, scene):
    key = cs.case_id(variant, scene)
    share = float(lit(oracle_render(cond[key], key, scene)).mean())
    print(f"{key}: {share:.3f} of the pixels lit")
    assert share >= 0.5, share


def first_hits(p, k):
    """Material ids (-1: none) of the first hits of 40 x 32 rays from CornellBox.xml's camera position
    through a grid on the box's middle plane z = 0, the whole figure scaled by k."""
    cam = np.array([0.0, 1.0, 3.6])
    out = np.full((32, 40), -1, np.int64)
    for j in range(32):
        for i in range(40):
            d = np.array([-0.95 + 1.9 * (i + 0.5) / 40, 0.05 + 1.9 * (j + 0.5) / 32, 0.0]) - cam
            hit, o, _ = oracle.intersect(p.triangle_data, p.bvh_data, list(cam * k), list(d / np.linalg.norm(d)))
            if hit:
                out[j, i] = int(o[7])
    return out


def test_small_loses_the_sphere(cond, packed):
    """x 1.1e-3 scales every det = e1 . (d x e2) by 1.21e-6: the walls' (edges of 2 units) stay above the
    triangle test's 1e-8, the sphere's facets' (edges of a few hundredths) fall under it, so the
    sphere is gone.  Seen twice.  The image: the 3-frame render differs from the unscaled scene's in at
    least 5 % of the pixels (bit for bit; the radiance is not scale-free, so this alone would say
    little).  The first hits: rays from the camera through a grid on the box's middle plane end on
    another material in at least 5 % of the grid where the sphere stood, while in CornellBox, which
    has no sphere, the same rays end on the same material under the same scaling."""
    key = cs.case_id("small", "CornellBox-Sphere")
    small, orig = oracle_render(cond[key], key, "CornellBox-Sphere"), \
        oracle_render(packed["CornellBox-Sphere"], "CornellBox-Sphere", "CornellBox-Sphere")
    image = float((small.view(np.uint32) != orig.view(np.uint32)).any(axis=-1).mean())
    sphere = float((first_hits(cond[key], 1.1e-3) != first_hits(packed["CornellBox-Sphere"], 1.0)).mean())
    box = float((first_hits(cond[cs.case_id("small", "CornellBox")], 1.1e-3) != first_hits(packed["CornellBox"], 1.0)).mean())
    print(f"pixels differing from the unscaled scene: {image:.3f}; first hits on another material: "
          f"sphere scene {sphere:.3f}, box {box:.3f}")
    assert image >= 0.05 and sphere >= 0.05, (image, sphere)
    assert box == 0.0, box
