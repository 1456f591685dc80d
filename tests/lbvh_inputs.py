"""Inputs of the LBVH tests (a helper module like tests/cond_scenes.py, not a conftest): packed
triangle_data buffers by name, and the numpy restatement of the key of include/pt_hip.h that the CPU
test checks the leaves' order with.  The scene inputs are packed by the Node host; the hand-made ones
are written here in the packer's layout (src/packer.ts:4-81)."""
import os
import sys

import numpy as np

import cond_scenes
from conftest import ALL_SCENES, ROOT, SCENES, pack_with_node

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import synth_scene  # noqa: E402

MAX_LEAVES = (1, 4, 8)
K_MAX_DEPTH = 28  # PT_LBVH_MAX_DEPTH


def triangle_data(verts, recs, ke, emissive=(0, 1), normals=()):
    """The packer's buffer for f32 vertices [n, 3], records [m, 4] (1-based indices, material) and one
    Ke triple per material.  emissive: (first record, count) of the one emissive range the header names
    (the light table reads the header, the builders' flags read Ke: tests set them apart)."""
    verts = np.asarray(verts, np.float32).reshape(-1)
    recs = np.asarray(recs, np.float32).reshape(-1)
    mats = np.concatenate([np.array([10, 1, 2, 0, 0, 0, .5, .5, .5, 0, 0, 0, *k], np.float32) for k in ke])
    i0 = 16 + verts.size
    m0 = i0 + recs.size
    head = np.array([verts.size // 3, len(ke), 16, i0, m0, m0 + mats.size, len(normals), 0,
                     i0 + 4 * emissive[0], i0 + 4 * (emissive[0] + emissive[1]), -1, -1, -1, -1, -1, -1], np.float32)
    out = np.concatenate([head, verts, recs, mats, np.asarray(normals, np.float32).reshape(-1)])
    return np.concatenate([out, np.zeros(16 - out.size % 16, np.float32)])


def _soup(rng, m, scale=1.0, flat_axis=None):
    tri = rng.uniform(-1, 1, (m, 3, 3)) * scale
    if flat_axis is not None:
        tri[:, :, flat_axis] = 0.25
    verts = tri.reshape(-1, 3)
    recs = np.stack([3 * np.arange(m) + 1, 3 * np.arange(m) + 2, 3 * np.arange(m) + 3, np.zeros(m, int)], 1)
    return verts, recs


def handmade():
    """name -> triangle_data of the degenerate and flag cases."""
    rng = np.random.default_rng(5)
    out = {}
    one = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    lit, dark = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    out["copies40"] = triangle_data(one, [[1, 2, 3, k % 3] for k in range(40)], [dark, lit, dark])
    out["single"] = triangle_data(one, [[1, 2, 3, 0]], [lit])
    m = 400
    c = np.stack([2.0 ** -(np.arange(m) / 8.0), np.zeros(m), np.zeros(m)], 1)
    tri = c[:, None, :] + rng.uniform(-1e-3, 1e-3, (m, 3, 3)) * (2.0 ** -(np.arange(m) / 8.0))[:, None, None]
    recs = np.stack([3 * np.arange(m) + 1, 3 * np.arange(m) + 2, 3 * np.arange(m) + 3, (np.arange(m) % 7 == 0).astype(int)], 1)
    out["shrinking400"] = triangle_data(tri.reshape(-1, 3), recs, [dark, lit])
    v, r = _soup(rng, 300, flat_axis=1)
    r[:, 3] = np.arange(300) % 2
    out["flat_axis"] = triangle_data(v, r, [dark, (0.0, 0.5, 0.0)])
    # a chain: small triangles in the grid cells whose Morton codes are 0 and the 30 powers of two (bounds
    # (0, 0, 0) .. (1024, 1024, 1024) from two vertices no record references), three to a cell: the radix tree
    # of the sorted codes is a comb 31 levels deep, past the depth cap
    cells = [(0, 0, 0)] + [tuple((1 << a) if ax == k else 0 for ax in range(3)) for a in range(10) for k in range(3)]
    tri = np.array([[np.add(c, 0.5) + rng.uniform(-0.2, 0.2, 3) for _ in range(3)] for c in cells for _ in range(3)])
    v = np.concatenate([tri.reshape(-1, 3), [[0, 0, 0], [1024, 1024, 1024]]])
    m = len(tri)
    r = np.stack([3 * np.arange(m) + 1, 3 * np.arange(m) + 2, 3 * np.arange(m) + 3, (np.arange(m) % 5 == 0).astype(int)], 1)
    out["chain"] = triangle_data(v, r, [dark, lit])
    v, r = _soup(rng, 150)
    out["all_flagged"] = triangle_data(v, r, [lit])
    out["none_flagged"] = triangle_data(v, r, [dark])
    return out


def restated_order(tri, isolate):
    """The records in the order the tree's leaves hold them, by a numpy restatement of include/pt_hip.h's
    key: (flagged records in record order or None, the others sorted by key)."""
    tri = np.asarray(tri, np.float32)
    nv, i0, m0 = int(tri[0]), int(tri[3]), int(tri[4])
    verts = tri[16:16 + 3 * nv].reshape(-1, 3)
    recs = tri[i0:m0].reshape(-1, 4).astype(np.int64)
    ke = tri[m0:m0 + 15 * int(tri[1])].reshape(-1, 15)[:, 12:15]
    flagged = ((ke[:, 0] + ke[:, 1]) + ke[:, 2] > 0)[recs[:, 3]]
    lo, hi = verts.min(0), verts.max(0)
    p = verts[recs[:, :3] - 1]
    c = (p.min(1) + p.max(1)) * np.float32(0.5)
    ext = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(ext > 0, np.float32(1024.0) / ext, np.float32(0)).astype(np.float32)
        x = ((c - lo) * inv).astype(np.float32)
    q = np.where(x >= 0, np.minimum(x, np.float32(1023.0)), 0).astype(np.uint64)
    morton = np.zeros(len(recs), np.uint64)
    for k in range(10):
        for axis, shift in ((0, 2), (1, 1), (2, 0)):
            morton |= ((q[:, axis] >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k + shift)
    key = morton << np.uint64(32) | np.arange(len(recs), dtype=np.uint64)
    iso = isolate and flagged.any() and not flagged.all()
    rest = np.flatnonzero(~flagged) if iso else np.arange(len(recs))
    rest = rest[np.argsort(key[rest], kind="stable")]
    return (recs[flagged] if iso else None), recs[rest]


def synth_packed(base, n, light_grid=1):
    d = os.path.join(str(base), f"synth_{n}_{light_grid}")
    return pack_with_node(synth_scene.write(n, d, light_grid), os.path.join(d, "packed"), "--native-bvh")


def scene_inputs(base, packed):
    """name -> conftest.Packed: the five scenes, CornellBox2 with all meshes, the synthetic ones, the
    288-emitter scene and the huge-triangle meshes."""
    out = {s: packed[s] for s in ALL_SCENES}
    out["CornellBox2-all"] = pack_with_node(os.path.join(SCENES, "scene_assets", "CornellBox2.xml"),
                                            os.path.join(str(base), "cb2"), "--all-meshes", "--native-bvh")
    for n in (36, 1000, 12500):
        out[f"synth{n}"] = synth_packed(base, n)
    out["emitters288"] = synth_packed(base, 1000, 12)
    for variant in ("giant", "nearly_giant"):
        out[variant] = cond_scenes.pack(variant, "CornellBox", base)
    return out
