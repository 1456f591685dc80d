"""Kernels against the oracle on ill-conditioned geometry (tests/cond_scenes.py): the test scenes
1e3 and 1e4 units from the origin, scaled by 1.1e3, 1.1e-3 and 37, flattened, with a fan of needles
and degenerate faces, and with one triangle of 2^63-unit edges.  tests/test_gpu_parity.py's bit-exact
claims rest on coordinates of order 1 to 10 and well-shaped triangles; the leaf chunks' skip rules
(a first-order rounding bound with absolute slack constants), SceneView::fast_rcp (a scene-derived
flag) and the triangle test's absolute 1e-8 are the code such inputs could break.  Bar: bit-exact,
counters equal, as there.  tests/test_cond_cpu.py checks on the oracle alone that the images are
worth comparing.

Renders: per variant one frame (salt 3) and a 3-frame render, counted and uncounted, through the
kernel sets KSETS, and once more on the SAH tree.  Device walks: tests/test_gpu_leafbvh.py's checks
of chunk_leaf / chunk_leaf_multi and of the leaf pass's walks against the sequential loop, on the
boat variants' leaves of >= 64 entries and on every leaf of `slivers` and of the far4 / small
CornellBox; the loop itself must take a hit for at least one ray in eight of the aimed and the
grazing family on every leaf of >= 16 entries, or the walks were compared on misses only.
"""
import numpy as np
import pytest

import cond_scenes as cs
import pt_amd
from test_gpu_leafbvh import _check, _check_pass
from test_gpu_parity import mismatch_report, same_bits
from test_gpu_step_narrow import oracle_frame, oracle_render

pytestmark = pytest.mark.gpu

IDS = [cs.case_id(v, s) for v, s in cs.CASES]

# written as test_gpu_parity.py's KERNELS
KSETS = {
    "auto": {},
    "mega": {"PT_KERNEL": "mega"},
    "wavefront": {"PT_KERNEL": "wavefront"},
    "wavefront_nofuse": {"PT_KERNEL": "wavefront", "PT_FUSE": "0"},
    "wavefront_div": {"PT_KERNEL": "wavefront", "PT_FASTRCP": "0"},
    "wavefront_leaf2_nopre": {"PT_KERNEL": "wavefront", "PT_MAILBOX": "0", "PT_LEAF_BVH": "2", "PT_LEAF_PRE": "0"},
    "wavefront_leaf2_pairs_always_1block": {"PT_KERNEL": "wavefront", "PT_MAILBOX": "0", "PT_LEAF_BVH": "2",
                                            "PT_LEAF_PRE": "1", "PT_LEAF_PAIRS": "2", "PT_LEAF_BLOCKS": "1"},
    "wavefront_big8": {"PT_KERNEL": "wavefront", "PT_BIG_LEAF": "8", "PT_MAILBOX": "0"},
    "wavefront_noskip": {"PT_KERNEL": "wavefront", "PT_LEAF_SKIP": "0"},
    "wavefront_nopool_nomailbox": {"PT_KERNEL": "wavefront", "PT_LEAF_POOL": "0", "PT_MAILBOX": "0"},
    "mega_leaf4_lean4": {"PT_KERNEL": "mega", "PT_LEAF_BVH": "4", "PT_TRAV": "lean4", "PT_MAILBOX": "0"},
}


@pytest.fixture(scope="module")
def cond(tmp_path_factory):
    base = tmp_path_factory.mktemp("cond")
    return {cs.case_id(v, s): cs.pack(v, s, base) for v, s in cs.CASES}


@pytest.fixture(scope="module")
def cond_sah(tmp_path_factory):
    base = tmp_path_factory.mktemp("cond_sah")
    return {cs.case_id(v, s): cs.pack(v, s, base, "--bvh", "sah") for v, s in cs.CASES}


def check_renders(p, key, scene):
    W, H = cs.size_of(scene)
    meta = p.meta_for(W, H)
    ref = oracle_frame(p, key, meta, 3, cs.DEPTH)
    racc, rc = oracle_render(p, key, meta, 3, cs.DEPTH)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        gpu = s.frame(meta, 3, cs.DEPTH)
        acc, gc = s.render(meta, 0, 3, 1, cs.DEPTH, pt_amd.MODE_AUTO, counters=True)
        plain = s.render(meta, 0, 3, 1, cs.DEPTH, pt_amd.MODE_AUTO)
    assert same_bits(gpu, ref), f"{key} frame: " + mismatch_report(gpu, ref)
    assert same_bits(acc, racc), f"{key} counted render: " + mismatch_report(acc, racc)
    assert same_bits(plain, racc), f"{key} render: " + mismatch_report(plain, racc)
    assert gc == rc, (gc, rc)


@pytest.mark.parametrize("kset", list(KSETS))
@pytest.mark.parametrize("variant,scene", cs.CASES, ids=IDS)
def test_conditioned_renders_bitexact(cond, ptopts, variant, scene, kset):
    for k, v in KSETS[kset].items():
        ptopts.set(k, v)
    key = cs.case_id(variant, scene)
    check_renders(cond[key], "cond-" + key, scene)


@pytest.mark.parametrize("variant,scene", cs.CASES, ids=IDS)
def test_conditioned_renders_bitexact_sah(cond_sah, ptopts, variant, scene):
    key = cs.case_id(variant, scene)
    check_renders(cond_sah[key], "cond-sah-" + key, scene)


# ---------------------------------------------------------------------------------------------
# device walks
# ---------------------------------------------------------------------------------------------
NRAYS = 1 << 13
WALKS = [(v, s, "64" if s == "MedievalBoat" else "2") for v, s in cs.CASES
         if s == "MedievalBoat" or v == "slivers" or (s == "CornellBox" and v in ("far4", "small"))]


def leaf_sizes(bvh):
    """Entries of the leaves a walk from the root meets, largest first (the order of the pre-resolvable leaves)."""
    out, stack = [], [6]
    while stack:
        q = stack.pop()
        for side in (0, 1):
            c = int(bvh[q + 2 + side])
            if bvh[c] == 1.0:
                out.append(int(bvh[c + 4]) // 4)
            else:
                stack.append(c)
    return sorted(out, reverse=True)


@pytest.mark.parametrize("variant,scene,leaf_bvh", WALKS, ids=[cs.case_id(v, s) for v, s, _ in WALKS])
def test_conditioned_leaf_walks_equal_loop(cond, ptopts, variant, scene, leaf_bvh):
    key = cs.case_id(variant, scene)
    p = cond[key]
    ptopts.set("leaf_bvh", leaf_bvh)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        stats = _check(s, key, nrays=NRAYS)
        nb, done = _check_pass(s, key, nrays=NRAYS)
    sizes = leaf_sizes(p.bvh_data)
    # the reference side: what the sequential loop took, families 1 (aimed) and 2 (grazing)
    walk = [(n, mode, hits) for _, n, _, mode, hits, _, _ in stats if n >= 16 and mode in (1, 2)]
    passes = [(sizes[b], fam, hits) for b, _, fam, hits in done if sizes[b] >= 16 and fam in (1, 2)]
    assert walk and passes, (stats, done)
    low = [x for x in walk + passes if 8 * x[2] < NRAYS]
    print(f"{key}: loop hits of {NRAYS} rays (entries, family, hits): walks {sorted(set(walk))[:16]} "
          f"pass {sorted(set(passes))[:16]}")
    assert not low, low
