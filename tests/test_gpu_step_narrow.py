"""The fused step kernel's narrow instance (32-bit sets + subtree pruning in the stackless replay,
scenes of <= 32 distinct entries and <= 32 internal nodes) against the CPU oracle.  Bar: bit-exact,
as tests/test_gpu_parity.py.

Which instance ran is read from pt_amd._lib.last_bf_width() (32 narrow, 64 wide, 0 the counting
instances); the scenes' entry and node counts are taken from the packed BVH on the CPU.
"""
import os
import re
import shutil
import sys

import numpy as np
import pytest

import oracle
import pt_amd
from pt_amd import _lib

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """Bitwise equality, treating every NaN as equal to every NaN."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def report(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad = np.argwhere(~((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
    return f"{len(bad)} mismatches; first {bad[:5].tolist()}"


def tree_facts(bvh):
    """(distinct leaf entries, internal nodes) of a packed bvh_data: the tree from offset 6, 17-float
    nodes with child offsets at +2 / +3, a leaf's (i0, i1, i2, material) entries after its header."""
    entries, nodes, work = set(), 0, [6]
    while work:
        o = work.pop()
        nodes += 1
        for c in (int(bvh[o + 2]), int(bvh[o + 3])):
            if bvh[c] == 1.0:
                n = int(bvh[c + 4]) // 4
                for k in range(n):
                    entries.add(tuple(int(x) for x in bvh[c + 17 + 4 * k: c + 21 + 4 * k]))
            else:
                work.append(c)
    return len(entries), nodes


def _cornell_variant(tmp_path_factory, name, edit):
    """CornellBox packed from a copy of its OBJ changed by edit(text)."""
    from conftest import SCENES, pack_with_node
    base = tmp_path_factory.mktemp(name)
    src = os.path.join(SCENES, "scene_assets")
    dst = base / "scene_assets"
    dst.mkdir()
    shutil.copy(os.path.join(src, "CornellBox.xml"), dst / "CornellBox.xml")
    mdir = dst / "models" / "CornellBox"
    mdir.mkdir(parents=True)
    shutil.copy(os.path.join(src, "models", "CornellBox", "CornellBox-Original.mtl"), mdir)
    with open(os.path.join(src, "models", "CornellBox", "CornellBox-Original.obj")) as f:
        obj = f.read()
    with open(mdir / "CornellBox-Original.obj", "w") as f:
        f.write(edit(obj))
    return pack_with_node(str(dst / "CornellBox.xml"), str(base / "packed"))


TWIN = "\ng backWallTwin\nusemtl leftWall\nf 9 10 11 12\n"  # test_mailbox_exact_ties' duplicated back wall


def _without_floor(obj):
    """The floor's face removed (its vertices stay, so every other index keeps its meaning)."""
    out, n = re.subn(r"(g floor\s*\nusemtl floor\s*\n)f -4 -3 -2 -1[^\n]*\n", r"\1", obj, count=1)
    assert n == 1
    return out


@pytest.fixture(scope="module")
def tie34(tmp_path_factory):
    return _cornell_variant(tmp_path_factory, "tie34", lambda obj: obj + TWIN)


@pytest.fixture(scope="module")
def tie32(tmp_path_factory):
    return _cornell_variant(tmp_path_factory, "tie32", lambda obj: _without_floor(obj) + TWIN)


SYNTH_N = 48  # the box's 36 triangles + 12 random ones: between 33 and 64 distinct entries


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    from conftest import ROOT, pack_with_node
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import synth_scene
    base = tmp_path_factory.mktemp("synth")
    return pack_with_node(synth_scene.write(SYNTH_N, str(base)), str(base / "packed"))


_ORACLE = {}


def oracle_frame(p, key, meta, t, depth):
    k = ("f", key, int(meta[0]), int(meta[1]), t, depth)
    if k not in _ORACLE:
        _ORACLE[k] = oracle.frame(p.triangle_data, p.bvh_data, meta, t, depth)[0]
    return _ORACLE[k]


def oracle_render(p, key, meta, n, depth):
    k = ("r", key, int(meta[0]), int(meta[1]), n, depth)
    if k not in _ORACLE:
        _ORACLE[k] = oracle.render(p.triangle_data, p.bvh_data, meta, 0, n, 1, depth)
    return _ORACLE[k]


def check_scene(p, key, W, H, width, salts=(3,), depth=8, counted=True):
    """Frames at `salts` and a 3-frame accumulating render (with counters when `counted`: the wide
    counting instance) against the oracle; the uncounted launches ran the `width`-bit instance."""
    meta = p.meta_for(W, H)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for t in salts:
            gpu = s.frame(meta, t, depth)
            assert _lib.last_bf_width() == width
            ref = oracle_frame(p, key, meta, t, depth)
            assert same_bits(gpu, ref), report(gpu, ref)
        acc = s.render(meta, 0, 3, 1, depth, pt_amd.MODE_WAVEFRONT)
        assert _lib.last_bf_width() == width
        racc, rc = oracle_render(p, key, meta, 3, depth)
        assert same_bits(acc, racc), report(acc, racc)
        if counted:
            acc2, gc = s.render(meta, 0, 3, 1, depth, pt_amd.MODE_WAVEFRONT, counters=True)
            assert _lib.last_bf_width() == 0  # the counting instance keeps the 64-bit stack walk
            assert same_bits(acc2, racc), report(acc2, racc)
            assert gc == rc, (gc, rc)


# 1. narrow path, plain: CornellBox, default and the recompute path, a partial last batch and 48 x 40
@pytest.mark.parametrize("slots", [None, "1"], ids=["slots8", "slots1"])
@pytest.mark.parametrize("W,H", [(33, 17), (48, 40)])
def test_narrow_cornell(packed, ptopts, W, H, slots):
    p = packed["CornellBox"]
    U, N = tree_facts(p.bvh_data)
    assert U <= 32 and N <= 32, (U, N)
    ptopts.set("kernel", "wavefront")
    if slots:
        ptopts.set("bf_slots", slots)
    check_scene(p, "cornell", W, H, 32, salts=(1, 3), depth=16 if W == 33 else 8)


# 2. narrow path, exact ties: the duplicated back wall without the floor (<= 32 entries)
@pytest.mark.parametrize("slots", [None, "1"], ids=["slots8", "slots1"])
@pytest.mark.parametrize("order", [None, "reverse"], ids=["forward", "reverse"])
def test_narrow_exact_ties(tie32, ptopts, order, slots):
    U, N = tree_facts(tie32.bvh_data)
    assert 30 <= U <= 32 and N <= 32, (U, N)
    ptopts.set("kernel", "wavefront")
    if order:
        ptopts.set("mb_uid_order", order)
    if slots:
        ptopts.set("bf_slots", slots)
    check_scene(tie32, "tie32", 48, 40, 32)


# 3. wide path unchanged: 34 entries, and a synthetic scene between 33 and 64
def test_wide_ties(tie34, ptopts):
    U, N = tree_facts(tie34.bvh_data)
    assert U == 34 and N <= 64, (U, N)
    ptopts.set("kernel", "wavefront")
    check_scene(tie34, "tie34", 48, 40, 64)


def test_wide_synthetic(synth, ptopts):
    U, N = tree_facts(synth.bvh_data)
    assert 33 <= U <= 63 and N <= 64, (U, N)
    ptopts.set("kernel", "wavefront")
    check_scene(synth, "synth", 48, 40, 64)


# 4. boundary: CornellBox forced wide equals CornellBox narrow, and both the oracle
def test_forced_wide_equals_narrow(packed, ptopts):
    p = packed["CornellBox"]
    meta = p.meta_for(48, 40)
    ptopts.set("kernel", "wavefront")
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        narrow = s.frame(meta, 2, 16)
        assert _lib.last_bf_width() == 32
        ptopts.set("bf_narrow", "0")
        wide = s.frame(meta, 2, 16)
        assert _lib.last_bf_width() == 64
        ptopts.set("bf_stackless", "0")  # no stackless replay: nothing narrow either
        stack = s.frame(meta, 2, 16)
        assert _lib.last_bf_width() == 0
    ref = oracle_frame(p, "cornell", meta, 2, 16)
    assert same_bits(narrow, wide), report(narrow, wide)
    assert same_bits(narrow, ref), report(narrow, ref)
    assert same_bits(stack, ref), report(stack, ref)
