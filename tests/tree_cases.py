"""Trees no builder here produces (a helper module like tests/cam_cases.py, not a conftest): the
catalogue tests/test_tree_cpu.py and tests/test_gpu_tree.py share.  The C ABI takes any packed
`bvh_data` whose traversal stack stays below kStackMax (pt_scene_layout.cpp build_layout); every tree
the suite rendered before came from the reference builder (max_stack <= 15) or the SAH builder (<= 19).
Here the geometry stays (the `packed` fixture's scenes and scripts/synth_scene.py's) and the TREE over
it changes: its depth, its node and entry counts around the thresholds of the brute-force kernels, its
leaf sizes around the lean flavours' turn widths, and the order of its records in memory.

Pure numpy.  decode() reads a packed bvh_data into scene_oracle.Node objects by following the child
offsets (so any layout decodes); trees are written back with scene_oracle.pack_bvh (pre-order, the
left child directly after its node), except relayout(), whose packer places the records as asked.

Transforms (each returns a packed bvh_data):
  stilts(bvh, k, side)   k nodes above the root, each with one empty leaf (17-float header, count 0) on
                         `side` (L, R, Z = alternating) and the rest of the tree as its other child,
                         both child boxes the scene's outer bounds.  fat=True: the sibling is an internal
                         node with two empty leaves instead, so that with side L every stilt PARKS its
                         sibling: the only cases whose traversal stack really grows to max_stack - 1
                         entries (a thin stilt or a chain never has two internal children to visit).
  bush(bvh, m)           m internal nodes more: a new root whose left child is the old root and whose
                         right child is a balanced tree of m - 1 nodes holding only empty leaves, all
                         boxes the outer bounds — walked by every ray that enters them, before the old
                         tree and so before any hit could prune them.
  relayout(bvh, how)     the same tree stored differently (LAYOUTS).
  chain(tri, entries, order, side, pad)   from scratch: node i holds the single-entry leaf order[i] and
                         the rest of the chain; the last node two single-entry leaves.  Boxes padded by
                         `pad` (an axis-aligned triangle's tight box has no thickness: the slab test
                         fails on it).
  grove(tri, entries, nodes, pad)         from scratch: a balanced tree of `nodes` internal nodes.
  with_leaf(tri, bvh, n, dup)             a new root whose left child is a leaf of n distinct entries
                         (box: the outer bounds), the right child the old root.  The entries: the
                         largest one, then the emissive ones, then the others by falling area.  (The
                         leaf is tested before the root decides about the old tree, and a ray that
                         starts inside the bounds compares its hit with the box's EXIT distance there:
                         it never enters the old tree.  Without the light in the leaf its shadow rays
                         find nothing and 1 % of the pixels are lit.)
                         dup: the leaf's first entry twice more (in the middle and at the end: n + 2).
  trim_to(tri, bvh, U)   drops entries (every occurrence) until U distinct ones remain, never an
                         emissive one; the highest vertex numbers go first (the synthetic scenes'
                         random triangles before the box's walls).

Lit shares (3-frame render, depth 8, the oracle's; tests/test_tree_cpu.py prints and bounds them) are
listed in DESIGN.md §4.
"""
import os
import sys

import numpy as np

import cam_cases as cc
import scene_oracle as so
from scene_oracle import Node

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH, SALT = cc.DEPTH, cc.SALT
STACK_MAX = 32    # pt_device.h kStackMax: max_stack >= 32 is refused
NARROW_MAX = 32   # pt_layout.h kBfNarrowMax: entries, and internal nodes
REPLAY_U, REPLAY_NODES = 63, 64  # pt_scene_layout.cpp build_mailbox: the stackless replay tree
MAILBOX_U = 64
LDS_BUDGET = 64 * 1024  # pt_kernels.h kLdsSceneBudget
MEGA_BLOCK = 256        # pt_kernels.h kMegaBlock
LAYOUTS = ("right_first", "leaves_last", "reverse", "padded")
PAD = 0.05


# ---------------------------------------------------------------------------------------------
# packed bvh_data <-> Node trees
# ---------------------------------------------------------------------------------------------
class Tree:
    """root: scene_oracle.Node tree (objs index `recs`); recs: the distinct entries (i0, i1, i2,
    material) in first-appearance order of a left-first pre-order walk; omin, omax: bvh[0:6]."""

    def __init__(self, root, recs, omin, omax):
        self.root, self.recs, self.omin, self.omax = root, recs, omin, omax


def _floats(a):
    return [float(x) for x in a]


def decode(bvh):
    bvh = np.asarray(bvh, np.float32)
    recs, index = [], {}

    def at(o, bmin, bmax):
        if bvh[o] == 1.0:
            objs = []
            for k in range(int(bvh[o + 4]) // 4):
                e = tuple(_floats(bvh[o + 17 + 4 * k: o + 21 + 4 * k]))
                if e not in index:
                    index[e] = len(recs)
                    recs.append(e)
                objs.append(index[e])
            return Node(True, int(bvh[o + 1]), bmin, bmax, np.array(objs, dtype=int))
        n = Node(False, int(bvh[o + 1]), bmin, bmax, np.zeros(0, dtype=int))
        n.left = at(int(bvh[o + 2]), _floats(bvh[o + 5:o + 8]), _floats(bvh[o + 8:o + 11]))
        n.right = at(int(bvh[o + 3]), _floats(bvh[o + 11:o + 14]), _floats(bvh[o + 14:o + 17]))
        return n

    omin, omax = _floats(bvh[0:3]), _floats(bvh[3:6])
    return Tree(at(6, list(omin), list(omax)), recs, omin, omax)


def pack(t):
    return so.pack_bvh(t.root, t.omin, t.omax, np.array(t.recs, dtype=np.float64).reshape(-1, 4))


def _pre_order(root, right_first=False):
    out, work = [], [root]
    while work:
        n = work.pop()
        out.append(n)
        if not n.is_leaf:
            work += [n.right, n.left] if not right_first else [n.left, n.right]
    return out


def pack_as(t, how):
    """The tree with its records in another order.  The root stays at offset 6 (the traversals start
    there); every other record may stand anywhere: the decoder and the oracle follow the offsets.
      right_first   pre-order with the right subtree directly after its node
      leaves_last   the internal nodes in pre-order, then all leaves
      reverse       the root, then the pre-order's other records backwards (children before parents)
      padded        pre-order with 1..16 floats of 1.0 (the leaf tag) after the records, in turn"""
    pre = _pre_order(t.root)
    if how == "right_first":
        seq = _pre_order(t.root, right_first=True)
    elif how == "leaves_last":
        seq = [n for n in pre if not n.is_leaf] + [n for n in pre if n.is_leaf]
    elif how == "reverse":
        seq = pre[:1] + pre[:0:-1]
    elif how == "padded":
        seq = pre
    else:
        raise ValueError(how)
    off, pos = {}, 6
    for i, n in enumerate(seq):
        off[id(n)] = pos
        pos += 17 + 4 * len(n.objs) + ((i % 16) + 1 if how == "padded" else 0)
    assert pos < 1 << 24  # offsets are f32
    out = np.ones(pos, np.float64)
    out[0:3], out[3:6] = t.omin, t.omax
    recs = np.array(t.recs, dtype=np.float64).reshape(-1, 4)
    for n in seq:
        o = off[id(n)]
        if n.is_leaf:
            out[o:o + 17] = [1, n.axis, -1, -1, 4 * len(n.objs)] + [0] * 12
            out[o + 17:o + 17 + 4 * len(n.objs)] = recs[n.objs].reshape(-1)
        else:
            out[o:o + 17] = [0, n.axis, off[id(n.left)], off[id(n.right)], -2, *n.left.bmin, *n.left.bmax,
                             *n.right.bmin, *n.right.bmax]
    return out.astype(np.float32)


def facts(bvh):
    """What the layout rules are stated in, read off the packed buffer: U distinct entries, internal
    nodes, leaves, the largest leaf, max_stack = the deepest internal node's depth + 1 (the root's
    depth is 0: pt_scene_layout.cpp build_layout), and the verdicts that follow from them."""
    bvh = np.asarray(bvh, np.float32)
    entries, nodes, leaves, max_leaf, depth, work = set(), 0, 0, 0, 0, [(6, 0)]
    while work:
        o, d = work.pop()
        nodes += 1
        depth = max(depth, d)
        for c in (int(bvh[o + 2]), int(bvh[o + 3])):
            if bvh[c] == 1.0:
                n = int(bvh[c + 4]) // 4
                leaves += 1
                max_leaf = max(max_leaf, n)
                for k in range(n):
                    entries.add(tuple(_floats(bvh[c + 17 + 4 * k: c + 21 + 4 * k])))
            else:
                work.append((c, d + 1))
    U = len(entries)
    mailbox = 1 <= U <= MAILBOX_U
    replay = mailbox and U <= REPLAY_U and nodes <= REPLAY_NODES
    narrow = replay and U <= NARROW_MAX and nodes <= NARROW_MAX
    return dict(U=U, nodes=nodes, leaves=leaves, max_leaf=max_leaf, max_stack=depth + 1, mailbox=mailbox,
                replay=replay, narrow=narrow)


# ---------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------
def vertex(tri, i):
    vs = int(tri[2])
    return np.asarray(tri[vs + 3 * (int(i) - 1): vs + 3 * int(i)], np.float64)


def corners(tri, rec):
    return np.array([vertex(tri, rec[k]) for k in range(3)])


def area(tri, rec):
    p = corners(tri, rec)
    return 0.5 * float(np.linalg.norm(np.cross(p[1] - p[0], p[2] - p[0])))


def emissive(tri, rec):
    m = int(tri[4]) + 15 * int(rec[3])
    return float(tri[m + 12]) + float(tri[m + 13]) + float(tri[m + 14]) > 0


def _box(tri, recs, objs, pad, empty):
    if len(objs) == 0:
        return list(empty[0]), list(empty[1])
    pts = np.concatenate([corners(tri, recs[o]) for o in objs])
    f32 = lambda v: [float(np.float32(x)) for x in v]  # noqa: E731
    return f32(pts.min(0) - pad), f32(pts.max(0) + pad)


def _empty(t):
    return Node(True, 0, list(t.omin), list(t.omax), np.zeros(0, dtype=int))


def _inner(t, left, right):
    n = Node(False, 0, list(t.omin), list(t.omax), np.zeros(0, dtype=int))
    n.left, n.right = left, right
    return n


def _hollow(t, m):
    """A balanced tree of m internal nodes whose leaves are all empty (m = 0: one empty leaf)."""
    if m == 0:
        return _empty(t)
    return _inner(t, _hollow(t, (m - 1) // 2), _hollow(t, m - 1 - (m - 1) // 2))


# ---------------------------------------------------------------------------------------------
# transforms
# ---------------------------------------------------------------------------------------------
def stilts(bvh, k, side, fat=False):
    t = decode(bvh)
    for i in reversed(range(k)):
        sd = side if side in "LR" else "LR"[i % 2]
        sib = _hollow(t, 1 if fat else 0)
        t.root = _inner(t, sib, t.root) if sd == "L" else _inner(t, t.root, sib)
    return pack(t)


def bush(bvh, m):
    assert m >= 1
    t = decode(bvh)
    t.root = _inner(t, t.root, _hollow(t, m - 1))
    return pack(t)


def relayout(bvh, how):
    return pack_as(decode(bvh), how)


def _scratch(tri, recs, pad):
    pts = np.concatenate([corners(tri, r) for r in recs])
    lo, hi = pts.min(0) - pad, pts.max(0) + pad
    return Tree(None, list(recs), [float(np.float32(x)) for x in lo], [float(np.float32(x)) for x in hi])


def chain(tri, entries, order, side, pad=PAD):
    order = list(order)
    assert len(order) >= 2
    t = _scratch(tri, entries, pad)
    empty = (t.omin, t.omax)

    def leaf(objs):
        return Node(True, 0, *_box(tri, t.recs, objs, pad, empty), np.array(objs, dtype=int))

    def rec(i):
        rest = order[i + 1:]
        node = Node(False, 0, *_box(tri, t.recs, order[i:], pad, empty), np.zeros(0, dtype=int))
        a, b = leaf([order[i]]), (leaf(rest) if len(rest) == 1 else rec(i + 1))
        sd = side if side in "LR" else "LR"[i % 2]
        node.left, node.right = (a, b) if sd == "L" else (b, a)
        return node
    t.root = rec(0)
    return pack(t)


def grove(tri, entries, nodes, pad=PAD):
    t = _scratch(tri, entries, pad)
    empty = (t.omin, t.omax)
    cen = np.array([corners(tri, r).mean(0) for r in t.recs])

    def build(objs, m):
        box = _box(tri, t.recs, objs, pad, empty)
        if m == 0:
            return Node(True, 0, *box, np.array(objs, dtype=int))
        ml = (m - 1) // 2
        mr = m - 1 - ml
        ext = cen[objs].max(0) - cen[objs].min(0) if len(objs) else np.zeros(3)
        objs = sorted(objs, key=lambda o: (cen[o][int(np.argmax(ext))], o))
        cut = len(objs) * (ml + 1) // (ml + mr + 2)
        n = Node(False, 0, *box, np.zeros(0, dtype=int))
        n.left, n.right = build(objs[:cut], ml), build(objs[cut:], mr)
        return n
    t.root = build(list(range(len(t.recs))), nodes)
    return pack(t)


def with_leaf(tri, bvh, n, dup=False):
    t = decode(bvh)
    by_area = sorted(range(len(t.recs)), key=lambda i: (-area(tri, t.recs[i]), i))
    assert n <= len(by_area)
    lights = [i for i in by_area if emissive(tri, t.recs[i])]
    rest = [i for i in by_area if i not in lights]
    objs = (rest[:1] + lights + rest[1:])[:n]
    if dup:
        objs = objs[:n // 2] + [objs[0]] + objs[n // 2:] + [objs[0]]
    leaf = Node(True, 0, list(t.omin), list(t.omax), np.array(objs, dtype=int))
    t.root = _inner(t, leaf, t.root)
    return pack(t)


def trim_to(tri, bvh, U):
    t = decode(bvh)
    spare = sorted((i for i in range(len(t.recs)) if not emissive(tri, t.recs[i])), key=lambda i: (-t.recs[i][0], i))
    drop = set(spare[:len(t.recs) - U])
    assert len(t.recs) - len(drop) == U, (len(t.recs), U)
    for n in _pre_order(t.root):
        if n.is_leaf:
            n.objs = np.array([o for o in n.objs if o not in drop], dtype=int)
    return pack(t)


def kept(tri, bvh, U):
    """The U entries trim_to keeps, as records."""
    return decode(trim_to(tri, bvh, U)).recs


def light_tree(tri, bvh, U):
    """The tree of the first U (1 or 2) emissive entries alone: one root, the entries in its leaves
    (U = 1: the right child is an empty leaf)."""
    t = decode(bvh)
    lights = [r for r in t.recs if emissive(tri, r)][:U]
    assert len(lights) == U
    s = _scratch(tri, lights, PAD)
    empty = (s.omin, s.omax)
    leaves = [Node(True, 0, *_box(tri, s.recs, [i], PAD, empty), np.array([i], dtype=int)) for i in range(U)]
    if U == 1:
        leaves.append(_empty(s))
    s.root = Node(False, 0, list(s.omin), list(s.omax), np.zeros(0, dtype=int))
    s.root.left, s.root.right = leaves
    return pack(s)


def probe_entries(bvh, kind):
    """The entries a reach condition asks for: "added": the leaf with_leaf put under the root's left;
    "deepest": the leaf children of the deepest internal node."""
    t = decode(bvh)
    if kind == "added":
        return {t.recs[o] for o in t.root.left.objs}
    best, work = (-1, None), [(t.root, 0)]
    while work:
        n, d = work.pop()
        if d > best[0]:
            best = (d, n)
        work += [(c, d + 1) for c in (n.left, n.right) if not c.is_leaf]
    return {t.recs[o] for c in (best[1].left, best[1].right) if c.is_leaf for o in c.objs}


class EntrySet:
    """`recs` with their corners, for on(): does a hit at distance t along (o, d) lie on one of them
    (f64 Moeller-Trumbore: barycentrics within 1e-4, the plane's distance within 1e-4 of t)?"""

    def __init__(self, tri, recs):
        p = np.array([corners(tri, r) for r in recs])
        self.p0, self.e1, self.e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]

    def on(self, o, d, t_hit):
        o, d = np.asarray(o[:3], np.float64), np.asarray(d[:3], np.float64)
        h = np.cross(d, self.e2)
        det = (self.e1 * h).sum(1)
        ok = np.abs(det) > 1e-12
        det = np.where(ok, det, 1.0)
        s = o - self.p0
        u = (s * h).sum(1) / det
        q = np.cross(s, self.e1)
        v = (q @ d) / det
        t = (self.e2 * q).sum(1) / det
        tol = 1e-4 * max(1.0, abs(float(t_hit)))
        return bool((ok & (u >= -1e-4) & (v >= -1e-4) & (u + v <= 1 + 1e-4) & (np.abs(t - float(t_hit)) <= tol)).any())


# ---------------------------------------------------------------------------------------------
# base scenes and the catalogue
# ---------------------------------------------------------------------------------------------
SYNTH = {"synth80": 80, "synth200": 200}
XML_SCENES = ("CornellBox", "CornellBox-Glossy", "CornellBox-Sphere", "MedievalBoat")


def bases(packed, tmp):
    """name -> conftest.Packed: the four XML scenes of the catalogue from the `packed` fixture and
    the synthetic ones (scripts/synth_scene.py) packed by the Node host under directory tmp."""
    from conftest import pack_with_node
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import synth_scene
    out = {s: packed[s] for s in XML_SCENES}
    for name, n in SYNTH.items():
        d = os.path.join(str(tmp), name)
        out[name] = pack_with_node(synth_scene.write(n, d), os.path.join(d, "packed"))
    return out


def camera_scene(base):
    return base if base in cc.CAMERAS else "CornellBox"  # the synthetic scenes stand under CornellBox.xml's camera


def size_of(base):
    return cc.size_of(base)


class Case:
    """One tree: `make(tri, bvh)` of base scene `base` -> bvh_data; `cam`: a cam_cases camera of the
    base's scene; `expect`: what the construction fixes among facts()'s keys; `probe`: the reach
    condition ("added" / "deepest" / None); `dim`: exempt from the lit-share bound (U <= 2)."""

    def __init__(self, cid, group, base, make, expect=None, cam="xml", probe=None, dim=False, same_image=False):
        self.id, self.group, self.base, self.make, self.cam, self.probe = cid, group, base, make, cam, probe
        self.expect, self.dim, self.same_image = dict(expect or {}), dim, same_image


class Built:
    """A case's buffers, with conftest.Packed's meta_for (the case's camera at another size)."""

    def __init__(self, case, p):
        self.case = case
        self.triangle_data = p.triangle_data
        self.bvh_data = case.make(p.triangle_data, p.bvh_data)
        self.size = size_of(case.base)
        self.meta = self.meta_for(*self.size)

    def meta_for(self, W, H):
        return cc.meta_of(camera_scene(self.case.base), self.case.cam, (W, H))


CASES = []
BOAT_CAM = "rigging"  # the boat's own camera lights 0.143 of the pixels, cam_cases' rigging 0.878


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


def _catalogue():
    # 1. depth: stilts to max_stack 20 and 31 (k = target - the scene's own max_stack), three sides;
    #    fat stilts with side L to 31 (the stack really holds 30 parked nodes); chains of 31 levels
    for s in XML_SCENES:
        cam = BOAT_CAM if s == "MedievalBoat" else "xml"
        for target in (20, 31):
            for side in "LRZ":
                _add(f"stilts-{s}-{target}{side}", "depth", s,
                     lambda tri, bvh, target=target, side=side: stilts(bvh, target - facts(bvh)["max_stack"], side),
                     {"max_stack": target}, cam=cam, same_image=True)
        _add(f"fat-stilts-{s}-31L", "depth", s,
             lambda tri, bvh: stilts(bvh, 31 - facts(bvh)["max_stack"], "L", fat=True), {"max_stack": 31}, cam=cam,
             same_image=True)
    # none of those scenes' LDS spans fits 64 KiB at any depth (0.4 .. 3.6 MB), CornellBox's fits at
    # every depth; the 200-triangle synthetic scene crosses scene_fits_lds between max_stack 8 and 9
    for target in (7, 9, 31):
        _add(f"stilts-synth200-{target}Z", "depth", "synth200",
             lambda tri, bvh, target=target: stilts(bvh, target - facts(bvh)["max_stack"], "Z"),
             {"max_stack": target, "fits_lds": target <= 7}, same_image=True)
    for side in "LRZ":
        _add(f"chain-CornellBox-{side}", "depth", "CornellBox",
             lambda tri, bvh, side=side: chain(tri, decode(bvh).recs, CHAIN_ORDER, side),
             {"max_stack": 31, "nodes": 31, "U": 32, "max_leaf": 1, "narrow": True}, probe="deepest")
    # 2. counts: CornellBox (U = 32, 16 nodes) with bushes; the light alone; synthetic scenes trimmed
    for total in (31, 32, 33, 63, 64, 65):
        _add(f"bush-CornellBox-{total}", "counts", "CornellBox",
             lambda tri, bvh, total=total: bush(bvh, total - facts(bvh)["nodes"]),
             {"nodes": total, "U": 32, "narrow": total <= 32, "replay": total <= 64, "mailbox": True}, same_image=True)
    _add("light-U2", "counts", "CornellBox", lambda tri, bvh: light_tree(tri, bvh, 2),
         {"U": 2, "nodes": 1, "narrow": True}, cam="tele3", dim=True)
    _add("light-U1", "counts", "CornellBox", lambda tri, bvh: light_tree(tri, bvh, 1),
         {"U": 1, "nodes": 1, "narrow": True}, cam="tele3", dim=True)
    for U in (31, 33, 62, 63, 64, 65):
        _add(f"trim-synth80-{U}", "counts", "synth80", lambda tri, bvh, U=U: trim_to(tri, bvh, U),
             {"U": U, "mailbox": U <= 64})
    _add("trim-synth80-63-bush65", "counts", "synth80",
         lambda tri, bvh: (lambda b: bush(b, 65 - facts(b)["nodes"]))(trim_to(tri, bvh, 63)),
         {"U": 63, "nodes": 65, "mailbox": True, "replay": False})
    _add("grove-synth80-64-16", "counts", "synth80", lambda tri, bvh: grove(tri, kept(tri, bvh, 64), 16),
         {"U": 64, "nodes": 16, "mailbox": True, "replay": False})
    # 3. leaves: one more leaf of exactly n distinct entries
    for s in ("CornellBox-Sphere", "synth200"):
        for n in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129):
            _add(f"leaf-{s}-{n}", "leaves", s, lambda tri, bvh, n=n: with_leaf(tri, bvh, n),
                 {"mailbox": False}, probe="added")
        for n in (17, 129):
            _add(f"leaf-{s}-{n}dup", "leaves", s, lambda tri, bvh, n=n: with_leaf(tri, bvh, n, dup=True),
                 {"mailbox": False}, probe="added")
    _add("twig-CornellBox-Sphere", "leaves", "CornellBox-Sphere", lambda tri, bvh: bush(bvh, 2), {"mailbox": False},
         same_image=True)
    _add("leaf-CornellBox-5dup", "leaves", "CornellBox", lambda tri, bvh: with_leaf(tri, bvh, 5, dup=True),
         {"U": 32, "nodes": 17, "narrow": True}, probe="added")
    # 4. layout
    for s in ("CornellBox", "CornellBox-Sphere", "MedievalBoat"):
        for how in LAYOUTS:
            _add(f"layout-{s}-{how}", "layout", s, lambda tri, bvh, how=how: relayout(bvh, how),
                 cam=BOAT_CAM if s == "MedievalBoat" else "xml", same_image=True)


# The chains' entry order over CornellBox's 32 distinct entries (decode()'s first-appearance order):
# backwards, so that the entries a walk from the root meets first lie deepest.  With the forward
# order the exit-distance pruning drops the rest of the chain after the first hit and 0.8 % of the
# pixels are lit; backwards half of them are, and the camera reaches the deepest leaves
# (tests/test_tree_cpu.py test_reach).
CHAIN_ORDER = list(range(31, -1, -1))

_catalogue()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
IDS = [c.id for c in CASES]

_BUILT = {}


def built(bases_, cid):
    if cid not in _BUILT:
        c = BY_ID[cid]
        _BUILT[cid] = Built(c, bases_[c.base])
    return _BUILT[cid]


def fits_lds(max_stack, span_bytes):
    """pt_kernels.hip scene_fits_lds: the megakernel block's stacks and the scene's LDS span in 64 KiB."""
    return max_stack * MEGA_BLOCK * 4 + span_bytes <= LDS_BUDGET
