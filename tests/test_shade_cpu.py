"""Lights and materials the five scenes never use (tests/shade_scenes.py), on the host and the oracle
alone: the images tests/test_gpu_shade.py compares the kernels with are worth comparing, and the host
tables the shade code reads (lights[], mats[]) equal a numpy restatement of the reference's arithmetic.
Everything at 40 x 32, depth 8: one frame (salt 3) and a 3-frame render.  The figures below are
conditions on the test's inputs, no tolerances of anything under test.

- Coverage.  One material at a time is made the only emitter (Ke = 1, every other Ke = 0) and one frame
  is rendered with depth 0: a pixel is lit when its camera ray ends on the material or when its first
  shade point's light sample is stopped by it, so the count says in how many pixels the material's
  record is read at the first bounce.  Each of CornellBox's seven non-emissive materials must have
  >= 64 (92 141 145 145 151 130 165 in five_objects), each sphere >= 32 (47, 78), each added emitter
  >= 8 (l2 52, l3 156, l4 312, l5 28).  Pixels whose camera ray itself ends on the material (exactly
  Ke): walls 78 .. 151, spheres 36 and 48, l2 1, l3 6, l4 5, l5 26, the light 5; every material must
  have one.  l5 is never sampled (the packer lists four objects), so only camera rays and stopped
  light samples reach it: it is placed and sized to be seen.
- Lit pixels (test_cond_cpu.lit): at least 1/3 of the frame and of the render, every case
  (measured 0.35 .. 0.66).
- Non-finite pixels in the frame: none, except `wild` (<= 1/4, measured 0.148; at least one NaN).  The
  random tables draw negative and non-finite parameters too; their seeds are chosen among those that
  keep the frame finite.
- Header ranges and Ntri per light variant; the layout harness's `lights (Ntri + 1) x 48` and `mats`
  digests equal the FNV-1a of the tables restated here: sample_area_lights' index arithmetic for
  k = 0 .. Ntri with clamped reads (k = Ntri: idx = -1 when range 4 is unused, the entry after range
  4 when it is used), and phong = (Ns + 2) / (2 * 3.14159f), Kd / 3.14159f in f32.
"""
import numpy as np
import pytest

import oracle
import shade_scenes as ss
from test_cond_cpu import lit
from test_scene_layout import harness as layout_harness  # noqa: F401  (the fixture, built as there)


@pytest.fixture(scope="module")
def lights(tmp_path_factory):
    base = tmp_path_factory.mktemp("shade_lights")
    return {v: ss.pack_light(v, base) for v in ss.LIGHT_VARIANTS}


@pytest.fixture(scope="module")
def cases(lights, packed, tmp_path_factory):
    return ss.all_cases(lights, packed["CornellBox-Sphere"], tmp_path_factory.mktemp("shade_tables"))


# ---------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------
def coverage(p, objects):
    """Per object (pixels lit, pixels of exactly Ke) of a depth-0 frame in which it alone emits."""
    tri = p.triangle_data
    nobj, m0 = int(tri[1]), int(tri[4])
    out = []
    for o in objects:
        t = tri.copy()
        for q in range(nobj):
            t[m0 + 15 * q + 12: m0 + 15 * q + 15] = 1.0 if q == o else 0.0
        img = oracle.frame(t, p.bvh_data, p.meta_for(ss.W, ss.H), ss.SALT, 0)[0]
        out.append((int((img != 0).any(axis=-1).sum()), int((img == 1).all(axis=-1).sum())))
    return out


def test_every_material_is_seen(lights, packed):
    p = lights["five_objects"]
    assert int(p.triangle_data[1]) == 12
    cov = coverage(p, range(12))
    names = ss.OBJECTS + ["light", "l2", "l3", "l4", "l5"]
    print("five_objects (lit, camera ray ends there):", dict(zip(names, cov)))
    for name, (n, first) in zip(names, cov):
        assert first >= 1, (name, first)
        if name in ss.OBJECTS:
            assert n >= 64, (name, n)
        elif name != "light":
            assert n >= 8, (name, n)
    sph = coverage(packed["CornellBox-Sphere"], range(2))
    print("CornellBox-Sphere spheres:", sph)
    for n, first in sph:
        assert n >= 32 and first >= 1, sph


# ---------------------------------------------------------------------------------------------
# the oracle's images
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ss.CASES)
def test_oracle_images_carry_light(cases, case):
    p = cases[case]
    meta = p.meta_for(ss.W, ss.H)
    frame = oracle.frame(p.triangle_data, p.bvh_data, meta, ss.SALT, ss.DEPTH)[0]
    render = oracle.render(p.triangle_data, p.bvh_data, meta, 0, 3, 1, ss.DEPTH)[0]
    bad = float((~np.isfinite(frame).all(axis=-1)).mean())
    print(f"{case}: lit {lit(frame).mean():.3f} of the frame, {lit(render).mean():.3f} of the render; "
          f"non-finite {bad:.3f} of the frame")
    assert lit(frame).mean() >= 1 / 3 and lit(render).mean() >= 1 / 3
    if case == "wild":
        assert bad <= 0.25, bad
    else:
        assert bad == 0.0, bad


def test_wild_is_not_tame(cases):
    """`wild` does produce non-finite radiance (or NaN == NaN would be compared on nothing)."""
    p = cases["wild"]
    frame = oracle.frame(p.triangle_data, p.bvh_data, p.meta_for(ss.W, ss.H), ss.SALT, ss.DEPTH)[0]
    assert np.isnan(frame).any()


# ---------------------------------------------------------------------------------------------
# header and host tables
# ---------------------------------------------------------------------------------------------
def wgsl_i32(f):
    """WGSL i32(f32): truncation toward zero, saturating, NaN -> 0."""
    f = float(f)
    if np.isnan(f):
        return 0
    return int(max(-2 ** 31, min(2 ** 31 - 1, np.trunc(f))))


def at(tri, i):
    """A read of the packed buffer with the index clamped as an unsigned one (Tint's robustness)."""
    u = i & 0xFFFFFFFF
    return tri[min(u, len(tri) - 1)]


def header_ranges(tri):
    return [(wgsl_i32(tri[8 + 2 * s]), wgsl_i32(tri[9 + 2 * s])) for s in range(4)]


def light_table(tri):
    """sample_area_lights' three vertices for k = 0 .. Ntri: [Ntri + 1, 12] f32 (xyz + a zero pad each)."""
    r = header_ranges(tri)
    n = [(e - s) // 4 if s != -1 else 0 for s, e in r]
    ntri, vs = sum(n), wgsl_i32(at(tri, 2))
    out = np.zeros((ntri + 1, 12), np.float32)
    for k in range(ntri + 1):
        if k < n[0]:
            idx = k * 4 + r[0][0]
        elif k < n[0] + n[1]:
            idx = (k - n[0]) * 4 + r[1][0]
        elif k < n[0] + n[1] + n[2]:
            idx = (k - n[0] - n[1]) * 4 + r[2][0]
        else:
            idx = (k - n[0] - n[1] - n[2]) * 4 + r[3][0]
        for j in range(3):
            i = (wgsl_i32(at(tri, idx + j)) - 1) * 3
            out[k, 4 * j: 4 * j + 3] = [at(tri, vs + i + c) for c in range(3)]
    return out


def material_table(tri):
    """[objects, 16] f32: Ns Ni illum phong | Kd kd_pi0 | Ks kd_pi1 | Ke kd_pi2."""
    nobj, m0 = int(tri[1]), int(tri[4])
    m = tri[m0: m0 + 15 * nobj].reshape(nobj, 15)
    pi = np.float32(3.14159)
    out = np.zeros((nobj, 16), np.float32)
    with np.errstate(all="ignore"):
        out[:, 0:3] = m[:, 0:3]
        out[:, 3] = (m[:, 0] + np.float32(2)) / (np.float32(2) * pi)
        out[:, 4:7], out[:, 8:11], out[:, 12:15] = m[:, 6:9], m[:, 9:12], m[:, 12:15]
        kd_pi = m[:, 6:9] / pi
    out[:, 7], out[:, 11], out[:, 15] = kd_pi[:, 0], kd_pi[:, 1], kd_pi[:, 2]
    return out


def fnv1a(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def harness_rows(out):
    assert out[0] == "rc 0", out[:2]
    rows = {ln.split()[0]: ln.split() for ln in out[2:]}
    flags = dict(zip(rows["leaf_min"][0::2], rows["leaf_min"][1::2]))
    return rows, flags


@pytest.mark.parametrize("variant", ss.LIGHT_VARIANTS)
def test_header_ranges(lights, variant):
    tri = lights[variant].triangle_data
    r = header_ranges(tri)
    used = [x for x in r if x != (-1, -1)]
    assert r == used + [(-1, -1)] * (4 - len(used)) and len(used) == ss.RANGES[variant], r
    assert sum((e - s) // 4 for s, e in used) == ss.NTRI[variant], r
    # each range is one object's (i0, i1, i2, object) rows: the light, then the added emitters in order
    first = 0 if variant == "emitter_first" else ss.LIGHT_OBJECT
    for j, (s, e) in enumerate(used):
        assert int(tri[3]) <= s < e <= int(tri[4]) and (e - s) % 4 == 0
        assert set(tri[s + 3: e: 4].astype(int).tolist()) == {first + j}, (variant, j)
    if variant == "five_objects":  # the fifth emissive object's triangle follows range 4, unlisted
        assert int(tri[1]) == 12 and int(tri[r[3][1] + 3]) == 11 and r[3][1] + 4 == int(tri[4])
    if variant == "listed_but_dark":
        ke = tri[int(tri[4]) + 15 * 8 + 12: int(tri[4]) + 15 * 8 + 15]
        assert (ke > 0).any() and float(ke.sum()) < 0


@pytest.mark.parametrize("case", ss.CASES)
def test_host_tables_equal_the_restatement(layout_harness, cases, case):  # noqa: F811
    p = cases[case]
    tri = p.triangle_data
    rows, flags = harness_rows(layout_harness(p.dir))
    lt, mt = light_table(tri), material_table(tri)
    ntri = len(lt) - 1
    if case in ss.NTRI:
        assert ntri == ss.NTRI[case]
    assert rows["lights"][1:4] == [str(ntri + 1), "x", "48"], rows["lights"]
    assert rows["lights"][4] == fnv1a(lt), (case, lt)
    assert rows["mats"][1:4] == [str(int(tri[1])), "x", "64"], rows["mats"]
    assert rows["mats"][4] == fnv1a(mt), (case, mt)
    assert flags["ntri"] == str(ntri)
    # at most 64 distinct leaf entries: AUTO stays on the fused kernel (CornellBox-Sphere is no mailbox scene)
    assert flags["mailbox"] == ("0" if case in ss.SPHERE_TABLES else "1"), flags


def test_clamped_slot(lights):
    """What the table's last entry is: on five_objects l5's triangle (the entry after range 4), on the
    variants that leave range 4 unused the clamped read of idx = -1: the buffer's last float (padding,
    0), then floats 0 and 1 (the vertex and object counts) as 1-based vertex numbers."""
    tri = lights["five_objects"].triangle_data
    assert np.array_equal(light_table(tri)[-1].reshape(3, 4)[:, :3], ss.written_triangles(ss.EMITTERS["l5"][1])[0])
    tri = lights["two_objects"].triangle_data
    vs = int(tri[2])
    want = [[at(tri, vs + (wgsl_i32(v) - 1) * 3 + c) for c in range(3)] for v in (tri[-1], tri[0], tri[1])]
    assert np.array_equal(light_table(tri)[-1].reshape(3, 4)[:, :3], np.array(want, np.float32))
