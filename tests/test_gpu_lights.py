"""Light sampling on the device, slot by slot: pt_selftest_lights runs the shade code's sample_area_lights
for caller-supplied (seed, point) and is compared with the oracle's, bit for bit.  Renders cannot reach
the light table's last entry (k == Ntri, drawn only when hash1 is exactly 1.0: 65 of 2^31 hash values,
never in a 40 x 32 render, tens of times per step at the benchmark's size), which resolves the
reference's out-of-range else-branch with clamped reads; here seeds that draw it are supplied
(shade_scenes.HASH1_ONE_SEEDS, found by the search under that module's __main__).  Scenes: 1, 5 and 11
emissive triangles, all four header ranges used with and without an emissive object after them, and
plain CornellBox.
"""
import numpy as np
import pytest

import oracle
import pt_amd
import shade_scenes as ss
from test_gpu_parity import mismatch_report, same_bits

pytestmark = pytest.mark.gpu

SCENES = {"one_tri": 1, "fan5": 5, "four_objects": 11, "five_objects": 11, "CornellBox": 2}


@pytest.fixture(scope="module")
def scenes(packed, tmp_path_factory):
    base = tmp_path_factory.mktemp("lights")
    out = {v: ss.pack_light(v, base) for v in SCENES if v != "CornellBox"}
    out["CornellBox"] = packed["CornellBox"]
    return out


def samples():
    """4096 random seeds + the seeds that draw k == Ntri, and as many points inside the box."""
    rng = np.random.default_rng(5)
    seeds = np.concatenate([rng.integers(0, 2 ** 32, 4096, dtype=np.uint64), ss.HASH1_ONE_SEEDS]).astype(np.uint32)
    pts = rng.uniform([-0.9, 0.1, -0.9], [0.9, 1.8, 0.9], (len(seeds), 3)).astype(np.float32)
    return seeds, pts


def aims_at(points, dirs, tri):
    """Every ray (point, dir) meets the triangle's plane inside the triangle (float64, 1e-4 of slack
    in the barycentrics: the directions are normalised in f32)."""
    a, e1, e2 = tri[0].astype(np.float64), (tri[1] - tri[0]).astype(np.float64), (tri[2] - tri[0]).astype(np.float64)
    for p, d in zip(points.astype(np.float64), dirs.astype(np.float64)):
        t, u, v = np.linalg.solve(np.stack([d, -e1, -e2], axis=1), a - p)
        if not (t > 0 and u >= -1e-4 and v >= -1e-4 and u + v <= 1 + 1e-4):
            return False
    return True


def test_the_literal_seeds_draw_hash1_one():
    assert len(ss.HASH1_ONE_SEEDS) >= 4
    for s in ss.HASH1_ONE_SEEDS:
        assert oracle.hash1(s * 7 + 11) == 1.0, s
    assert np.all(ss.hash1_masked((np.array(ss.HASH1_ONE_SEEDS, np.uint64) * 7 + 11).astype(np.uint32)) <= 64)


@pytest.mark.parametrize("name", list(SCENES))
def test_light_samples_bitexact_slot_by_slot(scenes, name):
    test_the_literal_seeds_draw_hash1_one()
    p, ntri = scenes[name], SCENES[name]
    tri = p.triangle_data
    seeds, pts = samples()
    rdir, rk, weight = oracle.sample_area_lights(tri, pts, seeds)
    with pt_amd.Scene(tri, p.bvh_data) as s:
        assert s.info["emissive_tris"] == ntri
        gdir, gk = s.selftest_lights(seeds, pts)
    assert weight == float(np.float32(1) / np.float32(ntri))
    assert sorted(set(rk.tolist())) == list(range(ntri + 1)), sorted(set(rk.tolist()))
    assert np.all(rk[-len(ss.HASH1_ONE_SEEDS):] == ntri) and np.all(rk[:4096] < ntri)
    assert np.array_equal(gk, rk), np.argwhere(gk != rk)[:5].tolist()
    assert same_bits(gdir, rdir), mismatch_report(gdir, rdir)
    last = rk == ntri
    if name == "five_objects":  # the entry after range 4: l5's triangle
        assert aims_at(pts[last], gdir[last], ss.written_triangles(ss.EMITTERS["l5"][1])[0])
    if name == "CornellBox":  # idx = -1: the buffer's last float, then floats 0 and 1, as 1-based vertex numbers
        vs, n = int(tri[2]), len(tri)
        corner = [[tri[min((vs + (int(v) - 1) * 3 + c) & 0xFFFFFFFF, n - 1)] for c in range(3)] for v in (tri[-1], tri[0], tri[1])]
        assert aims_at(pts[last], gdir[last], np.array(corner, np.float32))
