"""No GPU: the reference and the inputs of the radiance queries (radiance_ref.py), pinned on the oracle
alone, and what of pt_query_radiance / pt_camera_seeds needs no device — the header, the symbols, the
argument checks that come before the scene is touched, pt_amd.unit_rays."""
import ctypes
import os
import re

import numpy as np
import pytest

import cam_cases as cc
import oracle
import pt_amd
import radiance_ref as rr
from test_gpu_query import SCENES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
COMPOSE = [("CornellBox", "xml", (40, 32)), ("CornellBox", "oblique", (40, 32)), ("MedievalBoat", "rigging", (24, 16))]
NAMES = sorted({s for s, _ in SCENES})


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("radiance_ref"))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_header_and_symbols():
    with open(os.path.join(ROOT, "include", "pt_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define PT_ABI_VERSION 3\b", text)  # additions keep the version
    for name in ("pt_query_radiance", "pt_query_radiance_async", "pt_camera_seeds", "pt_camera_seeds_async"):
        assert re.search(rf"\bint {name}\(", text), name
        assert hasattr(pt_amd.load_library(), name), name
    assert "pt_radiance_params" in text and ctypes.sizeof(pt_amd.RadianceParams) == 16
    assert "pt_capi_radiance.hip" in pt_amd._lib._BUILD_SRCS
    with open(pt_amd.lib_path(), "rb") as f:
        data = f.read()
    for kernel in (b"k_wf_generate_rays", b"k_wf_accum_rays", b"k_camera_seeds"):
        assert kernel in data, kernel


def test_argument_checks_before_the_scene():
    """The checks the header orders before the scene: answered with no device and no allocation."""
    L = pt_amd.load_library()
    p = ctypes.c_void_p
    buf = np.zeros(64, F)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16

    def call(n, prm, rays=a, seeds=a, acc=a, fn=L.pt_query_radiance_async):
        args = [None, p(rays), p(seeds), n, ctypes.byref(prm) if prm else None, p(acc), None]
        return fn(*(args + [None] if fn is L.pt_query_radiance_async else args))

    ok = pt_amd.RadianceParams(0.9, 0, 8, 1)
    for fn in (L.pt_query_radiance_async, L.pt_query_radiance):
        assert call((1 << 26) + 1, ok, fn=fn) == -1 and b"2^26" in L.pt_last_error()
        assert call(4, pt_amd.RadianceParams(0.9, 0, -1, 1), fn=fn) == -1 and b"max_depth" in L.pt_last_error()
        assert call(4, pt_amd.RadianceParams(0.9, 0, 1025, 1), fn=fn) == -1
        assert call(4, None, fn=fn) == -1
        assert call(4, ok, rays=None, fn=fn) == -1 and b"null" in L.pt_last_error()
        assert call(4, ok, seeds=None, fn=fn) == -1
        assert call(4, ok, acc=None, fn=fn) == -1
        assert call(4, ok, fn=fn) == -1 and b"null scene" in L.pt_last_error()  # everything else in order
    assert call(4, ok, rays=a + 4) == -1 and b"aligned" in L.pt_last_error()
    assert call(4, ok, seeds=a + 2) == -1 and b"aligned" in L.pt_last_error()
    assert call(4, ok, acc=a + 1) == -1 and b"aligned" in L.pt_last_error()


@pytest.mark.parametrize("scene,camera,size", COMPOSE, ids=[f"{s}-{c}" for s, c, _ in COMPOSE])
def test_composition_on_the_oracle(packed, ref, scene, camera, size):
    """Camera rays and seeds restated in numpy + the reference with one sample = the oracle's frame with
    negatives clamped, bit for bit, and the same counters: the wrapper calls radiance() as main() does."""
    meta = cc.meta_of(scene, camera, size)
    ps = packed[scene]
    rays, seeds = rr.camera_rays_seeds(meta, rr.FRAME)
    assert rr.admitted(rays).all()
    acc, adm, cnt, _ = rr.radiance(ref, ps, rays, seeds, 1, cc.DEPTH, float(meta[45]), meta[46] > 0)
    want, wcnt = oracle.frame(ps.triangle_data, ps.bvh_data, meta, rr.FRAME, cc.DEPTH)
    want = np.where(want >= 0, want, F(0)).astype(F) + F(0)
    assert adm.all()
    assert np.array_equal(bits(acc), bits(want.reshape(-1, 3))), int((bits(acc) != bits(want.reshape(-1, 3))).sum())
    assert (acc > 0).any() and cnt == wcnt, (cnt, wcnt)


def test_unit_rays_are_admitted():
    """10^5 seeded vectors with components from 1e-20 to 1e20 in size: always admitted, and a unit vector
    in double precision too."""
    rng = np.random.default_rng(rr.SEED)
    n = 100000
    d = (10.0 ** rng.uniform(-20, 20, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(F)
    d[:1000, 1:] = 0  # axis directions
    rays = pt_amd.unit_rays(np.zeros((n, 3), F), d)
    assert rays.shape == (n, 8) and np.isinf(rays[:, 3]).all() and (rays[:, 7] == 0).all()
    x, y, z = (rays[:, k].astype(np.float64) for k in (4, 5, 6))
    assert np.abs(x * x + y * y + z * z - 1).max() < 4e-7
    # the f32 test as the header writes it (exact in float64 up to the last fused step, which _fma32 rounds)
    q = pt_amd._lib._fma32(rays[:, 6], rays[:, 6], pt_amd._lib._fma32(rays[:, 5], rays[:, 5], rays[:, 4] * rays[:, 4]))
    assert (np.abs(q - F(1)) <= rr.BAND).all(), float(np.abs(q - F(1)).max())
    assert rr.admitted(rays[:2000]).all()
    # the reference's normalize, bit for bit, where nothing needs scaling
    v = rng.standard_normal((2000, 3)).astype(F)
    u = pt_amd.unit_rays(np.zeros((2000, 3), F), v)[:, 4:7]
    for a, b in zip(v[:200], u[:200]):
        ln = np.sqrt(rr.dr.fmaf(a[2], a[2], rr.dr.fmaf(a[1], a[1], a[0] * a[0])))
        assert np.array_equal(bits(a / ln), bits(b)), (a, b)
    bad = pt_amd.unit_rays(np.zeros((3, 3), F), [(0, 0, 0), (np.nan, 1, 0), (np.inf, 1, 0)])
    assert not rr.admitted(bad).any()


def test_rejected_rays_fall_on_the_right_side():
    names = {n: adm for n, ray, adm in rr.rejected_rays((0, 0, 0), (0.6, 0.0, 0.8))}
    assert names == {"zero": False, "nan": False, "inf": False, "double": False, "long": False, "short": False,
                     "edge_hi_in": True, "edge_hi_out": False, "edge_lo_in": True, "edge_lo_out": False}, names
    for n, ray, adm in rr.rejected_rays((0, 0, 0), (0.6, 0.0, 0.8)):
        assert bool(rr.admitted(ray)[0]) == adm, n


@pytest.mark.parametrize("family", rr.FAMILIES)
@pytest.mark.parametrize("scene", NAMES)
def test_family_conditions(packed, ref, scene, family):
    """So that the device test cannot pass on black: at depth 8 and 3 samples at least a quarter of the
    admitted rays gather light, a path ends by a miss, shadow rays are traced; the rejected rays sit
    where the family says and nowhere else."""
    fam = rr.family(scene, packed, family)
    assert fam.rays.shape == (rr.N, 8) and fam.seeds.shape == (rr.N,)
    acc, adm, cnt, miss_ends = rr.reference(ref, scene, packed, family, 3)
    assert np.array_equal(np.flatnonzero(~adm), fam.rejected)
    assert np.array_equal(adm, rr.admitted(fam.rays))
    assert (len(fam.rejected) >= 8) == (family == "mixed")
    lit = float((acc[adm] > 0).any(axis=1).mean())
    print(scene, family, "lit", lit, "miss ends", miss_ends, cnt)
    assert lit >= 0.25 and miss_ends >= 1 and cnt["shadow_queries"] > 0
    assert cnt["samples"] == 3 * int(adm.sum()) and (acc[~adm] == 0).all()


@pytest.mark.parametrize("scene", ["CornellBox", "MedievalBoat"])
def test_seed_rule(packed, ref, scene):
    """Sample 0 uses the seed verbatim; three samples are three one-sample calls with the derived seeds,
    accumulated in order into the same buffer."""
    fam = rr.family(scene, packed, "mixed")
    ps, rrp = packed[scene], float(packed[scene].meta[45])
    init = rr.initial_accum()
    three, _, cnt3, _ = rr.radiance(ref, ps, fam.rays, fam.seeds, 3, 8, rrp, False, init)
    acc, total = init, dict.fromkeys(cnt3, 0)
    for s in range(3):
        sd = rr.sample_seeds(ref, fam.seeds, s)
        assert (s == 0) == np.array_equal(sd, fam.seeds)
        acc, _, c, _ = rr.radiance(ref, ps, fam.rays, sd, 1, 8, rrp, False, acc)
        total = {k: total[k] + c[k] for k in total}
    assert np.array_equal(bits(three), bits(acc)) and total == cnt3
    assert np.array_equal(bits(three[fam.rejected]), bits(init[fam.rejected]))
