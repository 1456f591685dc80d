"""No GPU: the reference and the inputs of the irradiance gathers (gather_ref.py), pinned on the oracle
alone, and what of pt_gather / pt_gather_rays needs no device — the header, the symbols, the argument
checks that come before the scene is touched, the admission band of the generated directions, the SH basis."""
import ctypes
import os
import re

import numpy as np
import pytest

import gather_ref as gr
import pt_amd
import radiance_ref as rr
from test_gpu_query import SCENES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = sorted({s for s, _ in SCENES})
FUNCS = ("pt_gather", "pt_gather_async", "pt_gather_rays", "pt_gather_rays_async")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return gr.build(tmp_path_factory.mktemp("gather_ref"))


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("gather_radiance_ref"))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_header_and_symbols():
    with open(os.path.join(ROOT, "include", "pt_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define PT_ABI_VERSION 3\b", text)  # additions keep the version
    for name in FUNCS:
        assert re.search(rf"\bint {name}\(", text), name
        assert hasattr(pt_amd.load_library(), name), name
    assert "pt_gather_point" in text and "pt_gather_params" in text and ctypes.sizeof(pt_amd._lib.GatherParams) == 24
    assert re.search(r"PT_GATHER_COSINE = 0, PT_GATHER_SH9 = 1", text)
    assert "pt_capi_gather.hip" in pt_amd._lib._BUILD_SRCS
    with open(pt_amd.lib_path(), "rb") as f:
        data = f.read()
    for kernel in (b"k_wf_generate_gather", b"k_wf_accum_gather", b"k_gather_rays"):
        assert kernel in data, kernel
    g = pt_amd.gather_points([(1, 2, 3)], [(0, 0, 1)], [0xDEADBEEF])
    assert g.shape == (1, 8) and g.view(np.uint32)[0, 3] == 0xDEADBEEF and g.view(np.uint32)[0, 7] == 0
    assert tuple(g[0, 0:3]) == (1, 2, 3) and tuple(g[0, 4:7]) == (0, 0, 1)


def test_argument_checks_before_the_scene():
    """The checks the header orders before the scene: answered with no device and no allocation."""
    L = pt_amd.load_library()
    p = ctypes.c_void_p
    buf = np.zeros(64, F)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16
    GP = pt_amd._lib.GatherParams

    def call(n, prm, pts=a, acc=a, fn=L.pt_gather_async):
        args = [None, p(pts), n, ctypes.byref(prm) if prm else None, p(acc), None]
        return fn(*(args + [None] if fn is L.pt_gather_async else args))

    ok = GP(0.9, 0, 8, 0, 1, 0)
    for fn in (L.pt_gather_async, L.pt_gather):
        assert call(4, None, fn=fn) == -1
        assert call(4, GP(0.9, 0, 8, 0, 1, 2), fn=fn) == -1 and b"mode" in L.pt_last_error()
        assert call((1 << 26) + 1, ok, fn=fn) == -1 and b"2^26" in L.pt_last_error()
        assert call(4, GP(0.9, 0, 8, (1 << 31) - 1, 2, 0), fn=fn) == -1 and b"2^31" in L.pt_last_error()
        assert call(4, GP(0.9, 0, 8, 0xFFFFFFFF, 0xFFFFFFFF, 0), fn=fn) == -1
        assert call(4, GP(0.9, 0, -1, 0, 1, 0), fn=fn) == -1 and b"max_depth" in L.pt_last_error()
        assert call(4, GP(0.9, 0, 1025, 0, 1, 1), fn=fn) == -1
        assert call(4, ok, pts=None, fn=fn) == -1 and b"null" in L.pt_last_error()
        assert call(4, ok, acc=None, fn=fn) == -1
        assert call(4, ok, fn=fn) == -1 and b"null scene" in L.pt_last_error()  # everything else in order
        assert call(4, GP(0.9, 0, 8, (1 << 31) - 1, 1, 1), fn=fn) == -1 and b"null scene" in L.pt_last_error()
    assert call(4, ok, pts=a + 4) == -1 and b"aligned" in L.pt_last_error()
    assert call(4, ok, acc=a + 1) == -1 and b"aligned" in L.pt_last_error()
    for fn, tail in ((L.pt_gather_rays_async, [None]), (L.pt_gather_rays, [])):
        assert fn(None, p(a), 4, 2, 0, p(a), p(a), *tail) == -1 and b"mode" in L.pt_last_error()
        assert fn(None, p(a), (1 << 26) + 1, 0, 0, p(a), p(a), *tail) == -1
        assert fn(None, p(a), 4, 0, 1 << 31, p(a), p(a), *tail) == -1
        assert fn(None, None, 4, 0, 0, p(a), p(a), *tail) == -1
        assert fn(None, p(a), 4, 0, 0, None, p(a), *tail) == -1
        assert fn(None, p(a), 4, 0, 0, p(a), None, *tail) == -1
        assert fn(None, p(a), 4, 0, 0, p(a), p(a), *tail) == -1 and b"null scene" in L.pt_last_error()
    assert L.pt_gather_rays_async(None, p(a), 4, 0, 0, p(a + 4), p(a), None) == -1 and b"aligned" in L.pt_last_error()
    assert L.pt_gather_rays_async(None, p(a), 4, 0, 0, p(a), p(a + 2), None) == -1 and b"aligned" in L.pt_last_error()


@pytest.mark.parametrize("scene", NAMES)
def test_cosine_is_radiance_on_the_emitted_rays(packed, ref, rref, scene):
    """The reference's COSINE sums equal radiance_ref.radiance, one sample at a time, on the rays and seeds
    of the reference's own gather_rays restatement — on a non-zero accumulator, with the same counters."""
    ps, rrp = packed[scene], float(packed[scene].meta[45])
    pts = gr.points(scene, packed).packed
    ns = gr.samples(scene)[1]
    want, adm, wcnt, _ = gr.reference(ref, scene, packed, "cosine", ns, init=True)
    acc, total = gr.initial_accum(), dict.fromkeys(wcnt, 0)
    for s in range(ns):
        rays, seeds = gr.rays(ref, pts, s)
        assert rr.admitted(rays).all() and np.isinf(rays[:, 3]).all() and (rays[:, 7] == 0).all()
        acc, _, c, _ = rr.radiance(rref, ps, rays, seeds, 1, 8, rrp, False, acc)
        total = {k: total[k] + c[k] for k in total}
    assert np.array_equal(bits(acc), bits(want)) and total == wcnt and (adm == ns).all()


@pytest.mark.parametrize("mode", gr.MODES)
@pytest.mark.parametrize("scene", NAMES)
def test_point_conditions(packed, ref, scene, mode):
    """So that the device tests cannot pass on black: at depth 8 no sample is rejected, at least a quarter
    of the points gather light (3 samples; the boat 8), a path ends by a miss, shadow rays are traced, and
    every sum is finite."""
    ns = gr.samples(scene)[1]
    acc, adm, cnt, miss_ends = gr.reference(ref, scene, packed, mode, ns)
    assert acc.shape == (gr.N, gr.width(mode)) and (adm == ns).all() and cnt["samples"] == ns * gr.N
    # SH9: coefficient 0 of a channel is 0.282095 times the channel's sum, positive when any light arrived
    lit = float((acc[:, ::9] > 0).any(axis=1).mean()) if mode == "sh9" else float((acc > 0).any(axis=1).mean())
    print(scene, mode, "samples", ns, "lit", lit, "miss ends", miss_ends, cnt)
    assert lit >= 0.25 and miss_ends >= 1 and cnt["shadow_queries"] > 0
    assert np.isfinite(acc).all()


def test_rejected_points_in_the_reference(packed, ref):
    """A zero, NaN, infinite, 2^-50- and 2^50-long normal: no COSINE sample, the accumulator's bits kept;
    SH9 ignores the normal."""
    g = gr.points("CornellBox", packed)
    nrm = g.n[:5].copy()
    nrm[0] = 0
    nrm[1, 0] = np.nan
    nrm[2, 1] = np.inf
    nrm[3] = (nrm[3] * F(2.0 ** -50)).astype(F)
    nrm[4] = (nrm[4] * F(2.0 ** 50)).astype(F)
    pts = pt_amd.gather_points(g.p[:5], nrm, g.seeds[:5])
    init = gr.initial_accum(5)
    init[1] = (-0.0, np.nan, np.inf)
    acc, adm, cnt, _ = gr.gather(ref, packed["CornellBox"], pts, 3, out=init)
    assert (adm == 0).all() and not any(cnt.values()) and np.array_equal(bits(acc), bits(init))
    rays, seeds = gr.rays(ref, pts, 1)
    assert (rays[:, 4:7] == 0).all() and (seeds == 0).all() and np.array_equal(bits(rays[:, 0:3]), bits(g.p[:5]))
    _, adm9, _, _ = gr.gather(ref, packed["CornellBox"], pts, 3, mode="sh9")
    assert (adm9 == 3).all()


def band_normals():
    """10^6 f32-normalised random normals, the six axes, and normals with one component scaled by 1e-5 ..
    1e-6 (nearly in a coordinate plane: the ONB's a = -1 / (s + n.z) and b = n.x n.y a at their extremes)."""
    rng = np.random.default_rng(gr.SEED + 7)
    v = rng.standard_normal((1000000, 3))
    small = rng.standard_normal((30000, 3))
    small[np.arange(30000), np.arange(30000) % 3] *= 10.0 ** rng.uniform(-6, -5, 30000)
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)
    return pt_amd.unit_rays(np.zeros((1030006, 3), F), np.concatenate([v, small, axes]))[:, 4:7]


def test_generated_directions_sit_inside_the_band(ref):
    """max |q - 1| of the generated directions <= 2^-19 in both modes — half the admission band, so no
    sample of a well-formed point is ever rejected — and no COSINE direction lies more than 1e-6 below the
    surface."""
    nrm = band_normals()
    n = nrm.shape[0]
    seeds = np.random.default_rng(gr.SEED + 8).integers(0, 2 ** 32, n, dtype=np.uint32)
    pts = pt_amd.gather_points(np.zeros((n, 3), F), nrm, seeds)
    fma = pt_amd._lib._fma32
    for mode in gr.MODES:
        worst = 0.0
        for sample in (0, 1, 2):
            d = gr.dirs(ref, pts, sample, mode)
            assert np.isfinite(d).all()
            q = fma(d[:, 2], d[:, 2], fma(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
            worst = max(worst, float(np.abs(q - F(1)).max()))
            if mode == "cosine":
                below = float((d.astype(np.float64) * nrm.astype(np.float64)).sum(axis=1).min())
                assert below >= -1e-6, (sample, below)
        print(mode, "max |q - 1| = 2^%.2f" % np.log2(worst))
        assert worst <= 2.0 ** -19, (mode, worst)
    # a normal of any admitted length gives the direction of its normalised copy — where normalising that
    # copy once more returns it (the call normalises whatever it is given, and n / sqrt(nn) is not always a
    # fixed point of itself: nn = 1 - 2^-23 gives sqrt(nn) = 1 - 2^-24): about half the normals, the ones compared
    for scale in (3.0, 1e-3):
        scaled, unit, fixed = gr.scaled_normals(nrm[:1000], seeds[:1000], scale)
        assert fixed.sum() >= 250
        assert np.array_equal(bits(gr.dirs(ref, scaled, 1)[fixed]), bits(gr.dirs(ref, unit, 1)[fixed]))


def test_sh9_basis_and_orthonormality(ref):
    """pt_amd.sh9_basis is the C file's basis bit for bit; over the sampler's own 2^16 directions
    (4 pi / N) sum Y_j Y_k is the identity within 6 standard errors per entry, the errors taken from the
    sample variance of each product.  The constants are six-digit roundings (0.282095^2 * 4 pi = 1 + 1.7e-6,
    and the sampler's 2 * 3.14159f leaves 5e-6 rad of the circle out), a bias that no sample count removes:
    each entry is allowed 1e-5 for it besides its 6 standard errors."""
    n = 1 << 16
    seeds = np.random.default_rng(gr.SEED + 9).integers(0, 2 ** 32, n, dtype=np.uint32)
    pts = pt_amd.gather_points(np.zeros((n, 3), F), None, seeds)
    d = gr.dirs(ref, pts, 0, "sh9")
    Y = pt_amd.sh9_basis(d)
    assert Y.dtype == F and Y.shape == (n, 9)
    assert np.array_equal(bits(Y[:4096]), bits(gr.sh9_basis(ref, d[:4096])))
    odd = np.array([(0.6, 0.0, -0.8), (0, 0, 1), (-1, 0, 0), (np.nan, 0.5, 0.5), (1e20, -1e20, 3)], F)
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(pt_amd.sh9_basis(odd)), bits(gr.sh9_basis(ref, odd)))
    Y64 = Y.astype(np.float64)
    for j in range(9):
        for k in range(j, 9):
            prod = 4.0 * np.pi * Y64[:, j] * Y64[:, k]
            mean, se = prod.mean(), prod.std(ddof=1) / np.sqrt(n)
            assert abs(mean - (1.0 if j == k else 0.0)) <= 6.0 * se + 1e-5, (j, k, mean, se)
    # the cosine-lobe convolution: a constant radiance L gives irradiance pi L whatever the normal
    coeffs = np.zeros((2, 3, 9))
    coeffs[:, :, 0] = 0.282095 * 4.0 * np.pi * np.array([1.0, 2.0, 0.5])
    e = pt_amd.sh9_irradiance(coeffs.reshape(2, 27), [(0, 0, 1), (0.6, 0.0, -0.8)])
    assert np.allclose(e, np.pi * np.array([1.0, 2.0, 0.5]), rtol=1e-5)
