"""GPU: the irradiance gathers (pt_gather, pt_gather_rays and their _async forms) against the reference
point by point (gather_ref.py), bit for bit with NaN equal to NaN, in both modes through every kernel set a
render of the scene can take; the slot map's edge shapes; composition over sample ranges and with the
radiance queries; points that are not admitted; normals of any length; vertex normals; streams; errors."""
import numpy as np
import pytest

import gather_ref as gr
import pt_amd
import radiance_ref as rr
from test_gpu_parity import mismatch_report, same_bits
from test_gpu_query import open_scene
from test_gpu_radiance import check_counters, rr_of

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = ["CornellBox", "CornellBox-Glossy", "CornellBox-Sphere", "MedievalBoat"]
SETS = {"default": {}, "trace_shade": {"kernel": "wavefront", "fuse": 0}, "no_lds": {"lds": 0}, "bf_wide": {"bf_narrow": 0},
        "no_region_perm": {"region_perm": 0}, "parts4": {"parts": 4}, "addr64": {"step_addr64": 1}}
BOAT_SETS = {"leaf_pre0": {"leaf_pre": 0}, "leaf_pre1": {"leaf_pre": 1}, "no_chunk_walks": {"leaf_walk": 0}}
MATRIX = [(s, k) for s in SCENES for k in list(SETS) + (list(BOAT_SETS) if s == "MedievalBoat" else [])]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return gr.build(tmp_path_factory.mktemp("gather_ref"))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def gather(s, g, ns, mode, rrp, **kw):
    return s.gather(g.p, g.n, g.seeds, ns, mode=mode, max_depth=8, rr=rrp, **kw)


@pytest.mark.parametrize("scene,kset", MATRIX, ids=[f"{s}-{k}" for s, k in MATRIX])
def test_parity(packed, ptopts, ref, scene, kset):
    """Both modes, 1 and 3 samples (the boat 8), added to a non-zero accumulator, the counting and the
    plain build."""
    for k, v in {**SETS, **BOAT_SETS}[kset].items():
        ptopts.set(k, v)
    with open_scene(packed, scene, False) as s:
        for mode in gr.MODES:
            g = gr.points(scene, packed, mode)
            init = gr.initial_accum(gr.N, gr.width(mode))
            for ns in gr.samples(scene):
                want, adm, wcnt, _ = gr.reference(ref, scene, packed, mode, ns, init=True)
                counted, cnt = gather(s, g, ns, mode, rr_of(packed, scene), out=init, counters=True)
                plain = gather(s, g, ns, mode, rr_of(packed, scene), out=init)
                for got in (counted, plain):
                    assert same_bits(got, want), (mode, ns, mismatch_report(got, want))
                check_counters(scene, cnt, wcnt)
                assert cnt["samples"] == int(adm.sum()) == ns * gr.N
                assert not same_bits(want, init)
        s.check()


@pytest.mark.parametrize("mode", gr.MODES)
@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Glossy"])
def test_slot_map_shapes(packed, ptopts, ref, scene, mode):
    """n on both sides of a wave and of two, five samples in one batch and (wf_paths = 2 n on a fresh scene)
    in batches of 2 + 2 + 1, and the empty calls."""
    g = gr.points(scene, packed, mode)
    ps, rrp = packed[scene], rr_of(packed, scene)
    full, _, fcnt, _ = gr.gather(ref, ps, g.packed, 5, 0, mode, 8, rrp)
    for wf in (None, 2):
        with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
            for n in (1, 63, 64, 65, 129):
                if wf is not None:
                    ptopts.set("wf_paths", wf * n)
                s.profile_enable(True)
                got, cnt = s.gather(g.p[:n], g.n[:n], g.seeds[:n], 5, mode=mode, max_depth=8, rr=rrp, counters=True)
                prof = s.profile_read()
                s.profile_enable(False)
                assert same_bits(got, full[:n]), (wf, n, mismatch_report(got, full[:n]))
                assert cnt["samples"] == 5 * n
                assert prof["k_wf_accum"]["launches"] == (1 if wf is None else 3), (wf, n, prof["k_wf_accum"])
                if n == gr.N:
                    check_counters(scene, cnt, fcnt)
    with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
        w = gr.width(mode)
        sentinel = np.full((7, w), -3.25, F)
        assert s.gather(np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, np.uint32), 3, mode=mode).shape == (0, w)
        got, cnt = s.gather(g.p[:7], g.n[:7], g.seeds[:7], 0, mode=mode, out=sentinel, counters=True)
        assert same_bits(got, sentinel) and not any(cnt.values())


@pytest.mark.parametrize("mode", gr.MODES)
@pytest.mark.parametrize("scene", ["CornellBox", "MedievalBoat"])
def test_sample_ranges_compose(packed, ptopts, ref, scene, mode):
    """Samples 0..2 then 2..5 into the same buffer equal samples 0..5, and equal the reference."""
    g = gr.points(scene, packed, mode)
    rrp = rr_of(packed, scene)
    init = gr.initial_accum(gr.N, gr.width(mode))
    want, _, _, _ = gr.gather(ref, packed[scene], g.packed, 5, 0, mode, 8, rrp, False, init)
    with open_scene(packed, scene, False) as s:
        whole = gather(s, g, 5, mode, rrp, out=init)
        first = gather(s, g, 2, mode, rrp, out=init)
        both = gather(s, g, 3, mode, rrp, out=first, sample0=2)
        s.check()
    assert same_bits(both, whole), mismatch_report(both, whole)
    assert same_bits(whole, want), mismatch_report(whole, want)
    assert not same_bits(first, whole)


@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Sphere"])
def test_gather_rays_and_radiance_queries_repeat_a_cosine_gather(packed, ptopts, ref, scene):
    """gather_rays = the reference's restatement, in both modes; gather_rays + query_radiance(1 sample),
    sample by sample, = the COSINE gather."""
    g = gr.points(scene, packed)
    rrp = rr_of(packed, scene)
    init = gr.initial_accum()
    with open_scene(packed, scene, False) as s:
        want = gather(s, g, 3, "cosine", rrp, out=init)
        acc = init
        for k in range(3):
            rays, seeds = s.gather_rays(g.p, g.n, g.seeds, k, "cosine")
            wrays, wseeds = gr.rays(ref, g.packed, k)
            assert same_bits(rays, wrays) and np.array_equal(seeds, wseeds), k
            acc = s.query_radiance(rays, seeds, 1, 8, rrp, out=acc)
        g9 = gr.points(scene, packed, "sh9")
        rays9, seeds9 = s.gather_rays(g9.p, None, g9.seeds, 4, "sh9")
        wrays9, wseeds9 = gr.rays(ref, g9.packed, 4, "sh9")
        s.check()
    assert same_bits(acc, want), mismatch_report(acc, want)
    assert same_bits(rays9, wrays9) and np.array_equal(seeds9, wseeds9)
    assert same_bits(rays9[:, 0:3], g9.p) and rr.admitted(rays9).all()


def rejected_normals(n):
    """[(name, normal)]: normals that no COSINE point is admitted with, from an admitted unit normal n."""
    n = np.asarray(n, F)
    return [("zero", np.zeros(3, F)), ("nan", np.array((np.nan, n[1], n[2]), F)), ("inf", np.array((n[0], np.inf, n[2]), F)),
            ("tiny", (n * F(2.0 ** -50)).astype(F)), ("huge", (n * F(2.0 ** 50)).astype(F))]


@pytest.mark.parametrize("scene", ["CornellBox", "MedievalBoat"])
def test_rejected_points(packed, ptopts, ref, scene):
    """Normals of length 0, NaN, infinity, 2^-50 and 2^50 between admitted neighbours, on accumulator
    words -0, NaN and infinity: the rejected rows keep their bits, the neighbours' rows are the
    reference's, samples counts the admitted samples alone; gather_rays gives them d = 0 and seed 0.
    SH9 ignores the normals: every point is admitted."""
    good = gr.points(scene, packed)
    p, nrm, seeds, names = [], [], [], []
    for k, (name, bad) in enumerate(rejected_normals(good.n[0])):
        p += [good.p[2 * k], good.p[2 * k + 1]]
        nrm += [good.n[2 * k], bad]
        seeds += [good.seeds[2 * k], 777 + k]
        names += ["good", name]
    p += [good.p[10]]
    nrm += [good.n[10]]
    seeds += [good.seeds[10]]
    g = gr.Points(p, nrm, seeds)
    n = len(p)
    rej = np.arange(1, n, 2)
    rrp = rr_of(packed, scene)
    init = gr.initial_accum(n)
    init[1] = (-0.0, np.nan, np.inf)
    init[3] = (np.inf, -0.0, -np.inf)
    init[5] = (np.nan, np.nan, -0.0)
    want, adm, wcnt, _ = gr.gather(ref, packed[scene], g.packed, 3, 0, "cosine", 8, rrp, False, init)
    assert np.array_equal(np.flatnonzero(adm == 0), rej) and (adm[::2] == 3).all()
    init9 = gr.initial_accum(n, 27)
    want9, adm9, wcnt9, _ = gr.gather(ref, packed[scene], g.packed, 3, 0, "sh9", 8, rrp, False, init9)
    assert (adm9 == 3).all()
    with open_scene(packed, scene, False) as s:
        got, cnt = gather(s, g, 3, "cosine", rrp, out=init, counters=True)
        rays, rseeds = s.gather_rays(g.p, g.n, g.seeds, 1, "cosine")
        got9, cnt9 = gather(s, g, 3, "sh9", rrp, out=init9, counters=True)
        s.check()
    assert np.array_equal(bits(got[rej]), bits(init[rej]))
    assert same_bits(got, want), mismatch_report(got, want)
    assert cnt["samples"] == int(adm.sum()) == 3 * (n - len(rej))
    check_counters(scene, cnt, wcnt)
    assert (rays[rej, 4:7] == 0).all() and (rseeds[rej] == 0).all() and (rseeds[::2] != 0).all()
    assert np.array_equal(bits(rays[rej, 0:3]), bits(g.p[rej]))
    assert same_bits(got9, want9), mismatch_report(got9, want9)
    assert cnt9["samples"] == 3 * n
    check_counters(scene, cnt9, wcnt9)


def test_normals_of_any_length(packed, ptopts, ref):
    """Normals of length 3 and 1e-3 give the result of their normalised copies — where that copy is its own
    normalised copy, bit for bit (gather_ref.scaled_normals) — and always the reference's."""
    scene = "CornellBox"
    g = gr.points(scene, packed)
    rrp = rr_of(packed, scene)
    with open_scene(packed, scene, False) as s:
        for scale in (3.0, 1e-3):
            scaled, unit, fixed = gr.scaled_normals(g.n, g.seeds, scale, g.p)
            assert fixed.sum() >= 32
            a = s.gather(g.p, scaled[:, 4:7], g.seeds, 3, max_depth=8, rr=rrp)
            b = s.gather(g.p, unit[:, 4:7], g.seeds, 3, max_depth=8, rr=rrp)
            want, adm, _, _ = gr.gather(ref, packed[scene], scaled, 3, 0, "cosine", 8, rrp)
            assert (adm == 3).all()
            assert same_bits(a, want), (scale, mismatch_report(a, want))
            assert same_bits(a[fixed], b[fixed]), scale
            assert (a > 0).any()
        s.check()


@pytest.mark.parametrize("mode", gr.MODES)
def test_vertex_normals_on_the_sphere(packed, ptopts, ref, mode):
    scene = "CornellBox-Sphere"
    g = gr.points(scene, packed, mode)
    want, _, wcnt, _ = gr.reference(ref, scene, packed, mode, 3, True, init=True)
    flat, _, _, _ = gr.reference(ref, scene, packed, mode, 3, False, init=True)
    assert not same_bits(want, flat)
    with open_scene(packed, scene, True) as s:
        got, cnt = gather(s, g, 3, mode, rr_of(packed, scene), out=gr.initial_accum(gr.N, gr.width(mode)), counters=True)
        s.check()
    assert same_bits(got, want), mismatch_report(got, want)
    check_counters(scene, cnt, wcnt)


def test_async_on_a_stream(packed, ptopts, ref):
    """The async form on a torch stream, both modes back to back into their own buffers, equals the
    blocking form; device counters are added to."""
    torch = pytest.importorskip("torch")
    scene = "CornellBox"
    ps, rrp = packed[scene], rr_of(packed, scene)
    st = torch.cuda.Stream()
    with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
        for mode in gr.MODES:
            g = gr.points(scene, packed, mode)
            w = gr.width(mode)
            init = gr.initial_accum(gr.N, w)
            want, wcnt = gather(s, g, 3, mode, rrp, out=init, counters=True)
            ref_want, _, _, _ = gr.reference(ref, scene, packed, mode, 3, init=True)
            assert same_bits(want, ref_want)
            d_pts = torch.from_numpy(g.packed).cuda()
            d_acc = torch.from_numpy(init).cuda()
            d_cnt = torch.zeros(6, dtype=torch.int64, device="cuda")
            d_rays = torch.zeros((gr.N, 8), dtype=torch.float32, device="cuda")
            d_seeds = torch.zeros(gr.N, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            s.gather_async(d_pts.data_ptr(), gr.N, d_acc.data_ptr(), 2, 0, mode, 8, rrp, stream_ptr=st.cuda_stream,
                           d_counters_ptr=d_cnt.data_ptr())
            s.gather_async(d_pts.data_ptr(), gr.N, d_acc.data_ptr(), 1, 2, mode, 8, rrp, stream_ptr=st.cuda_stream,
                           d_counters_ptr=d_cnt.data_ptr())
            s.gather_rays_async(d_pts.data_ptr(), gr.N, 1, d_rays.data_ptr(), d_seeds.data_ptr(), mode, st.cuda_stream)
            st.synchronize()
            s.check()
            got = d_acc.cpu().numpy()
            assert same_bits(got, want), (mode, mismatch_report(got, want))
            assert {k: int(d_cnt[i]) for i, k in enumerate(wcnt)} == wcnt
            wrays, wseeds = gr.rays(ref, g.packed, 1, mode)
            assert same_bits(d_rays.cpu().numpy(), wrays)
            assert np.array_equal(d_seeds.cpu().numpy().view(np.uint32), wseeds)


def test_errors(packed, ptopts):
    """Every rule of the header: PT_ERR_INVALID with a message, nothing allocated, launched or touched."""
    torch = pytest.importorskip("torch")
    scene = "CornellBox"
    g = gr.points(scene, packed)
    d = torch.full((1024,), -3.25, dtype=torch.float32, device="cuda")
    a = d.data_ptr()
    with pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data) as s:
        before = s.info["device_bytes"]
        for bad in (dict(n=(1 << 26) + 1), dict(n=4, max_depth=-1), dict(n=4, max_depth=1025), dict(n=4, pts=a + 4),
                    dict(n=4, acc=a + 1), dict(n=4, pts=0), dict(n=4, acc=0), dict(n=4, mode=2),
                    dict(n=4, sample0=(1 << 31) - 1, nsamples=2), dict(n=4, sample0=1 << 31, nsamples=1)):
            with pytest.raises(pt_amd.PtError) as e:
                s.gather_async(bad.get("pts", a), bad["n"], bad.get("acc", a), bad.get("nsamples", 1), bad.get("sample0", 0),
                               bad.get("mode", 0), bad.get("max_depth", 8), 0.9)
            assert e.value.code == -1 and len(str(e.value)) > len("PT_ERR_INVALID: "), bad
        for bad in (dict(mode=2), dict(sample=1 << 31), dict(pts=a + 4), dict(rays=a + 8), dict(seeds=a + 2), dict(rays=0)):
            with pytest.raises(pt_amd.PtError) as e:
                s.gather_rays_async(bad.get("pts", a), 4, bad.get("sample", 0), bad.get("rays", a), bad.get("seeds", a),
                                    bad.get("mode", 0))
            assert e.value.code == -1, bad
        with pytest.raises(pt_amd.PtError):
            s.gather(g.p[:4], g.n[:4], g.seeds[:4], 1, max_depth=-1)
        with pytest.raises(pt_amd.PtError):
            s.gather(g.p[:4], g.n[:4], g.seeds[:3], 1)
        with pytest.raises(pt_amd.PtError):
            s.gather(g.p[:4], g.n[:4], g.seeds[:4], 1, mode="sh4")
        with pytest.raises(pt_amd.PtError):
            s.gather(g.p[:4], g.n[:4], g.seeds[:4], 1, out=np.zeros((4, 27), F))
        torch.cuda.synchronize()
        assert s.info["device_bytes"] == before
        assert bool((d == -3.25).all())
        s.check()
