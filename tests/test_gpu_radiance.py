"""GPU: the radiance queries (pt_query_radiance, pt_camera_seeds and their _async forms) against the
oracle's radiance() ray by ray (radiance_ref.py), bit for bit with NaN equal to NaN, through every
kernel set a render of the scene can take; the slot map's edge shapes; rays that are not admitted; the
composition law with pt_frame_window / pt_render_window; streams; errors."""
import numpy as np
import pytest

import cam_cases as cc
import pt_amd
import radiance_ref as rr
from test_gpu_parity import mismatch_report, same_bits
from test_gpu_query import C, IDS, SCENES, open_scene

pytestmark = pytest.mark.gpu

F = np.float32
# option sets a render of n paths per frame can run with; the boat's own below
SETS = {"default": {}, "trace_shade": {"kernel": "wavefront", "fuse": 0}, "no_lds": {"lds": 0}, "bf_wide": {"bf_narrow": 0},
        "bf_stack": {"bf_stackless": 0}, "no_region_perm": {"region_perm": 0}, "parts4": {"parts": 4},
        "addr64": {"step_addr64": 1}}
BOAT_SETS = {"leaf_pre0": {"leaf_pre": 0}, "leaf_pre1": {"leaf_pre": 1}, "no_chunk_walks": {"leaf_walk": 0},
             "leaf_pre1_no_chunk_walks": {"leaf_pre": 1, "leaf_walk": 0}}
MATRIX = [(s, vn, k) for s, vn in SCENES for k in list(SETS) + (list(BOAT_SETS) if s == "MedievalBoat" else [])]
QUERY_COUNTS = ("samples", "ext_queries", "shadow_queries")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("radiance_ref"))


def rr_of(packed, scene):
    return float(packed[scene].meta[45])


def check_counters(scene, got, want):
    """The oracle's sums; the boat: the query counts only (a cooperative big-leaf turn counts by wave)."""
    if scene == "MedievalBoat":
        assert {k: got[k] for k in QUERY_COUNTS} == {k: want[k] for k in QUERY_COUNTS}, (got, want)
    else:
        assert got == want, (got, want)


@pytest.mark.parametrize("scene,vn,kset", MATRIX, ids=[f"{s}{'-vn' if vn else ''}-{k}" for s, vn, k in MATRIX])
def test_parity(packed, ptopts, ref, scene, vn, kset):
    """Every family, 1 and 3 samples, added to a non-zero accumulator, the counting and the plain build."""
    for k, v in {**SETS, **BOAT_SETS}[kset].items():
        ptopts.set(k, v)
    init = rr.initial_accum()
    with open_scene(packed, scene, vn) as s:
        for family in rr.FAMILIES:
            fam = rr.family(scene, packed, family)
            for ns in (1, 3):
                want, adm, wcnt, _ = rr.reference(ref, scene, packed, family, ns, vn, init=True)
                counted, cnt = s.query_radiance(fam.rays, fam.seeds, ns, 8, rr_of(packed, scene), out=init, counters=True)
                plain = s.query_radiance(fam.rays, fam.seeds, ns, 8, rr_of(packed, scene), out=init)
                for got in (counted, plain):
                    assert same_bits(got, want), (family, ns, mismatch_report(got, want))
                check_counters(scene, cnt, wcnt)
                assert not same_bits(want[adm], init[adm])
        s.check()


@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Glossy"])
def test_slot_map_shapes(packed, ptopts, ref, scene):
    """n on both sides of a wave and of two, five samples in batches of 2 + 2 + 1 (wf_paths = 2 n on a fresh
    scene: a batch never holds fewer than two samples of a call that has two, so wf_paths below n gives
    the same batches), prefixes, and the empty calls."""
    fam = rr.family(scene, packed, "mixed")
    ps, rrp = packed[scene], rr_of(packed, scene)
    full, _, _, _ = rr.radiance(ref, ps, fam.rays, fam.seeds, 5, 8, rrp)
    for wf in (None, 2, 0.5):
        # one scene per setting, n ascending: the wavefront buffers only grow, to the 2 n paths of each call
        with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
            for n in (1, 63, 64, 65, 127, 129):
                if wf is not None:
                    ptopts.set("wf_paths", max(1, int(wf * n)))
                s.profile_enable(True)
                got, cnt = s.query_radiance(fam.rays[:n], fam.seeds[:n], 5, 8, rrp, counters=True)
                prof = s.profile_read()
                s.profile_enable(False)
                assert same_bits(got, full[:n]), (wf, n, mismatch_report(got, full[:n]))
                assert cnt["samples"] == 5 * int(rr.admitted(fam.rays[:n]).sum())
                assert prof["k_wf_accum"]["launches"] == (1 if wf is None else 3), (wf, n, prof["k_wf_accum"])
    with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
        sentinel = np.full((7, 3), -3.25, F)
        assert s.query_radiance(np.zeros((0, 8), F), np.zeros(0, np.uint32)).shape == (0, 3)
        got, cnt = s.query_radiance(fam.rays[:7], fam.seeds[:7], 0, 8, rrp, out=sentinel, counters=True)
        assert same_bits(got, sentinel) and not any(cnt.values())


@pytest.mark.parametrize("scene,vn", SCENES[:1] + SCENES[-1:], ids=IDS[:1] + IDS[-1:])
def test_rejected_rays(packed, ptopts, ref, scene, vn):
    """d = 0, a NaN and an infinite component, 2 d, d (1 +- 2^-10) and both sides of both edges of the band
    between admitted neighbours: the rejected rows keep their initial bits, the neighbours' rows are the
    reference's, samples counts the admitted rays alone, the call is PT_OK and the scene checks clean.
    These rays terminate by construction: the generate kernel makes no queue entry for them, so no
    kernel ever traces one (and the accumulate kernel skips their rows)."""
    good = rr.family(scene, packed, "probe")
    rays, seeds, names = [], [], []
    for k, (name, ray, adm) in enumerate(rr.rejected_rays(good.rays[0, 0:3], good.rays[0, 4:7])):
        rays += [good.rays[k], ray]
        seeds += [good.seeds[k], 12345 + k]
        names += ["good", name]
    rays, seeds = np.array(rays, F), np.array(seeds, np.uint32)
    init = rr.initial_accum(len(rays))
    init[3] = (-0.0, np.nan, np.inf)  # bits an addition of zero would not keep
    want, adm, wcnt, _ = rr.radiance(ref, packed[scene], rays, seeds, 3, 8, rr_of(packed, scene), False, init, vn)
    assert [names[i] for i in np.flatnonzero(adm)].count("good") == len(rays) // 2
    assert sorted(names[i] for i in np.flatnonzero(adm) if names[i] != "good") == ["edge_hi_in", "edge_lo_in"]
    with open_scene(packed, scene, vn) as s:
        got, cnt = s.query_radiance(rays, seeds, 3, 8, rr_of(packed, scene), out=init, counters=True)
        s.check()
    assert np.array_equal(got[~adm].view(np.uint32), init[~adm].view(np.uint32))
    assert same_bits(got, want), mismatch_report(got, want)
    assert cnt["samples"] == 3 * int(adm.sum())
    check_counters(scene, cnt, wcnt)


def test_composition_with_the_render(packed, ptopts):
    """camera_rays + camera_seeds + query_radiance(1 sample) = frame_window clamped, on the oblique camera
    and a window across the image's edges; frames 0..2 by three calls = render_window; camera_seeds = the
    CPU restatement."""
    scene = "CornellBox"
    meta = cc.meta_of(scene, "oblique")
    n = C[2] * C[3]
    with pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data) as s:
        acc = np.zeros((n, 3), F)
        for k in range(3):
            rays, seeds = s.camera_rays(meta, k, window=C), s.camera_seeds(meta, window=C, frame=k)
            want_rays, want_seeds = rr.camera_rays_seeds(meta, k, C)
            assert same_bits(rays, want_rays) and np.array_equal(seeds, want_seeds)
            one = s.query_radiance(rays.reshape(-1, 8), seeds, 1, cc.DEPTH, float(meta[45]), meta[46] > 0)
            frame = s.frame(meta, k, cc.DEPTH, window=C)
            clamped = (np.where(frame >= 0, frame, F(0)) + F(0)).astype(F)
            assert same_bits(one, clamped.reshape(-1, 3)), (k, mismatch_report(one, clamped.reshape(-1, 3)))
            acc = s.query_radiance(rays.reshape(-1, 8), seeds, 1, cc.DEPTH, float(meta[45]), meta[46] > 0, out=acc)
        want = s.render(meta, 0, 3, 1, cc.DEPTH, window=C)
        whole = s.camera_seeds(meta, frame=2)
    assert same_bits(acc, want.reshape(-1, 3)), mismatch_report(acc, want.reshape(-1, 3))
    assert (acc > 0).any()
    assert np.array_equal(whole[C[1]:C[1] + C[3], C[0]:C[0] + C[2]], seeds)


def test_async_streams_and_renders(packed, ptopts, ref):
    """Two calls with different ray lists back to back on one stream into two buffers, then on two
    streams; a render and a radiance query alternating on one scene, each against its own reference."""
    torch = pytest.importorskip("torch")
    scene = "CornellBox"
    ps, rrp = packed[scene], rr_of(packed, scene)
    fams = [rr.family(scene, packed, f) for f in ("texel", "mixed")]
    wants = [rr.reference(ref, scene, packed, f, 3, init=True)[0] for f in ("texel", "mixed")]
    d_rays = [torch.from_numpy(f.rays).cuda() for f in fams]
    d_seeds = [torch.from_numpy(f.seeds.view(np.int32)).cuda() for f in fams]
    meta = ps.meta_for(40, 24)
    with pt_amd.Scene(ps.triangle_data, ps.bvh_data) as s:
        for streams in ([torch.cuda.Stream()] * 2, [torch.cuda.Stream(), torch.cuda.Stream()]):
            d_acc = [torch.from_numpy(rr.initial_accum()).cuda() for _ in fams]
            d_cnt = torch.zeros((2, 6), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            for k in range(2):
                s.query_radiance_async(d_rays[k].data_ptr(), d_seeds[k].data_ptr(), rr.N, d_acc[k].data_ptr(), 3, 8, rrp,
                                       stream_ptr=streams[k].cuda_stream, d_counters_ptr=d_cnt.data_ptr() + 48 * k)
                if streams[0] is not streams[1]:
                    streams[k].synchronize()  # one scene's wavefront buffers serve one call at a time
            for st in streams:
                st.synchronize()
            s.check()
            for k in range(2):
                got = d_acc[k].cpu().numpy()
                assert same_bits(got, wants[k]), (k, mismatch_report(got, wants[k]))
                assert int(d_cnt[k, 0]) == 3 * int(rr.admitted(fams[k].rays).sum())
        image = s.render(meta, 0, 2, 1, 8)
        for k in range(2):
            got = s.query_radiance(fams[k].rays, fams[k].seeds, 3, 8, rrp, out=rr.initial_accum())
            assert same_bits(got, wants[k]), (k, mismatch_report(got, wants[k]))
            assert same_bits(s.render(meta, 0, 2, 1, 8), image)


def test_errors(packed, ptopts):
    """PT_ERR_INVALID with a message, before anything is allocated or launched."""
    torch = pytest.importorskip("torch")
    scene = "CornellBox"
    fam = rr.family(scene, packed, "texel")
    d = torch.zeros(1024, dtype=torch.float32, device="cuda")
    a = d.data_ptr()
    with pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data) as s:
        before = s.info["device_bytes"]
        for bad in (dict(n=(1 << 26) + 1), dict(n=4, max_depth=-1), dict(n=4, max_depth=1025), dict(n=4, rays=a + 4),
                    dict(n=4, seeds=a + 2), dict(n=4, acc=a + 1), dict(n=4, rays=0), dict(n=4, seeds=0), dict(n=4, acc=0)):
            with pytest.raises(pt_amd.PtError) as e:
                s.query_radiance_async(bad.get("rays", a), bad.get("seeds", a), bad["n"], bad.get("acc", a), 1,
                                       bad.get("max_depth", 8), 0.9)
            assert e.value.code == -1 and len(str(e.value)) > len("PT_ERR_INVALID: "), bad
        with pytest.raises(pt_amd.PtError):
            s.query_radiance(fam.rays[:4], fam.seeds[:4], 1, -1)
        with pytest.raises(pt_amd.PtError):
            s.query_radiance(fam.rays[:4], fam.seeds[:3])
        with pytest.raises(pt_amd.PtError):
            s.camera_seeds(packed[scene].meta_for(40, 24), frame=1 << 24)
        assert s.info["device_bytes"] == before
        s.check()
