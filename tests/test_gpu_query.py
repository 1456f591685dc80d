"""GPU: the ray queries (pt_query_hits, pt_query_occluded, pt_camera_rays and their _async forms) against
the oracle, ray by ray (query_ref.py: one oracle.intersect per ray, seeded batches that mix hits and
misses, the occlusion batch derived from the hits with tmax on both sides of every hit).

Every scene runs the default grid, one block (query_blocks=1: about 40 windows of 64 rays over 4 waves,
so the refill chain and the last partial window run), refill off, and the prefixes n = 1, 63, 64, 65
of the batch, whose results must be those of the same rays in the full batch."""
import numpy as np
import pytest

import denoise_ref as dr
import pt_amd
import query_ref as qr
from test_gpu_parity import mismatch_report, same_bits
from test_gpu_window import A, H, W, crop

pytestmark = pytest.mark.gpu

C = (24, 14, 16, 10)  # test_gpu_features.py's window across the box's right and bottom edges
# scene, vertex normals.  Glossy: the deep tree, no big leaves; the boat: its 7,327-entry leaf through the
# cooperative turn's division instance
SCENES = [("CornellBox", False), ("CornellBox-Glossy", False), ("CornellBox-Sphere", False), ("CornellBox-Sphere", True),
          ("MedievalBoat", False)]
RUNS = {"default": {}, "one_block": {"query_blocks": 1}, "no_refill": {"query_refill": 0},
        "one_block_no_refill": {"query_blocks": 1, "query_refill": 0}}
PREFIXES = (1, 63, 64, 65)
IDS = [f"{s}{'-vn' if vn else ''}" for s, vn in SCENES]


def open_scene(packed, scene, vn):
    s = pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data)
    if vn:
        s.set_vertex_normals(True)
    return s


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("scene,vn", SCENES, ids=IDS)
def test_hits_bitexact(packed, ptopts, scene, vn, run):
    """All eight values of every record, the counting and the plain build; the counters are the oracle's
    summed over the rays (the boat: the query counts only — a cooperative turn counts by wave)."""
    b = qr.batch(scene, packed, vn)
    assert b.hit.any() and not b.hit.all()
    for k, v in RUNS[run].items():
        ptopts.set(k, v)
    with open_scene(packed, scene, vn) as s:
        counted, cnt = s.query_hits(b.rays, counters=True)
        plain = s.query_hits(b.rays)
    for got in (counted, plain):
        assert got.shape == (len(b.rays), 8)
        assert not qr.hits_mismatch(got, b), qr.hits_mismatch(got, b)
    if scene == "MedievalBoat":
        assert (cnt["samples"], cnt["ext_queries"], cnt["shadow_queries"]) == (0, len(b.rays), 0), cnt
    else:
        assert cnt == b.counters, (cnt, b.counters)


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("scene,vn", SCENES, ids=IDS)
def test_occluded_bytes(packed, ptopts, scene, vn, run):
    """Byte for byte; early exit tests no more triangles than the closest-hit query of the same rays."""
    b = qr.batch(scene, packed, vn)
    assert b.occ.any() and not b.occ.all()
    for k, v in RUNS[run].items():
        ptopts.set(k, v)
    n = len(b.occ)
    with open_scene(packed, scene, vn) as s:
        counted, cnt = s.query_occluded(b.occ_rays, counters=True)
        plain = s.query_occluded(b.occ_rays)
        _, hcnt = s.query_hits(b.occ_rays, counters=True)
    for got in (counted, plain):
        assert got.dtype == np.uint8 and got.shape == (n,)
        bad = np.flatnonzero(got != b.occ)
        assert bad.size == 0, (bad.size, n, bad[:8], b.occ_rays[bad[:4]], got[bad[:8]], b.occ[bad[:8]])
    assert (cnt["samples"], cnt["ext_queries"], cnt["shadow_queries"]) == (0, 0, n), cnt
    assert hcnt["ext_queries"] == n and hcnt["shadow_queries"] == 0
    assert cnt["tri_tests"] <= hcnt["tri_tests"], (cnt, hcnt)
    if scene != "MedievalBoat":
        assert cnt["tri_tests"] < hcnt["tri_tests"] and cnt["nodes"] <= hcnt["nodes"], (cnt, hcnt)


@pytest.mark.parametrize("scene,vn", SCENES, ids=IDS)
def test_prefixes(packed, ptopts, scene, vn):
    """n = 1, 63, 64, 65 (one ray, one short window, exactly one, one and a ray) and the empty batch."""
    b = qr.batch(scene, packed, vn)
    with open_scene(packed, scene, vn) as s:
        for n in PREFIXES:
            got = s.query_hits(b.rays[:n])
            assert not qr.hits_mismatch(got, b, n), (n, qr.hits_mismatch(got, b, n))
            occ = s.query_occluded(b.occ_rays[:n])
            assert np.array_equal(occ, b.occ[:n]), (n, occ, b.occ[:n])
        assert s.query_hits(np.zeros((0, 8), np.float32)).shape == (0, 8)
        assert s.query_occluded(np.zeros((0, 8), np.float32)).shape == (0,)


def test_host_rays_at_any_alignment(packed, ptopts):
    """The blocking calls copy host buffers in, so rays, hits and bytes 4 bytes off a 16-byte boundary
    (a pt_ray on the stack, a view into a larger array) are as good as aligned ones."""
    import ctypes
    b = qr.batch("CornellBox", packed)
    n = 131
    raw = np.zeros(8 * n + 4, np.float32)
    rays = raw[(1 - raw.ctypes.data // 4) % 4:][:8 * n].reshape(n, 8)  # 4 bytes past a 16-byte boundary
    rays[:] = b.rays[:n]
    out_raw = np.zeros(8 * n + 4, np.float32)
    out = out_raw[(1 - out_raw.ctypes.data // 4) % 4:][:8 * n].reshape(n, 8)
    occ = np.zeros(n + 1, np.uint8)[1:]
    assert rays.ctypes.data % 16 == 4 and out.ctypes.data % 16 == 4 and rays.flags.c_contiguous
    p = ctypes.c_void_p
    with pt_amd.Scene(packed["CornellBox"].triangle_data, packed["CornellBox"].bvh_data) as s:
        assert s._lib.pt_query_hits(s._h, p(rays.ctypes.data), n, p(out.ctypes.data), None) == 0, s._lib.pt_last_error()
        assert s._lib.pt_query_occluded(s._h, p(rays.ctypes.data), n, p(occ.ctypes.data), None) == 0, s._lib.pt_last_error()
        got = s.query_hits(rays)  # the binding keeps a contiguous view where it is
    assert not qr.hits_mismatch(out, b, n), qr.hits_mismatch(out, b, n)
    assert not qr.hits_mismatch(got, b, n)
    assert np.array_equal(occ != 0, b.hit[:n])  # tmax of the hits batch: the reported hit


def test_batch_cut_into_launches(packed, ptopts):
    """A batch above the 2^22 rays of one launch (by one window and a ray): two launches, every result
    that of the same ray alone, the cut at a window boundary and the last partial window included."""
    scene = "CornellBox"
    b = qr.batch(scene, packed)
    n = (1 << 22) + 65
    reps = -(-n // len(b.rays))
    rays = np.tile(b.rays, (reps, 1))[:n]
    ref = np.tile(b.ref, (reps, 1))[:n]
    hit = np.tile(b.hit, reps)[:n]
    with pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data) as s:
        s.profile_enable(True)
        hits, cnt = s.query_hits(rays, counters=True)
        occ = s.query_occluded(rays)
        prof = s.profile_read()
        s.profile_enable(False)
    assert np.array_equal(hits.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(occ != 0, hit)
    assert cnt["ext_queries"] == n and cnt["samples"] == 0
    assert prof["k_query_hits"]["launches"] == 2 and prof["k_query_occluded"]["launches"] == 2, prof


def test_reserved_is_ignored_and_records_are_named(packed, ptopts):
    b = qr.batch("CornellBox", packed)
    rays = b.rays.copy()
    rays[:, 7:8].view(np.uint32)[:] = 0xDEADBEEF
    with pt_amd.Scene(packed["CornellBox"].triangle_data, packed["CornellBox"].bvh_data) as s:
        got = s.query_hits(rays.view(pt_amd.RAY_DTYPE).reshape(-1))
    assert not qr.hits_mismatch(got, b), qr.hits_mismatch(got, b)
    rec = got.view(pt_amd.HIT_DTYPE).reshape(-1)
    assert np.array_equal(rec["material"] >= 0, b.hit) and np.array_equal(rec["t"] > 0, b.hit)


def test_camera_rays_bitexact(packed, ptopts):
    """The whole 40 x 24 image and the windows A and C against denoise_ref.camera_ray; tmax = +inf,
    reserved = 0; frames >= 2^24 are rejected."""
    scene = "CornellBox"
    b = qr.batch(scene, packed)
    meta = packed[scene].meta_for(W, H)
    assert b.camera.shape == (H, W, 8)
    with pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data) as s:
        whole = s.camera_rays(meta, qr.FRAME)
        assert same_bits(whole, b.camera), mismatch_report(whole, b.camera)
        for win in (A, C):
            got = s.camera_rays(meta, qr.FRAME, window=win)
            assert got.shape == (win[3], win[2], 8)
            assert same_bits(got, crop(b.camera, win)), (win, mismatch_report(got, crop(b.camera, win)))
        other = s.camera_rays(meta, qr.FRAME + 1)
        assert not same_bits(other, whole) and same_bits(other[..., :4], whole[..., :4])  # the jitter moves d only
        with pytest.raises(pt_amd.PtError):
            s.camera_rays(meta, 1 << 24)
    assert np.all(np.isposinf(whole[..., 3])) and not whole[..., 7].view(np.uint32).any()
    o, d = dr.camera_ray(meta, 17, 11, qr.FRAME)
    assert same_bits(whole[11, 17, 0:3], o[:3]) and same_bits(whole[11, 17, 4:7], d[:3])


@pytest.mark.parametrize("scene,vn", [("CornellBox", False), ("CornellBox-Sphere", True)], ids=["CornellBox", "Sphere-vn"])
def test_camera_hits_are_the_guide_buffers(packed, ptopts, scene, vn):
    """query_hits(camera_rays(frame k)) gives per pixel the (n, t) one frame of render_features adds to
    zeroed buffers: the new path tied to an existing one without the oracle."""
    meta = packed[scene].meta_for(W, H)
    k = 5
    with open_scene(packed, scene, vn) as s:
        rays = s.camera_rays(meta, k)
        hits = s.query_hits(rays.reshape(-1, 8)).reshape(H, W, 8)
        geo, alb = s.render_features(meta, k, 1)
    hit = hits[..., 7].view(np.int32) >= 0
    assert hit.any() and not hit.all()
    assert np.array_equal(alb[..., 3] == 1.0, hit)
    # "adds to zeroed buffers": 0 + (-0) is +0, so a -0 normal component arrives as +0
    want = np.where(hit[..., None], np.float32(0) + hits[..., [4, 5, 6, 3]], np.float32(0))
    assert same_bits(geo, want), mismatch_report(geo, want)


def test_async_on_a_stream_inside_sentinels(packed, ptopts):
    """Device pointers on a non-default torch stream: the results land inside larger sentinel-filled
    buffers and nothing outside [0, n) changes; device counters are added to."""
    torch = pytest.importorskip("torch")
    scene = "CornellBox"
    b = qr.batch(scene, packed)
    n, m = len(b.rays), len(b.occ)
    sentinel = -12345.5
    d_rays = torch.from_numpy(b.rays).cuda()
    d_occ_rays = torch.from_numpy(b.occ_rays).cuda()
    d_hits = torch.full((n + 8, 8), sentinel, dtype=torch.float32, device="cuda")
    d_occ = torch.full((m + 37,), 0xA5, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((2, 6), 1000, dtype=torch.int64, device="cuda")
    d_cam = torch.full((H * W + 2, 8), sentinel, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data) as s:
        s.query_hits_async(d_rays.data_ptr(), n, d_hits.data_ptr() + 4 * 32, stream_ptr=st.cuda_stream,
                           d_counters_ptr=d_cnt.data_ptr())
        s.query_occluded_async(d_occ_rays.data_ptr(), m, d_occ.data_ptr() + 5, stream_ptr=st.cuda_stream,
                               d_counters_ptr=d_cnt.data_ptr() + 48)
        s.camera_rays_async(packed[scene].meta_for(W, H), qr.FRAME, d_cam.data_ptr() + 32, stream_ptr=st.cuda_stream)
        st.synchronize()
        s.check()
        with pytest.raises(pt_amd.PtError):
            s.query_hits_async(d_rays.data_ptr() + 4, 1, d_hits.data_ptr())
    hits, occ, cnt, cam = d_hits.cpu().numpy(), d_occ.cpu().numpy(), d_cnt.cpu().numpy(), d_cam.cpu().numpy()
    assert not qr.hits_mismatch(hits[4:4 + n], b), qr.hits_mismatch(hits[4:4 + n], b)
    assert np.all(hits[:4] == np.float32(sentinel)) and np.all(hits[4 + n:] == np.float32(sentinel))
    assert np.array_equal(occ[5:5 + m], b.occ) and np.all(occ[:5] == 0xA5) and np.all(occ[5 + m:] == 0xA5)
    c = b.counters
    assert list(cnt[0] - 1000) == [0, n, 0, c["nodes"], c["tri_tests"], c["box_tests"]], (cnt, c)
    assert list(cnt[1, :3] - 1000) == [0, 0, m] and 0 < cnt[1, 4] - 1000 < c["tri_tests"] * 4
    assert same_bits(cam[1:1 + H * W].reshape(H, W, 8), b.camera)
    assert np.all(cam[0] == np.float32(sentinel)) and np.all(cam[-1] == np.float32(sentinel))


def test_scratch_is_counted_and_kernels_are_named(packed, ptopts):
    """The blocking calls' device scratch is the scene's (device_bytes grows while it is held), and the
    profile names the three kernels."""
    scene = "CornellBox"
    b = qr.batch(scene, packed)
    with pt_amd.Scene(packed[scene].triangle_data, packed[scene].bvh_data) as s:
        before = s.info["device_bytes"]
        s.profile_enable(True)
        s.query_hits(b.rays)
        s.query_occluded(b.occ_rays)
        s.camera_rays(packed[scene].meta_for(W, H), 0)
        prof = s.profile_read()
        s.profile_enable(False)
        grown = s.info["device_bytes"] - before
    assert grown >= max(64 * len(b.rays), 33 * len(b.occ)), grown
    for name in ("k_query_hits", "k_query_occluded", "k_camera_rays"):
        assert name in prof and prof[name]["launches"] == 1, prof
