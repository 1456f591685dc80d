"""GPU: the guide buffers of the first hit (pt_render_features, pt_render_features_async) against the
numpy reference (denoise_ref.FirstHits: the oracle's camera ray restated, the oracle's intersect).

The image, the windows and the frame range are test_gpu_window.py's: 40x24, A = (5, 3, 19, 7),
B = (13, 9, 17, 11), frame0 3, 3 frames, stride 4.  At 40x24 the box covers the pixels x 9..30,
y 5..22 and everything around it is a miss: A and the whole image hold hits and misses, and each such
case asserts both.  B lies inside the box entirely, so its reference cannot hold a miss (asserted too,
so that a change of the geometry shows); C = (24, 14, 16, 10) is B's counterpart across the box's
right and bottom edges and against the image's corner."""
import numpy as np
import pytest

import denoise_ref as dr
import oracle
import pt_amd
from test_gpu_parity import mismatch_report, same_bits
from test_gpu_window import A, B, H, W, crop

pytestmark = pytest.mark.gpu

WHOLE = (0, 0, W, H)
C = (24, 14, 16, 10)
FRAMES = (3, 3, 4)  # frame0, nframes, stride
WINDOWS = {"A": A, "B": B, "C": C, "whole": WHOLE}
ALL_HITS = {"B"}


def reference(packed, scene, win, geo=None, alb=None, vertex_normals=False):
    fh = dr.first_hits(scene, packed[scene], W, H, vertex_normals)
    oracle.set_vertex_normals(vertex_normals)
    try:
        return fh.features(win, *FRAMES, geo, alb)
    finally:
        oracle.set_vertex_normals(False)


def check_hits_and_misses(packed, scene, name, vertex_normals=False):
    _, alb, cnt = reference(packed, scene, WINDOWS[name], vertex_normals=vertex_normals)
    hits = int(alb[..., 3].sum())
    assert hits > 0
    assert (cnt["samples"] - hits == 0) if name in ALL_HITS else (cnt["samples"] - hits > 0), (name, hits, cnt)


@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Sphere"])
def test_features_bitexact(packed, ptopts, scene, win):
    """Onto random starting buffers, the counting and the plain build: geo, alb and every counter."""
    p = packed[scene]
    meta = p.meta_for(W, H)
    x0, y0, w, h = WINDOWS[win]
    rng = np.random.default_rng(11)
    g0 = rng.uniform(-1, 1, (h, w, 4)).astype(np.float32)
    a0 = rng.uniform(0, 1, (h, w, 4)).astype(np.float32)
    check_hits_and_misses(packed, scene, win)
    rg, ra, rc = reference(packed, scene, WINDOWS[win], g0, a0)
    window = None if win == "whole" else WINDOWS[win]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        cg, ca, cc = s.render_features(meta, *FRAMES, geo=g0.copy(), alb=a0.copy(), counters=True, window=window)
        pg, pa = s.render_features(meta, *FRAMES, geo=g0.copy(), alb=a0.copy(), window=window)
    assert cg.shape == (h, w, 4) and ca.shape == (h, w, 4)
    for got, ref in ((cg, rg), (pg, rg), (ca, ra), (pa, ra)):
        assert same_bits(got, ref), mismatch_report(got, ref)
    assert cc == rc, (cc, rc)
    assert cc["samples"] == cc["ext_queries"] == w * h * FRAMES[1] and cc["shadow_queries"] == 0


def test_features_vertex_normals(packed, ptopts):
    """The sphere's smooth normals (po_set_vertex_normals governs po_intersect: its leaf test takes the
    vertex-normal triangle test): window B holds the sphere, and the normals differ from the flat ones."""
    scene = "CornellBox-Sphere"
    p = packed[scene]
    meta = p.meta_for(W, H)
    check_hits_and_misses(packed, scene, "whole", vertex_normals=True)
    rg, ra, rc = reference(packed, scene, WHOLE, vertex_normals=True)
    flat, _, _ = reference(packed, scene, WHOLE)
    assert not same_bits(rg, flat) and same_bits(rg[..., 3], flat[..., 3])
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        s.set_vertex_normals(True)
        g, a, c = s.render_features(meta, *FRAMES, counters=True)
        s.set_vertex_normals(False)
        g2, _ = s.render_features(meta, *FRAMES)
    assert same_bits(g, rg), mismatch_report(g, rg)
    assert same_bits(a, ra), mismatch_report(a, ra)
    assert c == rc, (c, rc)
    assert same_bits(g2, flat), mismatch_report(g2, flat)


def test_features_boat_big_leaves(packed, ptopts):
    """MedievalBoat (24x16, window A as in test_gpu_window.py): the scene's big leaves take the
    cooperative turns of the megakernel's big-leaf flavour.  geo and alb bit for bit; of the counters
    only the queries (the cooperative turns' traversal counts depend on which rays share a wave)."""
    scene, w, h = "MedievalBoat", 24, 16
    p = packed[scene]
    meta = p.meta_for(w, h)
    rg, ra, rc = dr.first_hits(scene, p, w, h).features(A, *FRAMES)
    assert ra[..., 3].sum() > 0
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        g, a, c = s.render_features(meta, *FRAMES, counters=True, window=A)
        g2, a2 = s.render_features(meta, *FRAMES, window=A)
    for got, ref in ((g, rg), (g2, rg), (a, ra), (a2, ra)):
        assert same_bits(got, ref), mismatch_report(got, ref)
    assert (c["samples"], c["ext_queries"], c["shadow_queries"]) == (rc["samples"], rc["ext_queries"], 0)


def test_features_async_in_place_row_pitch(packed, ptopts):
    """Windows rendered in place inside full [H, W, 4] images filled with a sentinel: row_pitch = W,
    nothing outside the windows changes."""
    torch = pytest.importorskip("torch")
    scene = "CornellBox"
    p = packed[scene]
    meta = p.meta_for(W, H)
    wins = (A, C)  # disjoint; C touches the image's right and bottom edges
    sentinel = -12345.5
    geo = torch.full((H, W, 4), sentinel, dtype=torch.float32, device="cuda")
    alb = torch.full((H, W, 4), sentinel, dtype=torch.float32, device="cuda")
    for x0, y0, w, h in wins:
        geo[y0:y0 + h, x0:x0 + w] = 0.0
        alb[y0:y0 + h, x0:x0 + w] = 0.0
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for win in wins:
            off = 16 * (win[1] * W + win[0])
            s.render_features_async(meta, *FRAMES, geo.data_ptr() + off, alb.data_ptr() + off, stream_ptr=st.cuda_stream,
                                    window=win, row_pitch=W)
        st.synchronize()
        s.check()
    gg, ga = geo.cpu().numpy(), alb.cpu().numpy()
    outside = np.ones((H, W), bool)
    for win in wins:
        rg, ra, _ = reference(packed, scene, win)
        assert rg[..., 3].sum() > 0
        assert same_bits(crop(gg, win), rg), f"{win}: " + mismatch_report(crop(gg, win), rg)
        assert same_bits(crop(ga, win), ra), f"{win}: " + mismatch_report(crop(ga, win), ra)
        outside[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] = False
    assert np.all(gg[outside] == np.float32(sentinel)) and np.all(ga[outside] == np.float32(sentinel))
