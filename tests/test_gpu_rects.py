"""GPU: rectangle-list renders (pt_render_rects, pt_render_rects_async) against the oracle.

A list is a third slot -> pixel map beside the window's two, and nothing else: every pixel of a
rectangle carries the bits of the same pixel of the full render, so every comparison here is
`same_bits` (or integer equality) against the oracle's rows cropped to the rectangle, and everything
outside the rectangles keeps the bits it had.

The image is test_gpu_window's 40x24 (24x16 for the boat): no multiple of a 16x16 block, of a 64-path
batch or of the 8x8 wave tile.  The lists:
  L1  a one-pixel rectangle at the image's last pixel, A (133 pixels), a 17x10 one and a 3x2 one at
      the origin: 310 paths per frame, not in raster order, the borders inside 64-path batches
      (slots 1, 134, 304);
  L1F L1's shape inside the frame F = (2, 1, 30, 20) — L1 itself touches two corners of the image, so
      no smaller frame holds it: the one-pixel rectangle sits at F's last pixel and the 3x2 one at its
      origin, the slots are L1's;
  L2  window B alone;
  L3  8 of the image's 5x3 tiles of 8x8, every rectangle exactly one 64-path batch: the checkerboard's
      8 tiles, in its order, but with its four corner tiles — the image's outer columns are black in
      every scene here — moved one tile inward, which makes the ring around the centre tile;
  L4  the same over the 7x5 tiling, whose right tiles are 5 wide;
  LB  L1 for the boat's 24x16 image;
  BANDS  two full-width row bands, the only shape whose counters the oracle gives directly.

Counters: the oracle counts whole rows (oracle.render's y0, y1), so for BANDS the list's samples,
ext_queries and shadow_queries are compared with the oracle's sums, and for L1, L3 and L4 with the sum
of the per-rectangle counts of window renders (which test_gpu_window ties to the oracle's bands);
samples must also be pixels x frames.  The traversal counts depend on which rays share a batch
(render_tiled's docstring) and are not compared.

Light: every comparison asserts that the list's reference is not black, and every rectangle of at
least 64 pixels that its own reference is not: a black list cannot pass as equal.
"""
import functools

import numpy as np
import pytest

import adaptive_ref as ar
import oracle
import pt_amd
from test_gpu_parity import ENV_KEYS, KERNELS, mismatch_report, same_bits
from test_gpu_window import A, B, DEPTH, H, W, ref_frame, ref_render

pytestmark = pytest.mark.gpu

F = (2, 1, 30, 20)
L1 = ((39, 23, 1, 1), A, (13, 10, 17, 10), (0, 0, 3, 2))
L1F = ((31, 20, 1, 1), A, (13, 10, 17, 10), (2, 1, 3, 2))
L2 = (B,)
BANDS = ((0, 9, W, 11), (0, 0, W, 2))
LB = ((23, 15, 1, 1), A, (12, 10, 11, 6), (0, 0, 3, 2))
QUERIES = ("samples", "ext_queries", "shadow_queries")


def checkerboard(tile):
    tw, th = tile
    return tuple((x, y, min(tw, W - x), min(th, H - y)) for j, y in enumerate(range(0, H, th))
                 for i, x in enumerate(range(0, W, tw)) if (i + j) % 2 == 0)


L3 = tuple(((8, y, 8, 8) if x == 0 else (24, y, 8, 8) if x == 32 else (x, y, w, h)) for x, y, w, h in checkerboard((8, 8)))
L4 = checkerboard((7, 5))
LISTS = {"L1": L1, "L2": L2, "L3": L3, "L4": L4, "BANDS": BANDS}
_PACKED = {}


def start(w, h, seed=7):
    """The random accumulator (seed + 1: second moments) every list render starts from."""
    return np.random.default_rng(seed).uniform(0, 1, (h, w, 3)).astype(np.float32)


def paste(dst, rect, src, frame=(0, 0)):
    x0, y0, w, h = rect
    dst[y0 - frame[1]:y0 - frame[1] + h, x0 - frame[0]:x0 - frame[0] + w] = src


def cut(img, rect, frame=(0, 0)):
    x0, y0, w, h = rect
    return np.ascontiguousarray(img[y0 - frame[1]:y0 - frame[1] + h, x0 - frame[0]:x0 - frame[0] + w])


@functools.lru_cache(maxsize=None)
def _expected(scene, w, h, rects, frame0, nframes, stride, frame):
    """The accumulator and the second moments [frame.h, frame.w, 3] after the list render from start():
    the oracle's inside every rectangle, the start's bits outside.  Asserts the light."""
    p = _PACKED[scene]
    meta = p.meta_for(w, h)
    fx, fy, fw, fh = frame
    acc, m2 = start(fw, fh), start(fw, fh, 8)
    total = 0.0
    for r in rects:
        ref, _ = ref_render(p, meta, r, frame0, nframes, stride, DEPTH, cut(acc, r, frame))
        frames = [ref_frame(_PACKED, scene, w, h, r, frame0 + i * stride) for i in range(nframes)]
        again, sq = ar.moments(frames, cut(acc, r, frame), cut(m2, r, frame))
        assert same_bits(again, ref)  # the two references agree on the accumulator
        lit, _ = ar.moments(frames)
        if r[2] * r[3] >= 64:
            assert lit.mean() > 0, f"{scene}: rectangle {r} is black"
        total += float(lit.sum())
        paste(acc, r, ref, frame)
        paste(m2, r, sq, frame)
    assert total > 0, f"{scene}: the list is black"
    acc.setflags(write=False)
    m2.setflags(write=False)
    return acc, m2


def expected(packed, scene, w, h, rects, frame0=3, nframes=3, stride=4, frame=None):
    _PACKED[scene] = packed[scene]
    return _expected(scene, w, h, tuple(rects), frame0, nframes, stride, frame or (0, 0, w, h))


def set_kernel(ptopts, name):
    for k in ENV_KEYS:
        ptopts.unset(k, raising=False)
    for k, v in KERNELS[name].items():
        ptopts.set(k, v)


@pytest.fixture
def defaults(ptopts):
    for k in ENV_KEYS:
        ptopts.unset(k, raising=False)
    return ptopts


# ---------------------------------------------------------------------------------------------
# 1. bits against the oracle over the whole variant matrix
# ---------------------------------------------------------------------------------------------
def _check_list(packed, scene, w, h, rects, framed, label):
    p = packed[scene]
    meta = p.meta_for(w, h)
    ref, _ = expected(packed, scene, w, h, rects)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        got = s.render_rects(meta, rects, 3, 3, 4, DEPTH, accum=start(w, h))
        assert got.shape == (h, w, 3)
        assert same_bits(got, ref), f"{scene} {label}: " + mismatch_report(got, ref)
        if framed is not None:  # a frame that is not the image, a dense buffer of its size
            frame, frects = framed
            fref, _ = expected(packed, scene, w, h, frects, frame=frame)
            fgot = s.render_rects(meta, frects, 3, 3, 4, DEPTH, accum=start(frame[2], frame[3]), frame=frame)
            assert fgot.shape == (frame[3], frame[2], 3)
            assert same_bits(fgot, fref), f"{scene} {label} framed: " + mismatch_report(fgot, fref)


@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Sphere"])
@pytest.mark.parametrize("variant", list(KERNELS))
def test_rects_bitexact(packed, ptopts, variant, scene):
    """CornellBox: the fused kernel and the mailbox path; the sphere: k_wf_generate + k_wf_trace."""
    set_kernel(ptopts, variant)
    _check_list(packed, scene, W, H, L1, (F, L1F), variant)


@pytest.mark.parametrize("variant", ["auto", "wavefront_lean_lds"])
@pytest.mark.parametrize("scene,w,h,rects", [("CornellBox-Glossy", W, H, L1), ("MedievalBoat", 24, 16, LB)],
                         ids=["glossy", "boat"])
def test_rects_glossy_and_boat(packed, ptopts, variant, scene, w, h, rects):
    set_kernel(ptopts, variant)
    _check_list(packed, scene, w, h, rects, None, variant)


# ---------------------------------------------------------------------------------------------
# 2. second moments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pt_amd.MODE_MEGAKERNEL, pt_amd.MODE_WAVEFRONT, pt_amd.MODE_AUTO],
                         ids=["megakernel", "wavefront", "auto"])
@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Sphere"])
def test_rects_moments(packed, defaults, scene, mode):
    p = packed[scene]
    meta = p.meta_for(W, H)
    ref, ref2 = expected(packed, scene, W, H, L1)
    fref, fref2 = expected(packed, scene, W, H, L1F, frame=F)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        acc, m2, cnt = s.render_rects(meta, L1, 3, 3, 4, DEPTH, mode, accum=start(W, H), m2=start(W, H, 8), counters=True)
        facc, fm2 = s.render_rects(meta, L1F, 3, 3, 4, DEPTH, mode, accum=start(F[2], F[3]), m2=start(F[2], F[3], 8), frame=F)
    assert same_bits(acc, ref), mismatch_report(acc, ref)
    assert same_bits(m2, ref2), mismatch_report(m2, ref2)
    assert same_bits(facc, fref), mismatch_report(facc, fref)
    assert same_bits(fm2, fref2), mismatch_report(fm2, fref2)
    assert cnt["samples"] == 310 * 3


# ---------------------------------------------------------------------------------------------
# 3. the pipelines, counted and uncounted builds; the counters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pt_amd.MODE_MEGAKERNEL, pt_amd.MODE_WAVEFRONT, pt_amd.MODE_AUTO],
                         ids=["megakernel", "wavefront", "auto"])
@pytest.mark.parametrize("name", ["L1", "L3", "L4", "BANDS"])
def test_rects_modes_and_counters(packed, defaults, name, mode):
    rects = LISTS[name]
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    ref, _ = expected(packed, "CornellBox", W, H, rects)
    want = dict.fromkeys(QUERIES, 0)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        counted, cnt = s.render_rects(meta, rects, 3, 3, 4, DEPTH, mode, accum=start(W, H), counters=True)
        plain = s.render_rects(meta, rects, 3, 3, 4, DEPTH, mode, accum=start(W, H))
        for r in rects:
            if name == "BANDS":
                _, c = oracle.render(p.triangle_data, p.bvh_data, meta, 3, 3, 4, DEPTH, y0=r[1], y1=r[1] + r[3])
            else:
                _, c = s.render(meta, 3, 3, 4, DEPTH, pt_amd.MODE_MEGAKERNEL, counters=True, window=r)
            for k in QUERIES:
                want[k] += c[k]
    assert same_bits(counted, ref), mismatch_report(counted, ref)
    assert same_bits(plain, ref), mismatch_report(plain, ref)
    assert {k: cnt[k] for k in QUERIES} == want, (cnt, want)
    assert cnt["samples"] == 3 * sum(r[2] * r[3] for r in rects)
    assert cnt["shadow_queries"] > 0 and cnt["ext_queries"] > cnt["samples"]


def test_the_lists_are_what_the_docstring_says():
    first, npix = pt_amd.rect_plan(L1, W, H)
    assert npix == 310 and first.tolist() == [0, 1, 134, 304]
    assert pt_amd.rect_plan(L1F, W, H, frame=F)[0].tolist() == [0, 1, 134, 304]
    assert len(L3) == 8 and all(r[2] * r[3] == 64 for r in L3) and (16, 8, 8, 8) not in L3
    assert pt_amd.rect_plan(L3, W, H)[0].tolist() == list(range(0, 512, 64))
    assert len(L4) == 15 and {r[2] for r in L4} == {7, 5} and all(r[3] in (5, 4) for r in L4)
    assert pt_amd.rect_plan(LB, 24, 16)[1] == 1 + 133 + 66 + 6


# ---------------------------------------------------------------------------------------------
# 4. equivalence on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pt_amd.MODE_MEGAKERNEL, pt_amd.MODE_WAVEFRONT], ids=["megakernel", "wavefront"])
def test_one_rectangle_is_the_window_render(packed, defaults, mode):
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    init = start(W, H)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        lst, lc = s.render_rects(meta, L2, 3, 3, 4, DEPTH, mode, accum=init.copy(), counters=True)
        win, wc = s.render(meta, 3, 3, 4, DEPTH, mode, accum=cut(init, B), counters=True, window=B)
        framed = s.render_rects(meta, L2, 3, 3, 4, DEPTH, mode, accum=cut(init, B), frame=B)  # the frame is the rectangle
    zero, _ = ref_render(p, meta, B, 3, 3, 4, DEPTH)
    assert zero.mean() > 0
    assert cut(lst, B).tobytes() == win.tobytes() == framed.tobytes()
    assert {k: lc[k] for k in QUERIES} == {k: wc[k] for k in QUERIES}
    paste(lst, B, cut(init, B))
    assert lst.tobytes() == init.tobytes()  # nothing else changed


@pytest.mark.parametrize("mode", [pt_amd.MODE_MEGAKERNEL, pt_amd.MODE_WAVEFRONT], ids=["megakernel", "wavefront"])
def test_a_list_is_its_window_renders_pasted_together(packed, defaults, mode):
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    init = start(W, H)
    expected(packed, "CornellBox", W, H, L1)  # the light
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        lst = s.render_rects(meta, L1, 3, 3, 4, DEPTH, mode, accum=init.copy())
        pasted = init.copy()
        for r in L1:
            paste(pasted, r, s.render(meta, 3, 3, 4, DEPTH, mode, accum=cut(init, r), window=r))
    assert lst.tobytes() == pasted.tobytes()


# ---------------------------------------------------------------------------------------------
# 5. several batches, a ragged last one, parts
# ---------------------------------------------------------------------------------------------
# 7 frames of L1's 310 paths.  wf_paths 930 holds 3 frames: batches of 3 + 3 + 1 on one stream (parts
# 1); with parts 2 (and 4, which 930 paths cut down to 2) a part holds one frame: 2 + 2 + 2 + 1, the
# last batch with fewer frames than parts.  wf_paths 1240 with parts 4: 4 + 3, three of four parts.
BATCHES = [{"wf_paths": 930, "parts": 1}, {"wf_paths": 930, "parts": 2}, {"wf_paths": 930, "parts": 4},
           {"wf_paths": 1240, "parts": 4}, {"wf_paths": 930, "parts": 2, "fuse_gen": 0}, {"wf_paths": 930, "regen": 1}]


@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Sphere"])
def test_rects_several_batches(packed, defaults, scene):
    p = packed[scene]
    meta = p.meta_for(W, H)
    ref, ref2 = expected(packed, scene, W, H, L1, 2, 7, 3)
    for opts in BATCHES:
        for k in ("wf_paths", "parts", "fuse_gen", "regen"):
            defaults.unset(k)
        for k, v in opts.items():
            defaults.set(k, v)
        with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
            acc, m2 = s.render_rects(meta, L1, 2, 7, 3, DEPTH, pt_amd.MODE_WAVEFRONT, accum=start(W, H), m2=start(W, H, 8))
        assert same_bits(acc, ref), f"{opts}: " + mismatch_report(acc, ref)
        assert same_bits(m2, ref2), f"{opts}: " + mismatch_report(m2, ref2)


# ---------------------------------------------------------------------------------------------
# 6. the asynchronous call into a pitched device buffer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pt_amd.MODE_MEGAKERNEL, pt_amd.MODE_WAVEFRONT], ids=["megakernel", "wavefront"])
def test_rects_async_row_pitch(packed, defaults, mode):
    """40 columns inside 64-wide buffers that are NaN beyond them: the rectangles get the oracle's
    bits (no NaN was read into them), everything else keeps its own."""
    torch = pytest.importorskip("torch")
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    ref, ref2 = expected(packed, "CornellBox", W, H, L1)
    wide = [np.full((H, 64, 3), np.nan, np.float32) for _ in range(2)]
    wide[0][:, :W], wide[1][:, :W] = start(W, H), start(W, H, 8)
    d_acc, d_m2 = torch.from_numpy(wide[0]).cuda(), torch.from_numpy(wide[1]).cuda()
    d_only = torch.from_numpy(wide[0]).cuda()  # the call without moments
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        s.render_rects_async(meta, L1, 3, 3, 4, DEPTH, mode, d_acc.data_ptr(), d_m2.data_ptr(), row_pitch=64,
                             stream_ptr=st.cuda_stream)
        s.render_rects_async(meta, L1, 3, 3, 4, DEPTH, mode, d_only.data_ptr(), row_pitch=64, stream_ptr=st.cuda_stream)
        st.synchronize()
        s.check()
    for got, want in ((d_acc, ref), (d_m2, ref2), (d_only, ref)):
        g = got.cpu().numpy()
        assert same_bits(np.ascontiguousarray(g[:, :W]), want), mismatch_report(np.ascontiguousarray(g[:, :W]), want)
        assert np.all(np.isnan(g[:, W:]))


# ---------------------------------------------------------------------------------------------
# 7. rejections on the device path
# ---------------------------------------------------------------------------------------------
def test_bad_lists_rejected_and_buffers_untouched(packed, defaults):
    torch = pytest.importorskip("torch")
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    init = start(W, H)
    d_acc, d_m2 = torch.from_numpy(init).cuda(), torch.from_numpy(init).cuda()
    bad = [([A, B], None, "overlap"), ([A, (30, 20, 11, 2)], None, "outside"), ([A, (1, 3, 2, 2)], F, "outside the frame"),
           ([], None, "empty"), ([(7, 7, 0, 3)], None, "at least 1")]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for rects, frame, word in bad:
            w, h = (frame[2], frame[3]) if frame else (W, H)
            acc, m2 = np.ascontiguousarray(init[:h, :w]), np.ascontiguousarray(init[:h, :w])
            for call in (lambda: s.render_rects(meta, rects, 0, 2, 1, DEPTH, accum=acc, m2=m2, frame=frame),
                         lambda: s.render_rects_async(meta, rects, 0, 2, 1, DEPTH, pt_amd.MODE_AUTO, d_acc.data_ptr(),
                                                      d_m2.data_ptr(), row_pitch=W, frame=frame)):
                with pytest.raises(pt_amd.PtError) as e:
                    call()
                assert e.value.code == -1 and word in str(e.value), (rects, str(e.value))
            assert acc.tobytes() == init[:h, :w].tobytes() and m2.tobytes() == init[:h, :w].tobytes()
        with pytest.raises(pt_amd.PtError) as e:  # the pitch is checked against the frame's width
            s.render_rects_async(meta, [A], 0, 1, 1, DEPTH, pt_amd.MODE_AUTO, d_acc.data_ptr(), row_pitch=W - 1)
        assert e.value.code == -1 and "row_pitch" in str(e.value)
        torch.cuda.synchronize()
        assert d_acc.cpu().numpy().tobytes() == init.tobytes() and d_m2.cpu().numpy().tobytes() == init.tobytes()
        got = s.render_rects(meta, L1, 3, 3, 4, DEPTH, accum=init.copy())  # the scene is still usable
    ref, _ = expected(packed, "CornellBox", W, H, L1)
    assert same_bits(got, ref), mismatch_report(got, ref)
