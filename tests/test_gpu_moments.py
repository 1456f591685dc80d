"""GPU: second moments beside the accumulator (pt_render_moments, pt_render_moments_async).

m2 = m2 + c * c with c = clamp(L), f32, frame after frame from the buffer's value: the reference is
numpy f32 over the oracle's frames (adaptive_ref.moments), every comparison bit for bit.  The
accumulator and the counters must be those of the call without moments.  Image, windows and frame
ranges are the window tests' (test_gpu_window.py): 40x24, A = (5, 3, 19, 7), B = (13, 9, 17, 11),
frames 3, 7, 11; each parity case asserts that its reference is not black.
"""
import numpy as np
import pytest

import pt_amd
from adaptive_ref import moments
from test_gpu_parity import ENV_KEYS, KERNELS, mismatch_report, same_bits
from test_gpu_window import A, B, DEPTH, EDGES, H, W, crop, ref_frame

pytestmark = pytest.mark.gpu

WHOLE = (0, 0, W, H)
MODES = {"megakernel": pt_amd.MODE_MEGAKERNEL, "wavefront": pt_amd.MODE_WAVEFRONT, "auto": pt_amd.MODE_AUTO}
# the three modes at the default options, then kernel variants under AUTO: the literal megakernel, a
# megakernel with the scene in global memory, two more megakernel flavours, separate trace and shade
# kernels (fuse=0), k_wf_generate instead of the fused kernel's camera batches, and the lean traversal
VARIANTS = ["megakernel", "wavefront", "auto", "literal", "mega_flat_global", "mega_lean_lds", "mega_nested",
            "wavefront_bf_nofuse", "wavefront_nogen", "wavefront_lean_lds", "wavefront_3parts_nofuse"]


@pytest.fixture
def defaults(ptopts):
    for k in ENV_KEYS:
        ptopts.unset(k, raising=False)
    return ptopts


def select(ptopts, variant):
    """The options of a variant; returns the mode to call with."""
    for k in ENV_KEYS:
        ptopts.unset(k, raising=False)
    if variant in MODES:
        return MODES[variant]
    for k, v in KERNELS[variant].items():
        ptopts.set(k, v)
    return pt_amd.MODE_AUTO


def ref_moments(packed, scene, win, salts, acc=None, m2=None):
    return moments([ref_frame(packed, scene, W, H, win, t) for t in salts], acc, m2)


def start(win, seed=7):
    rng = np.random.default_rng(seed)
    shape = (win[3], win[2], 3)
    return rng.uniform(0, 1, shape).astype(np.float32), rng.uniform(0, 2, shape).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# 1. parity of m2, the accumulator and the counters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [A, B, WHOLE], ids=["A", "B", "whole"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Sphere"])
def test_moments_bitexact(packed, ptopts, scene, variant, win):
    """frame0 3, 3 frames, stride 4, onto a random accumulator and a random m2; counted and plain."""
    mode = select(ptopts, variant)
    p = packed[scene]
    meta = p.meta_for(W, H)
    acc0, sq0 = start(win)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        cacc, cm2, ccnt = s.render_moments(meta, 3, 3, 4, DEPTH, mode, accum=acc0.copy(), m2=sq0.copy(), counters=True,
                                           window=win)
        pacc, pm2 = s.render_moments(meta, 3, 3, 4, DEPTH, mode, accum=acc0.copy(), m2=sq0.copy(), window=win)
        racc, rcnt = s.render(meta, 3, 3, 4, DEPTH, mode, accum=acc0.copy(), counters=True, window=win)
    zero_acc, zero_m2 = ref_moments(packed, scene, win, (3, 7, 11))
    assert zero_acc.mean() > 0 and zero_m2.mean() > 0
    ref_acc, ref_m2 = ref_moments(packed, scene, win, (3, 7, 11), acc0, sq0)
    assert same_bits(cm2, ref_m2), "counted m2: " + mismatch_report(cm2, ref_m2)
    assert same_bits(pm2, ref_m2), "plain m2: " + mismatch_report(pm2, ref_m2)
    assert same_bits(racc, ref_acc), mismatch_report(racc, ref_acc)
    assert cacc.tobytes() == racc.tobytes() and pacc.tobytes() == racc.tobytes()
    assert ccnt == rcnt, (ccnt, rcnt)
    assert ccnt["samples"] == win[2] * win[3] * 3


# ---------------------------------------------------------------------------------------------
# 2. several batches: m2 continues across k_wf_accum's calls as acc does
# ---------------------------------------------------------------------------------------------
BATCHES = [{}, {"wf_paths": 200, "fuse_gen": 0}, {"wf_paths": 200, "fuse_gen": 1}, {"parts": 3, "fuse_gen": 0},
           {"parts": 3, "fuse_gen": 1}]


@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Sphere"])
def test_moments_several_batches(packed, defaults, scene):
    """Window A (133 paths), 5 frames: wf_paths=200 makes batches of 2 + 2 + 1 frames, parts=3 up to
    three parts; the first entry is the single batch of the default options."""
    p = packed[scene]
    meta = p.meta_for(W, H)
    salts = [2 + 3 * k for k in range(5)]
    acc0, sq0 = start(A, 11)
    ref_acc, ref_m2 = ref_moments(packed, scene, A, salts, acc0, sq0)
    assert ref_moments(packed, scene, A, salts)[1].mean() > 0
    got = []
    for opts in BATCHES:
        for k in ("wf_paths", "parts", "fuse_gen"):
            defaults.unset(k)
        for k, v in opts.items():
            defaults.set(k, v)
        with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
            got.append(s.render_moments(meta, 2, 5, 3, DEPTH, pt_amd.MODE_WAVEFRONT, accum=acc0.copy(), m2=sq0.copy(),
                                        window=A))
        assert same_bits(got[-1][0], ref_acc), f"{opts} accum: " + mismatch_report(got[-1][0], ref_acc)
        assert same_bits(got[-1][1], ref_m2), f"{opts} m2: " + mismatch_report(got[-1][1], ref_m2)
    for acc, m2 in got[1:]:
        assert acc.tobytes() == got[0][0].tobytes() and m2.tobytes() == got[0][1].tobytes()


# ---------------------------------------------------------------------------------------------
# 3. in place with a row pitch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pt_amd.MODE_MEGAKERNEL, pt_amd.MODE_WAVEFRONT], ids=["megakernel", "wavefront"])
def test_moments_async_row_pitch(packed, defaults, mode):
    torch = pytest.importorskip("torch")
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    wins = (A, (24, 10, 16, 14))  # disjoint; the second touches the image's right and bottom edges
    sentinels = (-12345.5, -777.25)
    bufs = [torch.full((H, W, 3), v, dtype=torch.float32, device="cuda") for v in sentinels]
    for x0, y0, w, h in wins:
        for b in bufs:
            b[y0:y0 + h, x0:x0 + w] = 0.0
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for win in wins:
            off = 12 * (win[1] * W + win[0])
            s.render_moments_async(meta, 3, 3, 4, DEPTH, mode, bufs[0].data_ptr() + off, bufs[1].data_ptr() + off,
                                   stream_ptr=st.cuda_stream, window=win, row_pitch=W)
        st.synchronize()
        s.check()
        full_acc, full_m2 = s.render_moments(meta, 3, 3, 4, DEPTH, mode)
    ref_acc, ref_m2 = ref_moments(packed, "CornellBox", WHOLE, (3, 7, 11))
    assert same_bits(full_acc, ref_acc) and same_bits(full_m2, ref_m2), mismatch_report(full_m2, ref_m2)
    outside = np.ones((H, W), bool)
    for win in wins:
        outside[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] = False
    for buf, full, sentinel in zip(bufs, (full_acc, full_m2), sentinels):
        got = buf.cpu().numpy()
        for win in wins:
            assert crop(full, win).mean() > 0
            assert same_bits(crop(got, win), crop(full, win)), f"{win}: " + mismatch_report(crop(got, win), crop(full, win))
        assert np.all(got[outside] == np.float32(sentinel))


# ---------------------------------------------------------------------------------------------
# 4. edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", EDGES, ids=["corner00", "cornerWH", "row", "column", "64paths", "65paths"])
@pytest.mark.parametrize("kern", ["mega", "wavefront"])
def test_moments_edges(packed, defaults, win, kern):
    defaults.set("kernel", kern)
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    acc0, sq0 = start(win, 3)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        acc, m2 = s.render_moments(meta, 3, 3, 4, DEPTH, accum=acc0.copy(), m2=sq0.copy(), window=win)
    ref_acc, ref_m2 = ref_moments(packed, "CornellBox", win, (3, 7, 11), acc0, sq0)
    assert acc.shape == m2.shape == (win[3], win[2], 3)
    assert same_bits(acc, ref_acc), mismatch_report(acc, ref_acc)
    assert same_bits(m2, ref_m2), mismatch_report(m2, ref_m2)


# ---------------------------------------------------------------------------------------------
# 5. rejection
# ---------------------------------------------------------------------------------------------
def test_moments_bad_arguments_rejected_and_scene_stays_usable(packed, defaults):
    torch = pytest.importorskip("torch")
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    sq = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        with pytest.raises(pt_amd.PtError) as e:  # NULL m2
            s.render_moments_async(meta, 0, 1, 1, DEPTH, pt_amd.MODE_AUTO, acc.data_ptr(), 0)
        assert e.value.code == -1
        with pytest.raises(pt_amd.PtError) as e:  # NULL accumulator
            s.render_moments_async(meta, 0, 1, 1, DEPTH, pt_amd.MODE_AUTO, 0, sq.data_ptr())
        assert e.value.code == -1
        for win in ((30, 0, 11, 4), (0, 20, 4, 5), (0, 0, 0, 4), (0, 0, 4, 0), (W, 0, 1, 1), (0, H, 1, 1)):
            for call in (lambda: s.render_moments(meta, 0, 1, 1, DEPTH, window=win),
                         lambda: s.render_moments_async(meta, 0, 1, 1, DEPTH, pt_amd.MODE_AUTO, acc.data_ptr(),
                                                        sq.data_ptr(), window=win, row_pitch=W)):
                with pytest.raises(pt_amd.PtError) as e:
                    call()
                assert e.value.code == -1 and "window" in str(e.value), win
        for pitch in (A[2] - 1, 0):
            with pytest.raises(pt_amd.PtError) as e:
                s.render_moments_async(meta, 0, 1, 1, DEPTH, pt_amd.MODE_AUTO, acc.data_ptr(), sq.data_ptr(), window=A,
                                       row_pitch=pitch)
            assert e.value.code == -1 and "row_pitch" in str(e.value)
        with pytest.raises(pt_amd.PtError) as e:  # frames past 2^24
            s.render_moments(meta, (1 << 24) - 1, 2, 1, DEPTH)
        assert e.value.code == -1
        torch.cuda.synchronize()
        assert float(acc.abs().max()) == 0.0 and float(sq.abs().max()) == 0.0  # nothing was rendered
        gacc, gm2 = s.render_moments(meta, 3, 3, 4, DEPTH, window=A)
    ref_acc, ref_m2 = ref_moments(packed, "CornellBox", A, (3, 7, 11))
    assert ref_m2.mean() > 0
    assert same_bits(gacc, ref_acc), mismatch_report(gacc, ref_acc)
    assert same_bits(gm2, ref_m2), mismatch_report(gm2, ref_m2)
