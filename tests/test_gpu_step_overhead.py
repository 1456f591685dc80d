"""The fused step kernel's per-batch bookkeeping — 32-bit queue addressing (and its 64-bit instance),
region tails, and the ray reciprocals from ray_inv — against the CPU oracle.  Bar: bit-exact.

Shapes where addressing and region bookkeeping can go wrong: CornellBox at 40 x 24, 3 frames = 2,880
paths, depth 8, rr 0.9, rendered as the full image and as a crop window into a buffer whose rows are
wider than the window.  2,880 is 45 whole batches of 64 (and a part's 1,920 or 960 paths are whole
batches too), so the partial last camera batch comes from the crop — 29 x 17 = 493 pixels per frame —
and from a second image size, 41 x 23; the survivors' region tails are partial from the first bounce on
in every case.  One block (wf_trace_blocks = 1) makes one wave serve several batches of a region; two
parts offset every array of the second part.
Which addressing ran is read from pt_amd._lib.last_step_addr().
"""
import numpy as np
import pytest

import oracle
import pt_amd
from pt_amd import _lib

pytestmark = pytest.mark.gpu

W, H, FRAMES, DEPTH = 40, 24, 3, 8
WIN = (7, 4, 29, 17)  # x0, y0, w, h: odd sizes, 493 pixels per frame
PITCH = 37            # the crop's rows in its buffer: wider than the window
SENTINEL = -12345.5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """Bitwise equality, treating every NaN as equal to every NaN."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def report(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad = np.argwhere(~((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
    return f"{len(bad)} mismatches; first {bad[:5].tolist()}"


_ORACLE = {}


def reference(packed, scene, w=W, h=H):
    """oracle.render of the full image, once per scene and size."""
    if (scene, w, h) not in _ORACLE:
        p = packed[scene]
        _ORACLE[scene, w, h] = oracle.render(p.triangle_data, p.bvh_data, p.meta_for(w, h, rr=0.9), 0, FRAMES, 1, DEPTH)[0]
    return _ORACLE[scene, w, h]


def render_both(packed, scene, addr):
    """The scene through the fused pipeline as the full image and as the crop (row pitch PITCH), each
    against the oracle; both launches used `addr`-bit queue addressing."""
    torch = pytest.importorskip("torch")
    p = packed[scene]
    meta = p.meta_for(W, H, rr=0.9)
    ref = reference(packed, scene)
    x0, y0, w, h = WIN
    buf = torch.full((h, PITCH, 3), SENTINEL, dtype=torch.float32, device="cuda")
    buf[:, :w] = 0.0
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        full = s.render(meta, 0, FRAMES, 1, DEPTH, pt_amd.MODE_WAVEFRONT)
        assert _lib.last_bf_width() in (32, 64)  # the fused kernel (CornellBox: its narrow instance, the bench's)
        assert _lib.last_step_addr() == addr
        s.render_window_async(meta, WIN, 0, FRAMES, 1, DEPTH, pt_amd.MODE_WAVEFRONT, buf.data_ptr(), row_pitch=PITCH,
                              stream_ptr=st.cuda_stream)
        st.synchronize()
        s.check()
        assert _lib.last_step_addr() == addr
    assert full.mean() > 0
    assert same_bits(full, ref), report(full, ref)
    got = buf.cpu().numpy()
    want = ref[y0:y0 + h, x0:x0 + w]
    assert same_bits(got[:, :w], want), report(got[:, :w], want)
    assert np.all(got[:, w:] == np.float32(SENTINEL))


WAYS = {
    "one_block": {"parts": "1", "wf_trace_blocks": "1"},  # 8 waves: a wave serves several batches of its region
    "default_grid": {"parts": "1"},
    "two_parts": {"parts": "2"},  # 3 frames: a part of two frames and a part of one
}


@pytest.mark.parametrize("way", list(WAYS))
def test_cornell_full_and_crop(packed, ptopts, way):
    ptopts.set("kernel", "wavefront")
    for k, v in WAYS[way].items():
        ptopts.set(k, v)
    render_both(packed, "CornellBox", 32)


@pytest.mark.parametrize("way", list(WAYS))
def test_cornell_partial_last_camera_batch(packed, ptopts, way):
    """41 x 23 x 3 frames = 2,829 paths: 44 batches and 13 paths (parts of 1,886 and 943)."""
    ptopts.set("kernel", "wavefront")
    for k, v in WAYS[way].items():
        ptopts.set(k, v)
    p = packed["CornellBox"]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        got = s.render(p.meta_for(41, 23, rr=0.9), 0, FRAMES, 1, DEPTH, pt_amd.MODE_WAVEFRONT)
        assert _lib.last_step_addr() == 32
    ref = reference(packed, "CornellBox", 41, 23)
    assert same_bits(got, ref), report(got, ref)


@pytest.mark.parametrize("way", ["one_block", "two_parts"])
def test_cornell_forced_64_bit_addressing(packed, ptopts, way):
    ptopts.set("kernel", "wavefront")
    ptopts.set("step_addr64", "1")
    for k, v in WAYS[way].items():
        ptopts.set(k, v)
    render_both(packed, "CornellBox", 64)


@pytest.mark.parametrize("addr", [32, 64])
def test_mirror_specular_continuations(packed, ptopts, addr):
    ptopts.set("kernel", "wavefront")
    if addr == 64:
        ptopts.set("step_addr64", "1")
    render_both(packed, "CornellBox-Mirror", addr)


# ---------------------------------------------------------------------------------------------
# ray_inv on the device (pt_selftest_math "ray_inv"): triple i on thread i, so a wave votes on 64
# consecutive triples; every result against the IEEE 1.0f / x
# ---------------------------------------------------------------------------------------------
def f32(u):
    return np.array(u, np.uint32).view(np.float32)


LO, HI = 0x00800000, 0x7E000000  # 2^-126, 2^125: the reciprocal's verified range
SPECIAL_BITS = [0x00000000, 0x00000001, 0x00400000, 0x007FFFFF,  # zero, denormals (0x007fffff: 2^-126's lower neighbour)
                LO, LO + 1, HI - 1, HI, HI + 1,                      # the range's ends and their neighbours
                0x7F7FFFFF, 0x7F800000]                              # the largest finite value, infinity
SPECIALS = np.concatenate([f32(SPECIAL_BITS), f32([b | 0x80000000 for b in SPECIAL_BITS]), f32([0x7FC00000, 0xFFC00000, 0x7F800001])])


def ordinary(rng, n):
    """n unit vectors with no component near zero: every component deep inside the verified range."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = np.where(np.abs(v) < 1e-3, 0.5, v).astype(np.float32)
    assert np.all((np.abs(v) >= f32(LO)) & (np.abs(v) <= f32(HI)))
    return v


def test_ray_inv_equals_the_division():
    rng = np.random.default_rng(20261)
    nwaves = 64  # 4,096 triples
    d = ordinary(rng, nwaves * 64).reshape(nwaves, 64, 3)
    ns = len(SPECIALS)
    kind = []
    for wv in range(nwaves):
        if wv < 2 * ns:  # exactly one lane holds one special component among 63 ordinary lanes
            d[wv, (wv * 7 + 3) % 64, wv % 3] = SPECIALS[wv % ns]
            kind.append("one")
        elif wv < 2 * ns + 6:  # all ordinary
            kind.append("ordinary")
        elif wv == 2 * ns + 6:  # every component an end of the verified range or its inner neighbour, either
            # sign: the vote keeps the wave on the reciprocal, so the ends themselves go through it
            ends = f32([b | sg for b in (LO, LO + 1, HI - 1, HI) for sg in (0, 0x80000000)])
            d[wv] = ends[np.arange(64 * 3) * 5 % 8].reshape(64, 3)
            d[wv, :8, 0] = ends  # each of the eight at least once
            kind.append("ends")
        else:  # all special: every lane one, two or three special components
            for lane in range(64):
                for c in range(1 + (lane + wv) % 3):
                    d[wv, lane, (lane + c) % 3] = SPECIALS[(wv * 64 + lane * 3 + c) % ns]
            kind.append("special")
    assert kind.count("one") == 2 * ns and kind.count("ordinary") == 6 and kind.count("ends") == 1 and kind.count("special") >= 6
    flat = d.reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        want = (np.float32(1.0) / flat).astype(np.float32)
    got = pt_amd.selftest_math("ray_inv", flat)
    assert same_bits(got, want), report(got.reshape(-1, 3), want.reshape(-1, 3))
    # the fallback gives the axis-aligned directions their infinities, with the sign of the zero
    z = flat == 0
    assert z.any() and np.all(np.isinf(got[z])) and np.all(np.signbit(got[z]) == np.signbit(flat[z]))
