"""GPU: the denoiser (pt_denoise, pt_denoise_async, pt_render_denoised_image) against the numpy
reference (denoise_ref.py), out and var bit for bit, for 1..5 passes, both ways a pass can read its
taps (option denoise_lds: from global memory, or from the block's region staged in LDS) and two sets
of sigmas.

Shapes: (a) 40x24, the moments of 8 oracle frames with the reference's guide buffers — not a multiple
of the 16x16 block, and at step 16 (pass 5) a pixel has taps off both the top and the bottom; (b)
random positive buffers of 17x33 (block edges both ways), 5x3 and 1x1 (smaller than one halo) with
tiles of 16x8 whose frame counts run through 0, 1, 2, 5, 16 in 17x33 (the n = 0 and n < 2 rules; the
two single-tile images have 5 and 16 frames, so their buffers are positive) and with Q < S^2 / n on a
part of the pixels (the v = 0 branch).  The test asserts that no reference image is trivial."""
import functools

import numpy as np
import pytest

import adaptive_ref as ar
import denoise_ref as dr
import oracle
import pt_amd
from test_gpu_adaptive import FLOOR, FRACTION, TOL, simulate
from test_gpu_parity import mismatch_report, same_bits
from test_gpu_window import DEPTH, H, W, ref_frame

pytestmark = pytest.mark.gpu

WHOLE = (0, 0, W, H)
SCENE = "CornellBox"
ODD = dict(sigma_n=0.37, sigma_a=0.21, sigma_z=0.13, sigma_l=2.5)
SIGMAS = {"defaults": {k: v for k, v in dr.DEFAULTS.items() if k != "iters"}, "odd": ODD}
LDS = (0, 2, 4)
NFRAMES, FEATURE_FRAMES = 8, 4
_CACHE = {}


def oracle_inputs(packed):
    """(a): acc, m2 of frames 0..7, geo, alb of frames 0..3 (reference), computed once."""
    if "a" not in _CACHE:
        acc, m2 = ar.moments([ref_frame(packed, SCENE, W, H, WHOLE, k) for k in range(NFRAMES)])
        geo, alb, _ = dr.first_hits(SCENE, packed[SCENE], W, H).features(WHOLE, 0, FEATURE_FRAMES, 1)
        assert acc.mean() > 0 and 0 < alb[..., 3].sum() < W * H * FEATURE_FRAMES
        for a in (acc, m2, geo, alb):
            a.setflags(write=False)
        _CACHE["a"] = (acc, m2, geo, alb)
    return _CACHE["a"]


def oracle_passes(packed, sig):
    if ("a", sig) not in _CACHE:
        acc, m2, geo, alb = oracle_inputs(packed)
        _CACHE[("a", sig)] = dr.denoise_passes(acc, m2, NFRAMES, geo, alb, FEATURE_FRAMES, iters=5, **SIGMAS[sig])
    return _CACHE[("a", sig)]


@functools.lru_cache(maxsize=None)
def random_inputs(w, h):
    """(b): sums of up to 16 'frames' of random positive values per tile of 16x8, Q < S^2 / n on a
    fifth of the pixels, random guides; and the reference's five passes."""
    rng = np.random.default_rng(100 * w + h)
    tile = (16, 8)
    tx, ty = ar.tile_grid(w, h, tile)
    # 17x33's ten tiles run twice through 0, 1, 2, 5, 16; an image of a single tile has 5 (5x3) or 16 (1x1)
    # frames, so that its buffers are positive and the filter has something to weigh
    first = 0 if tx * ty > 1 else (3 if w * h > 1 else 4)
    fr = np.array([0, 1, 2, 5, 16], np.uint32)[(first + np.arange(tx * ty)) % 5].reshape(ty, tx)
    n = dr.frames_of_pixels(fr, w, h, tile).astype(np.float32)[..., None]
    mean = rng.uniform(0.05, 2.0, (h, w, 3)).astype(np.float32)
    acc = (mean * n).astype(np.float32)
    m2 = (mean * mean * n * rng.uniform(1.0, 1.5, (h, w, 3)).astype(np.float32)).astype(np.float32)
    low = rng.random((h, w)) < 0.2
    m2[low] = (m2[low] * np.float32(0.25)).astype(np.float32)
    ff = 3
    geo = np.concatenate([rng.uniform(-1, 1, (h, w, 3)) * ff, rng.uniform(0.5, 9.0, (h, w, 1)) * ff], axis=2).astype(np.float32)
    alb = np.concatenate([rng.uniform(0, 1, (h, w, 3)) * ff, np.full((h, w, 1), ff)], axis=2).astype(np.float32)
    S, Q = acc.astype(np.float64), m2.astype(np.float64)
    with np.errstate(all="ignore"):
        neg = (Q - S * S / n.astype(np.float64) < 0) & (n >= 2)
    passes = dr.denoise_passes(acc, m2, fr, geo, alb, ff, tile=tile, iters=5)
    mean0 = dr.prepare(acc, m2, dr.frames_of_pixels(fr, w, h, tile), geo, alb, ff)[0]  # what the first pass starts from
    return acc, m2, fr, geo, alb, ff, tile, passes, bool(neg.any()), bool((~neg & (n >= 2)).any()), mean0


def check(got, ref, what):
    out, var = got
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1]))
    assert same_bits(out, ref[0]), f"{what} out: " + mismatch_report(out, ref[0])
    assert same_bits(var, ref[1]), f"{what} var: " + mismatch_report(var, ref[1])


@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("sig", list(SIGMAS))
@pytest.mark.parametrize("iters", [1, 2, 3, 4, 5])
def test_denoise_oracle_inputs_bitexact(packed, ptopts, iters, sig, lds):
    p = packed[SCENE]
    acc, m2, geo, alb = oracle_inputs(packed)
    ref = oracle_passes(packed, sig)[iters - 1]
    ptopts.set("denoise_lds", lds)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        got = s.denoise(acc, m2, geo, alb, FEATURE_FRAMES, NFRAMES, params=dict(iters=iters, **SIGMAS[sig]))
    check(got, ref, f"iters {iters} {sig} lds {lds}")
    if iters == 1:  # the filter does something: the result is not the mean it started from
        assert not same_bits(got[0], acc / np.float32(NFRAMES))


def test_denoise_defaults_are_four_passes(packed, ptopts):
    p = packed[SCENE]
    acc, m2, geo, alb = oracle_inputs(packed)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        before = s.info["device_bytes"]
        got = s.denoise(acc, m2, geo, alb, FEATURE_FRAMES, NFRAMES)
        held = s.info["device_bytes"] - before
    check(got, oracle_passes(packed, "defaults")[3], "defaults")
    assert held == 4 * W * H * 16  # the scene holds the four float4 planes


@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("size", [(17, 33), (5, 3), (1, 1)], ids=["17x33", "5x3", "1x1"])
def test_denoise_random_buffers_bitexact(packed, ptopts, size, lds):
    p = packed[SCENE]
    w, h = size
    acc, m2, fr, geo, alb, ff, tile, passes, has_neg, has_pos, mean0 = random_inputs(w, h)
    if size == (17, 33):
        assert has_neg and has_pos and set(fr.ravel().tolist()) == {0, 1, 2, 5, 16}
    else:
        assert fr.min() >= 2 and mean0.min() > 0
    # the reference is no trivial image: positive somewhere at every size and, where the image has a
    # neighbour to weigh (more than one pixel), not the mean the filter started from
    for out, var in passes:
        assert out.max() > 0 and (w * h == 1 or not same_bits(out, mean0))
    assert passes[0][1].max() > 0
    ptopts.set("denoise_lds", lds)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for iters in range(1, 6):
            got = s.denoise(acc, m2, geo, alb, ff, fr, tile=tile, params=dict(iters=iters))
            check(got, passes[iters - 1], f"{w}x{h} iters {iters} lds {lds}")


@pytest.mark.parametrize("lds", [0, 4])
def test_denoise_async_pitched_with_sentinels(packed, ptopts, lds):
    """17 columns inside 24-wide device buffers: nothing right of the 17 columns is read (NaN in the
    inputs there) or written (a sentinel in the outputs)."""
    torch = pytest.importorskip("torch")
    p = packed[SCENE]
    w, h, pitch = 17, 33, 24
    acc, m2, fr, geo, alb, ff, tile, passes, _, _, _ = random_inputs(w, h)
    sentinel = -12345.5

    def padded(a, fill):
        b = np.full((h, pitch) + a.shape[2:], fill, np.float32)
        b[:, :w] = a
        return torch.from_numpy(b).cuda()

    d_acc, d_m2, d_geo, d_alb = (padded(a, np.nan) for a in (acc, m2, geo, alb))
    d_out = torch.full((h, pitch, 3), sentinel, dtype=torch.float32, device="cuda")
    d_var = torch.full((h, pitch), sentinel, dtype=torch.float32, device="cuda")
    d_fr = torch.from_numpy(fr.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ptopts.set("denoise_lds", lds)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        s.denoise_async(d_acc.data_ptr(), d_m2.data_ptr(), w, h, tile, d_fr.data_ptr(), d_geo.data_ptr(), d_alb.data_ptr(), ff,
                        d_out.data_ptr(), d_var.data_ptr(), params=dict(iters=3), row_pitch=pitch, stream_ptr=st.cuda_stream)
        st.synchronize()
        s.check()
    out, var = d_out.cpu().numpy(), d_var.cpu().numpy()
    check((out[:, :w], var[:, :w]), passes[2], f"pitched lds {lds}")
    assert np.all(out[:, w:] == np.float32(sentinel)) and np.all(var[:, w:] == np.float32(sentinel))


def test_render_denoised_is_the_reference_pipeline(packed, ptopts):
    """8 frames, 4 feature frames, the defaults: the tone map (sample_runs 1) of the reference's
    denoised image, byte for byte."""
    p = packed[SCENE]
    meta = p.meta_for(W, H)
    ref = oracle_passes(packed, "defaults")[3][0]
    want = oracle.tonemap(ref, 1).reshape(H, W, 4)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        rgba, cnt = s.render_denoised(meta, 0, NFRAMES, 1, DEPTH, feature_frames=FEATURE_FRAMES, counters=True)
        plain = s.render_denoised(meta, 0, NFRAMES, 1, DEPTH, feature_frames=FEATURE_FRAMES)
        raw = s.render_image(meta, 0, NFRAMES, 1, DEPTH)
    assert want[..., :3].max() > 0
    assert rgba.tobytes() == want.tobytes()
    assert plain.tobytes() == want.tobytes()
    assert raw.tobytes() != want.tobytes()
    assert cnt["samples"] == W * H * (NFRAMES + FEATURE_FRAMES)


def test_adaptive_then_denoise_matches_the_simulation(packed, ptopts):
    """render_adaptive -> render_features -> denoise(tile, tile_frames) equals the same composition over
    adaptive_ref's simulation of the driver."""
    p = packed[SCENE]
    meta = p.meta_for(W, H)
    tile, (lo, step, hi) = (8, 8), (4, 4, 16)
    sim = simulate(packed, SCENE, WHOLE, tile, (lo, step, hi))
    assert len(set(sim["tile_frames"].ravel().tolist())) >= 3
    fh = dr.first_hits(SCENE, packed[SCENE], W, H)
    geo, alb, _ = fh.features(WHOLE, 0, FEATURE_FRAMES, 1)
    ref = dr.denoise(sim["accum"], sim["m2"], sim["tile_frames"], geo, alb, FEATURE_FRAMES, tile=tile)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        r = s.render_adaptive(meta, 0, DEPTH, pt_amd.MODE_AUTO, tile=tile, min_frames=lo, step_frames=step, max_frames=hi,
                              tol=TOL, floor=FLOOR, noisy_fraction=FRACTION)
        g, a = s.render_features(meta, 0, FEATURE_FRAMES)
        got = s.denoise(r["accum"], r["m2"], g, a, FEATURE_FRAMES, r["tile_frames"], tile=tile)
    assert np.array_equal(r["tile_frames"], sim["tile_frames"])
    check(got, ref, "adaptive")
