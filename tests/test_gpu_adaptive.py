"""GPU: the tile noise estimate, the per-tile mean and the adaptive driver (pt_noise_tiles[_async],
pt_tile_mean_async, pt_render_adaptive) against numpy (adaptive_ref.py).

The estimate is double arithmetic with every operation rounded once in a fixed order, its per-tile
count and maximum do not depend on the reduction's order, and a tile that has received n frames
holds the bits of that rectangle of a plain n-frame render — so every comparison is exact: integer
equality, same_bits, or equality of max_err's bits.  The driver is compared with a numpy simulation
of itself over the oracle's frames.
"""
import collections
import functools

import numpy as np
import pytest

import adaptive_ref as ar
import pt_amd
from test_gpu_parity import ENV_KEYS, mismatch_report, same_bits
from test_gpu_window import B, DEPTH, H, W, ref_frame

pytestmark = pytest.mark.gpu

WHOLE = (0, 0, W, H)
TOL, FLOOR, FRACTION = 0.5, 0.05, 0.05
MODES = {"megakernel": pt_amd.MODE_MEGAKERNEL, "wavefront": pt_amd.MODE_WAVEFRONT, "auto": pt_amd.MODE_AUTO}


@pytest.fixture
def defaults(ptopts):
    for k in ENV_KEYS:
        ptopts.unset(k, raising=False)
    return ptopts


def same_noise(got, ref):
    """Tile verdicts equal: the counts, and max_err bit for bit."""
    return (got.shape == ref.shape and np.array_equal(got["noisy"], ref["noisy"]) and
            np.array_equal(got["pixels"], ref["pixels"]) and
            np.array_equal(np.ascontiguousarray(got["max_err"]).view(np.uint64),
                           np.ascontiguousarray(ref["max_err"]).view(np.uint64)))


# ---------------------------------------------------------------------------------------------
# 6. pt_noise_tiles against numpy on synthetic accumulators
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic():
    """40x24 sums of 5 'frames' of random positive values, then the special pixels and regions (the
    16x16 tiling's tiles: (0,0) Q < S^2/n everywhere, (1,0) all zero; single NaN and inf pixels)."""
    rng = np.random.default_rng(2240)
    c = rng.gamma(0.6, 0.8, (5, H, W, 3)).astype(np.float32)
    c[:, :, 20:] *= np.float32(0.05)  # a dark half: the floor decides there
    acc, m2 = ar.moments(list(c))
    m2[0:16, 0:16] = acc[0:16, 0:16] * acc[0:16, 0:16] / np.float32(8)  # below S^2 / 5: clamped to 0
    acc[0:16, 16:32] = 0
    m2[0:16, 16:32] = 0
    m2[20, 3, 1] = np.nan
    m2[21, 3, 0] = np.inf
    acc[5, 36, 2] = np.nan
    acc.setflags(write=False)
    m2.setflags(write=False)
    return acc, m2


def synthetic_frames(tile):
    """5 frames everywhere but two tiles: the last has 1, the one before it 0 (where there are three)."""
    tx, ty = ar.tile_grid(W, H, tile)
    fr = np.full((ty, tx), 5, np.uint32)
    if fr.size >= 3:
        fr.flat[-1], fr.flat[-2] = 1, 0
    return fr


@pytest.mark.parametrize("tile", [(16, 16), (7, 5), (1, 1), (64, 64)], ids=lambda t: f"{t[0]}x{t[1]}")
def test_noise_tiles_matches_numpy(packed, defaults, tile):
    torch = pytest.importorskip("torch")
    acc, m2 = synthetic()
    fr = synthetic_frames(tile)
    ref = ar.noise_tiles(acc, m2, tile, fr, 0.4, 0.3)
    if tile == (16, 16):  # the synthetic cases are what they claim to be
        assert ref[0, 0]["noisy"] == 0 and ref[0, 0]["max_err"] == 0.0  # variance clamped to 0
        assert ref[0, 1]["noisy"] == 0 and ref[0, 1]["max_err"] == 0.0  # all zero
        assert ref[1, 2]["noisy"] == ref[1, 2]["pixels"] == 64 and np.isinf(ref[1, 2]["max_err"])  # 1 frame
        assert np.isinf(ref[1, 1]["max_err"]) and ref[1, 1]["noisy"] == 128  # 0 frames
        assert np.isinf(ref[1, 0]["max_err"]) and 0 < ref[1, 0]["noisy"] < 128  # the inf pixel
        assert [int(v) for v in ref["pixels"].ravel()] == [256, 256, 128, 128, 128, 64]
    if tile == (7, 5):
        assert 0 < ref["noisy"].sum() < W * H and len(set(ref["noisy"].ravel().tolist())) > 3
    p = packed["CornellBox"]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        host = s.noise_tiles(acc, m2, tile, fr, 0.4, 0.3)
        d_acc, d_m2 = torch.from_numpy(acc.copy()).cuda(), torch.from_numpy(m2.copy()).cuda()
        d_fr = torch.from_numpy(fr.astype(np.int32)).cuda()
        d_out = torch.zeros(fr.size * 2, dtype=torch.float64, device="cuda")
        s.noise_tiles_async(d_acc.data_ptr(), d_m2.data_ptr(), W, H, tile, d_fr.data_ptr(), 0.4, 0.3, d_out.data_ptr())
        torch.cuda.synchronize()
        dev = d_out.cpu().numpy().view(ar.TILE_NOISE_DTYPE).reshape(fr.shape)
    assert same_noise(host, ref), (host, ref)
    assert same_noise(dev, ref), (dev, ref)


def test_noise_tiles_and_mean_pitched(packed, defaults):
    """40 columns inside a 64-wide buffer: the verdicts are the dense buffer's, and nothing outside
    the 40 columns is read (NaN there) or, for the mean, written."""
    torch = pytest.importorskip("torch")
    acc, m2 = synthetic()
    tile = (16, 16)
    fr = synthetic_frames(tile)
    ref = ar.noise_tiles(acc, m2, tile, fr, 0.4, 0.3)
    wide = [np.full((H, 64, 3), np.nan, np.float32) for _ in range(2)]
    wide[0][:, :W], wide[1][:, :W] = acc, m2
    clean = np.where(np.isnan(wide[0]), np.float32(1.5), wide[0])  # the mean's input: no NaN (its payload is not pinned)
    ref_mean = ar.tile_mean(clean[:, :W], tile, fr)
    p = packed["CornellBox"]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        d_acc, d_m2 = torch.from_numpy(wide[0]).cuda(), torch.from_numpy(wide[1]).cuda()
        d_fr = torch.from_numpy(fr.astype(np.int32)).cuda()
        d_out = torch.zeros(fr.size * 2, dtype=torch.float64, device="cuda")
        d_mean = torch.full((H, 64, 3), -5.5, dtype=torch.float32, device="cuda")
        s.noise_tiles_async(d_acc.data_ptr(), d_m2.data_ptr(), W, H, tile, d_fr.data_ptr(), 0.4, 0.3, d_out.data_ptr(),
                            row_pitch=64)
        d_clean = torch.from_numpy(clean).cuda()
        s.tile_mean_async(d_clean.data_ptr(), W, H, tile, d_fr.data_ptr(), d_mean.data_ptr(), row_pitch=64)
        torch.cuda.synchronize()
        dev = d_out.cpu().numpy().view(ar.TILE_NOISE_DTYPE).reshape(fr.shape)
        mean = d_mean.cpu().numpy()
    assert same_noise(dev, ref), (dev, ref)
    assert same_bits(np.ascontiguousarray(mean[:, :W]), ref_mean), mismatch_report(np.ascontiguousarray(mean[:, :W]), ref_mean)
    assert np.all(mean[:, W:] == np.float32(-5.5))


# ---------------------------------------------------------------------------------------------
# 7. pt_tile_mean_async
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [(16, 16), (7, 5), (1, 1), (64, 64)], ids=lambda t: f"{t[0]}x{t[1]}")
def test_tile_mean_matches_numpy(packed, defaults, tile):
    torch = pytest.importorskip("torch")
    acc = np.nan_to_num(synthetic()[0], nan=1.5)  # a NaN's payload is not pinned
    tx, ty = ar.tile_grid(W, H, tile)
    fr = np.random.default_rng(5).integers(1, 300, (ty, tx)).astype(np.uint32)
    fr.flat[0] = 0
    if fr.size > 1:
        fr.flat[-1] = 3
    ref = ar.tile_mean(acc, tile, fr)
    n = ar.frames_of_pixels(fr, W, H, tile)
    with np.errstate(all="ignore"):  # the quotient where frames are 0 is not looked at
        quotient = acc / n.astype(np.float32)[..., None]
    assert np.all(ref[n == 0] == 0) and same_bits(ref[n > 0], quotient[n > 0])
    p = packed["CornellBox"]
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        d_acc = torch.from_numpy(acc.copy()).cuda()
        d_fr = torch.from_numpy(fr.astype(np.int32)).cuda()
        d_mean = torch.full((H, W, 3), -5.5, dtype=torch.float32, device="cuda")
        s.tile_mean_async(d_acc.data_ptr(), W, H, tile, d_fr.data_ptr(), d_mean.data_ptr())
        torch.cuda.synchronize()
        mean = d_mean.cpu().numpy()
    assert same_bits(mean, ref), mismatch_report(mean, ref)


# ---------------------------------------------------------------------------------------------
# 8. the driver against a numpy simulation of itself over the oracle's frames
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _simulate(scene, win, tile, frames):
    lo, step, hi = frames
    r = ar.simulate(lambda k: ref_frame(_simulate.packed, scene, W, H, win, k), win[2], win[3], tile, 0, lo, step, hi,
                    TOL, FLOOR, FRACTION)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def simulate(packed, scene, win, tile, frames):
    _simulate.packed = packed
    return _simulate(scene, win, tile, frames)


def check_driver(packed, scene, win, tile, frames, mode, expect=None):
    lo, step, hi = frames
    sim = simulate(packed, scene, win, tile, frames)
    counts = dict(collections.Counter(int(v) for v in sim["tile_frames"].ravel()))
    # a run where every tile stops at once, or none does, must not pass
    assert len(counts) >= 3 and lo in counts and hi in counts, counts
    if expect is not None:
        assert counts == expect, counts
    assert sim["accum"].mean() > 0
    p = packed[scene]
    meta = p.meta_for(W, H)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        r = s.render_adaptive(meta, 0, DEPTH, mode, window=None if win == WHOLE else win, tile=tile, min_frames=lo,
                              step_frames=step, max_frames=hi, tol=TOL, floor=FLOOR, noisy_fraction=FRACTION,
                              counters=True)
    assert np.array_equal(r["tile_frames"], sim["tile_frames"]), (r["tile_frames"], sim["tile_frames"])
    assert same_bits(r["accum"], sim["accum"]), mismatch_report(r["accum"], sim["accum"])
    assert same_bits(r["m2"], sim["m2"]), mismatch_report(r["m2"], sim["m2"])
    assert same_noise(r["tile_noise"], sim["tile_noise"]), (r["tile_noise"], sim["tile_noise"])
    assert r["passes"] == sim["passes"]
    n = ar.frames_of_pixels(sim["tile_frames"], win[2], win[3], tile)
    assert r["counters"]["samples"] == int(n.astype(np.int64).sum())
    assert np.array_equal(r["rgba"], pt_amd.tonemap(ar.tile_mean(sim["accum"], tile, sim["tile_frames"]), 1))


CASES = [
    ("CornellBox", (8, 8), (4, 4, 16), {4: 7, 8: 1, 12: 3, 16: 4}),
    ("CornellBox-Sphere", (8, 8), (4, 4, 16), {4: 9, 8: 2, 12: 3, 16: 1}),
    ("CornellBox-Glossy", (8, 8), (4, 4, 16), {4: 7, 8: 4, 16: 4}),
    ("CornellBox", (16, 16), (4, 4, 16), {4: 2, 8: 2, 16: 2}),
    ("CornellBox", (7, 5), (4, 4, 16), {4: 16, 8: 2, 12: 4, 16: 8}),
    ("CornellBox-Sphere", (8, 8), (2, 3, 9), {2: 7, 5: 2, 8: 2, 9: 4}),  # the clamped last pass: 8 + 1
]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("scene,tile,frames,expect", CASES,
                         ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}-{'_'.join(map(str, c[2]))}" for c in CASES])
def test_adaptive_matches_simulation(packed, defaults, scene, tile, frames, expect, mode):
    check_driver(packed, scene, WHOLE, tile, frames, MODES[mode], expect)


@pytest.mark.parametrize("mode", list(MODES))
def test_adaptive_on_a_window(packed, defaults, mode):
    """Window B of the image: the tiles are the window's, the rays the image's."""
    check_driver(packed, "CornellBox", B, (8, 8), (4, 4, 16), MODES[mode], {4: 3, 8: 1, 16: 2})


# ---------------------------------------------------------------------------------------------
# 9. degenerate drivers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["megakernel", "wavefront"])
def test_adaptive_large_tol_is_one_pass(packed, defaults, mode):
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        r = s.render_adaptive(meta, 0, DEPTH, MODES[mode], tile=(8, 8), min_frames=4, step_frames=4, max_frames=16,
                              tol=1.0e6, floor=FLOOR, noisy_fraction=FRACTION, counters=True)
        acc, m2, cnt = s.render_moments(meta, 0, 4, 1, DEPTH, MODES[mode], counters=True)
    assert r["passes"] == 1 and np.all(r["tile_frames"] == 4) and np.all(r["tile_noise"]["noisy"] == 0)
    assert acc.mean() > 0
    assert r["accum"].tobytes() == acc.tobytes() and r["m2"].tobytes() == m2.tobytes()
    assert r["counters"] == cnt


@pytest.mark.parametrize("mode", ["megakernel", "wavefront"])
def test_adaptive_tiny_tol_reaches_max_frames(packed, defaults, mode):
    """Every tile with a pixel of non-zero variance runs to max_frames and holds the plain render's
    bits; a tile without one (all its pixels black or constant) stops after pass 0."""
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    tile = (8, 8)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        r = s.render_adaptive(meta, 0, DEPTH, MODES[mode], tile=tile, min_frames=4, step_frames=5, max_frames=16,
                              tol=1.0e-12, floor=FLOOR, noisy_fraction=0.0)
        full = s.render(meta, 0, 16, 1, DEPTH, MODES[mode])
        first = s.render(meta, 0, 4, 1, DEPTH, MODES[mode])
    n = ar.frames_of_pixels(r["tile_frames"], W, H, tile)
    assert set(np.unique(r["tile_frames"]).tolist()) <= {4, 16} and (r["tile_frames"] == 16).sum() >= 8
    assert r["passes"] == 4  # 4, +5, +5, +2
    lit = n == 16
    assert full[lit].mean() > 0
    assert same_bits(r["accum"][lit], full[lit]), mismatch_report(r["accum"][lit], full[lit])
    assert same_bits(r["accum"][~lit], first[~lit])
    assert np.all(r["tile_noise"]["noisy"][r["tile_frames"] == 4] == 0)
