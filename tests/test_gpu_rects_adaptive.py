"""GPU: pt_render_adaptive renders every refinement pass as ONE list render (pt_render_rects_async)
over the rectangles of its active tiles, not one window render per rectangle.

Seen through the scene's kernel profile: in wavefront mode every render call ends each of its batches
with one k_wf_accum launch, and a pass of these sizes is one batch — so the launches of k_wf_accum
equal the passes.  With a render call per rectangle they equal 1 + the rectangles summed over the
refinement passes, which is more for both cases here (asserted: a pass has at least two rectangles).
The results stay what test_gpu_adaptive.py pins: the bits of the numpy simulation over the oracle.
"""
import numpy as np
import pytest

import pt_amd
from test_gpu_adaptive import FLOOR, FRACTION, TOL, WHOLE, same_noise, simulate
from test_gpu_parity import ENV_KEYS, mismatch_report, same_bits
from test_gpu_window import DEPTH, H, W

pytestmark = pytest.mark.gpu

CASES = [("CornellBox", (8, 8), (4, 4, 16)), ("CornellBox-Sphere", (8, 8), (2, 3, 9))]


def pass_rects(tile_frames, frames):
    """The rectangles (in tiles) of every refinement pass, rebuilt from the final frame counts: a tile
    is active in a pass iff it ended with more frames than every active tile had before the pass."""
    lo, step, hi = frames
    out, done = [], lo
    while done < hi and (tile_frames > done).any():
        out.append(pt_amd.tile_rects(tile_frames > done))
        done += min(step, hi - done)
    return out


@pytest.mark.parametrize("scene,tile,frames", CASES, ids=[c[0] for c in CASES])
def test_one_accumulation_launch_per_pass(packed, ptopts, scene, tile, frames):
    for k in ENV_KEYS:
        ptopts.unset(k, raising=False)
    lo, step, hi = frames
    sim = simulate(packed, scene, WHOLE, tile, frames)
    rects = pass_rects(sim["tile_frames"], frames)
    assert len(rects) == sim["passes"] - 1
    for mine, theirs in zip(rects, sim["rects"]):  # the simulation's own log agrees
        assert np.array_equal(mine, theirs)
    assert max(len(r) for r in rects) >= 2, "every pass is a single rectangle: the test shows nothing"
    per_rectangle = 1 + sum(len(r) for r in rects)
    assert per_rectangle > sim["passes"]
    p = packed[scene]
    meta = p.meta_for(W, H)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        s.profile_enable()
        r = s.render_adaptive(meta, 0, DEPTH, pt_amd.MODE_WAVEFRONT, tile=tile, min_frames=lo, step_frames=step,
                              max_frames=hi, tol=TOL, floor=FLOOR, noisy_fraction=FRACTION, counters=True)
        prof = s.profile_read()
        s.profile_enable(False)
    assert sim["accum"].mean() > 0
    assert r["passes"] == sim["passes"]
    assert prof["k_wf_accum"]["launches"] == sim["passes"], (prof["k_wf_accum"]["launches"], sim["passes"], per_rectangle)
    assert "k_regen" not in prof and "k_mega" not in prof
    assert np.array_equal(r["tile_frames"], sim["tile_frames"])
    assert same_bits(r["accum"], sim["accum"]), mismatch_report(r["accum"], sim["accum"])
    assert same_bits(r["m2"], sim["m2"]), mismatch_report(r["m2"], sim["m2"])
    assert same_noise(r["tile_noise"], sim["tile_noise"])
