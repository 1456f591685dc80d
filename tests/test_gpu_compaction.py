"""GPU: the four compacting generate kernels (k_wf_generate_rays, _gather, _cam, _views; compact_slot, DESIGN.md
§5.15) under rejection patterns laid out against their waves, blocks and regions (compaction_cases.py), through
the region form (8 to 512 regions, with and without the permutation, two parts) and the flat form (the 16-wave
and the 4-wave scan), in one batch and in several.

Every comparison is exact: the oracle's radiance() per path on the ADMITTED SUBSET alone, scattered into the
initial accumulator, bit for bit with NaN equal to NaN; rejected rows keep their initial bits (-0, NaN and +-inf
among them); the counters are the oracle's.  Immediately before every masked call the same scene runs an
unmasked call of the same shape with other seeds, so that queue entries a wrong count replayed would carry other
values, and runs it again afterwards: counts left behind by the masked call would show there."""
import numpy as np
import pytest

import compaction_cases as kc
import gather_ref as gr
import lens_ref as lr
import pt_amd
import radiance_ref as rr
from test_gpu_parity import mismatch_report, same_bits
from test_gpu_query import open_scene
from test_gpu_radiance import check_counters, rr_of

pytestmark = pytest.mark.gpu

F = np.float32
# name -> (scene, options, samples, the fused kernel's regions: the region form of compact_slot).  At the default two
# parts take one sample each (launches of n slots); one part puts both samples into one launch of 2 n.  A batch holds
# both samples of a call that has two, so the sets that need more launches run NS_BATCHED samples: "parts4_5s" four
# parts and then one, "batched" (wf_paths = 2 n, set per n) launches of 2 n, 2 n and n slots with a memset before each
SETS = {
    "default": ("CornellBox", {}, kc.NS, True),
    "regions8": ("CornellBox", {"parts": 1, "wf_trace_blocks": 1}, kc.NS, True),
    "regions8_no_perm": ("CornellBox", {"parts": 1, "wf_trace_blocks": 1, "region_perm": 0}, kc.NS, True),
    "parts4": ("CornellBox", {"parts": 4}, kc.NS, True),
    "parts4_5s": ("CornellBox", {"parts": 4}, kc.NS_BATCHED, True),
    "flat": ("CornellBox", {"kernel": "wavefront", "fuse": 0}, kc.NS, False),
    "flat_one_part": ("CornellBox", {"kernel": "wavefront", "fuse": 0, "parts": 1}, kc.NS, False),
    "glossy": ("CornellBox-Glossy", {}, kc.NS, False),
    "batched": ("CornellBox", {"parts": 1}, kc.NS_BATCHED, True),
}
# generate launches, accumulate launches (= batches) of one call
LAUNCHES = {"default": (2, 1), "regions8": (1, 1), "regions8_no_perm": (1, 1), "parts4": (2, 1), "parts4_5s": (5, 2),
            "flat": (2, 1), "flat_one_part": (1, 1), "glossy": (2, 1), "batched": (3, 3)}
GATHER_SETS = ["default", "regions8", "parts4", "parts4_5s", "flat", "glossy"]
LENS_SETS = ["default", "regions8", "flat", "glossy"]
RAY_MATRIX = [(k, n, m) for k in SETS for n in kc.SIZES for m in kc.MASKS]
GATHER_MATRIX = [(k, n, m) for k in GATHER_SETS for n in kc.SIZES for m in kc.GATHER_MASKS]
LENS_MATRIX = [(k, name) for k in LENS_SETS for name in kc.LENS_FOCUS]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("radiance_ref"))


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return gr.build(tmp_path_factory.mktemp("gather_ref"))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def apply(ptopts, kset, n=None):
    scene, opts, ns, _ = SETS[kset]
    for k, v in opts.items():
        ptopts.set(k, v)
    if kset == "batched":
        ptopts.set("wf_paths", 2 * n)
    return scene, ns


def check_masked(scene, got, cnt, want, wcnt, keep, init, ns, what):
    """One masked call's result (cnt: None for the plain instance) against the subset reference."""
    keep = np.asarray(keep, bool)
    assert np.array_equal(bits(got)[~keep], bits(init)[~keep]), (what, "a rejected row changed")
    assert same_bits(got, want), (what, mismatch_report(got, want))
    if cnt is None:
        return
    assert cnt["samples"] == ns * int(keep.sum()), (what, cnt)
    if keep.any():
        check_counters(scene, cnt, wcnt)
    else:  # the all-rejected call: nothing counted, no word of the buffer touched
        assert not any(cnt.values()), (what, cnt)
        assert np.array_equal(bits(got), bits(init)), what


def run_masked(s, scene, call, control, masked, cwant, want, wcnt, keep, init, ns, what):
    """control (other seeds, scratch) -> masked, for the counting and the plain instance; then the control again.
    call(args, out, counters) runs one call on the scene s."""
    for counters in (True, False):
        scratch = call(control, None, False)
        got = call(masked, init, counters)
        cnt = None
        if counters:
            got, cnt = got
        assert same_bits(scratch, cwant), (what, "control before", mismatch_report(scratch, cwant))
        check_masked(scene, got, cnt, want, wcnt, keep, init, ns, (what, "counted" if counters else "plain"))
    s.check()
    after = call(control, None, False)
    s.check()
    assert same_bits(after, cwant), (what, "control after", mismatch_report(after, cwant))


@pytest.mark.parametrize("kset,n,mask", RAY_MATRIX, ids=[f"{k}-{n}-{m}" for k, n, m in RAY_MATRIX])
def test_ray_masks(packed, ptopts, ref, kset, n, mask):
    scene, ns = apply(ptopts, kset, n)
    rrp = rr_of(packed, scene)
    want, wcnt, keep, init = kc.rays_reference(ref, scene, packed, n, mask, ns)
    masked = kc.masked_rays(scene, packed, n, mask, ns)[:2]
    control = kc.control_rays(scene, packed, n)
    cwant = kc.rays_control_reference(ref, scene, packed, n, ns)
    with open_scene(packed, scene, False) as s:
        def call(args, out, counters):
            return s.query_radiance(args[0], args[1], ns, 8, rrp, out=out, counters=counters)
        run_masked(s, scene, call, control, masked, cwant, want, wcnt, keep, init, ns, (kset, n, mask))


@pytest.mark.parametrize("kset,n,mask", GATHER_MATRIX, ids=[f"{k}-{n}-{m}" for k, n, m in GATHER_MATRIX])
def test_gather_masks(packed, ptopts, gref, kset, n, mask):
    scene, ns = apply(ptopts, kset, n)
    rrp = rr_of(packed, scene)
    want, wcnt, keep, init = kc.gather_reference(gref, scene, packed, n, mask, ns=ns)
    masked = kc.masked_points(scene, packed, n, mask)[0]
    control = kc.masked_points(scene, packed, n, "none", base=kc.CONTROL_BASE)[0]
    cwant = kc.gather_control_reference(gref, scene, packed, n, ns=ns)
    with open_scene(packed, scene, False) as s:
        def call(g, out, counters):
            return s.gather(g.p, g.n, g.seeds, ns, mode="cosine", max_depth=8, rr=rrp, out=out, counters=counters)
        run_masked(s, scene, call, control, masked, cwant, want, wcnt, keep, init, ns, (kset, n, mask))


@pytest.mark.parametrize("kset", ["default", "flat"])
def test_sh9_control(packed, ptopts, gref, kset):
    """Every SH9 point is admitted, whatever its normal: the mask's zero normals reject nothing."""
    scene, ns = apply(ptopts, kset)
    n, rrp = kc.N_RAGGED, rr_of(packed, scene)
    g, keep = kc.masked_points(scene, packed, n, "alt_lanes", "sh9")
    init = kc.initial_rows(n, 27, np.ones(n, bool))
    want, adm, wcnt, _ = gr.gather(gref, packed[scene], g.packed, ns, 0, "sh9", 8, rrp, False, init)
    with open_scene(packed, scene, False) as s:
        got, cnt = s.gather(g.p, g.n, g.seeds, ns, mode="sh9", max_depth=8, rr=rrp, out=init, counters=True)
        plain = s.gather(g.p, g.n, g.seeds, ns, mode="sh9", max_depth=8, rr=rrp, out=init)
        s.check()
    assert not keep.all() and (adm == ns).all()
    for out in (got, plain):
        assert same_bits(out, want), mismatch_report(out, want)
    assert cnt["samples"] == ns * n
    check_counters(scene, cnt, wcnt)


def test_large_list_at_the_default(packed, ptopts, ref):
    """40,000 rays, one sample, every other one rejected at random: 625 batches over at most 512 regions, so a
    region's second batch lands on a count that is no multiple of 64."""
    scene = "CornellBox"
    rrp = rr_of(packed, scene)
    rays, seeds, keep = kc.big_rays(scene, packed)
    want, wcnt, _, init = kc.big_reference(ref, scene, packed)
    with open_scene(packed, scene, False) as s:
        s.query_radiance(kc.base_rays(scene, packed, kc.BIG_N), kc.seeds_of(kc.BIG_N, kc.CONTROL_BASE), 1, 8, rrp)
        got, cnt = s.query_radiance(rays, seeds, 1, 8, rrp, out=init, counters=True)
        s.query_radiance(kc.base_rays(scene, packed, kc.BIG_N), kc.seeds_of(kc.BIG_N, kc.CONTROL_BASE), 1, 8, rrp)
        plain = s.query_radiance(rays, seeds, 1, 8, rrp, out=init)
        s.check()
    check_masked(scene, got, cnt, want, wcnt, keep, init, 1, "counted")
    check_masked(scene, plain, None, want, wcnt, keep, init, 1, "plain")


@pytest.mark.parametrize("kset,name", LENS_MATRIX, ids=[f"{k}-{n}" for k, n in LENS_MATRIX])
def test_lens_renders(packed, ptopts, ref, kset, name):
    """The degenerate thin lens at three focus distances — no sample admitted, 0.032 of them, 0.942 — after a
    pinhole render of the same shape that sees light, and before one."""
    scene, _ = apply(ptopts, kset)
    want, wcnt, init, dead = kc.lens_reference(ref, scene, packed, name)
    cwant = kc.lens_control_reference(ref, scene, packed)
    adm = np.stack([f[2] for f in kc.lens_frames(name)])
    meta, cmeta = kc.lens_meta(), kc.control_meta(scene)

    with open_scene(packed, scene, False) as s:
        def control():
            s.set_camera("pinhole")
            return s.render(cmeta, kc.CONTROL_FRAME0, kc.LFRAMES, 1, lr.DEPTH, mode=pt_amd.MODE_WAVEFRONT)

        def masked(counters):
            s.set_camera(*kc.lens_cam(name))
            return s.render(meta, 0, kc.LFRAMES, 1, lr.DEPTH, accum=init.copy(), counters=counters)
        for counters in (True, False):
            before = control()
            got = masked(counters)
            cnt = None
            if counters:
                got, cnt = got
            assert same_bits(before, cwant), (counters, mismatch_report(before, cwant))
            assert np.array_equal(bits(got)[dead], bits(init)[dead]), counters
            assert same_bits(got, want), (counters, mismatch_report(got, want))
            if counters:
                assert cnt["samples"] == int(adm.sum())
                if adm.any():
                    check_counters(scene, cnt, wcnt)
                else:
                    assert not any(cnt.values()), cnt
                    assert np.array_equal(bits(got), bits(init))
        s.check()
        after = control()
        s.check()
    assert same_bits(after, cwant), mismatch_report(after, cwant)


@pytest.mark.parametrize("parts", (0, 1), ids=("default", "one_part"))
@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Glossy"])
def test_view_atlas(packed, ptopts, ref, scene, parts):
    """A pinhole 9 x 7 window, the dead lens, the sparse lens and a pinhole 5 x 3 window in one list: the views'
    borders fall inside waves.  One part: one launch of the three frames, 156 of its 196 waves and 34 of its 49
    blocks empty; the default: two parts, frames 0 and 1 in one launch and frame 2 in another."""
    if parts:
        ptopts.set("parts", parts)
    views, cviews = kc.atlas_views(scene), kc.atlas_control_views(scene)
    want, wcnt, init, inside, dead = kc.atlas_reference(ref, scene, packed)
    cwant = kc.atlas_control_reference(ref, scene, packed)
    with open_scene(packed, scene, False) as s:
        def control():
            return s.render_views(cviews, kc.LFRAMES, 1, lr.DEPTH, atlas=kc.ATLAS)
        for counters in (True, False):
            before = control()
            got = s.render_views(views, kc.LFRAMES, 1, lr.DEPTH, atlas=kc.ATLAS, accum=init.copy(), counters=counters)
            if counters:
                got, cnt = got
                check_counters(scene, cnt, wcnt)
                assert cnt["samples"] == 3 * (63 + 15) + kc.LENS_MEASURED["sparse"][0]
            assert same_bits(before, cwant), (counters, mismatch_report(before, cwant))
            assert np.array_equal(bits(got)[~inside | dead], bits(init)[~inside | dead]), counters
            assert same_bits(got, want), (counters, mismatch_report(got, want))
        s.check()
        after = control()
        s.check()
    assert same_bits(after, cwant), mismatch_report(after, cwant)


@pytest.mark.parametrize("kset", list(SETS))
def test_the_sets_take_their_form(packed, ptopts, kset):
    """What the sets are named for, from the launch records of one masked call: the fused kernel (its regions:
    compact_slot's region form) or the trace and shade kernels (the flat form), a generate launch per part, an
    accumulate launch per batch."""
    n = kc.N_RAGGED
    scene, ns = apply(ptopts, kset, n)
    rays, seeds, keep = kc.masked_rays(scene, packed, n, "bernoulli50", ns)
    with open_scene(packed, scene, False) as s:
        s.profile_enable(True)
        _, cnt = s.query_radiance(rays, seeds, ns, 8, rr_of(packed, scene), counters=True)
        prof = s.profile_read()
        s.profile_enable(False)
    assert cnt["samples"] == ns * int(keep.sum())
    region = SETS[kset][3]
    assert ("k_wf_step" in prof) == region and ("k_wf_trace" in prof) == (not region), prof.keys()
    assert (prof["k_wf_generate"]["launches"], prof["k_wf_accum"]["launches"]) == LAUNCHES[kset], prof
