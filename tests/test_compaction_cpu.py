"""No GPU: the inputs of test_gpu_compaction.py (compaction_cases.py), pinned on the oracle alone — every mask
reaches in launch-slot space what it is there for (empty, full and mixed waves, empty blocks, a region that
receives nothing, a second batch on a ragged region count), the degenerate lenses' measured shares, and the
reference computed from the admitted subset alone equals the oracle's on the full list, bit for bit."""
import numpy as np
import pytest

import compaction_cases as kc
import gather_ref as gr
import lens_ref as lr
import radiance_ref as rr
import views_ref as vr
from test_gpu_parity import mismatch_report, same_bits

F = np.float32
SCENE = "CornellBox"
CASES = [(n, m) for n in kc.SIZES for m in kc.MASKS]
GATHER_CASES = [(n, m) for n in kc.SIZES for m in kc.GATHER_MASKS]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("radiance_ref"))


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return gr.build(tmp_path_factory.mktemp("gather_ref"))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("n,mask", CASES, ids=[f"{n}-{m}" for n, m in CASES])
def test_masks_reach_what_they_are_for(n, mask):
    keep = kc.keep_rows(mask, n)
    c = kc.census(kc.slots_of_rows(keep, kc.NS), 1024)
    for need in kc.NEEDS[mask]:
        assert c[need] > 0, (need, c)
    assert c["admitted"] == kc.NS * int(keep.sum())
    nblocks = -(-kc.NS * n // 1024)
    assert (nblocks, -(-kc.NS * n // 64)) == {3072: (6, 96), 2500: (5, 79)}[n]
    if mask == "none":
        assert keep.all()
    if mask == "all":
        assert not keep.any() and c["empty_blocks"] == nblocks and c["empty_regions8"] == 8
    if mask in ("first_row", "last_row"):
        assert keep.sum() == 1 and keep[0 if mask == "first_row" else -1]
    if mask == "region3_only" and n == kc.N_ALIGNED:
        assert c["empty_regions8"] == 7
    if mask == "region3_out":
        slots = kc.slots_of_rows(keep, kc.NS)
        assert all(not slots[j * 64:(j + 1) * 64].any() for j in range(3, -(-len(slots) // 64), 8))
    if mask in ("wave0_of_block", "wave15_of_block") and n == kc.N_ALIGNED:  # the scan's two ends, in every block
        slots = kc.slots_of_rows(keep, kc.NS).reshape(-1, 16, 64)
        w = 0 if mask == "wave0_of_block" else 15
        assert slots[:, w].all() and slots.sum() == 6 * 64
    # one sample alone (a part of a two-part call, the last batch of 2 + 2 + 1) starts at slot 0 like the first
    one = kc.census(keep, 1024)
    assert all(one[need] > 0 for need in kc.NEEDS[mask]), one


def test_the_ragged_size_shifts_the_pattern():
    """n = 2500 is no multiple of 64: the second sample's rows sit 4 lanes further on, so the masks made of whole
    waves have mixed waves there, which n = 3072 never has."""
    assert kc.N_RAGGED % 64 == 4 and kc.N_ALIGNED % 1024 == 0
    for mask in ("alt_waves", "block0", "wave0_of_block", "wave15_of_block"):
        assert kc.census(kc.slots_of_rows(kc.keep_rows(mask, kc.N_ALIGNED), 2), 1024)["mixed_waves"] == 0
        assert kc.census(kc.slots_of_rows(kc.keep_rows(mask, kc.N_RAGGED), 2), 1024)["mixed_waves"] > 0


@pytest.mark.parametrize("n,mask", CASES, ids=[f"{n}-{m}" for n, m in CASES])
def test_ray_subset_reference_is_the_full_lists(packed, ref, n, mask):
    """The oracle on the compacted list, scattered = the oracle on the full list with the rejected rows in it;
    admitted = the mask; the rejected rows keep the initial bits; other seeds give other bits."""
    rays, seeds, keep = kc.masked_rays(SCENE, packed, n, mask)
    want, cnt, wkeep, init = kc.rays_reference(ref, SCENE, packed, n, mask)
    full, adm, fcnt, _ = rr.radiance(ref, packed[SCENE], rays, seeds, kc.NS, 8, float(packed[SCENE].meta[45]), False, init)
    assert np.array_equal(adm, keep) and np.array_equal(rr.admitted(rays), keep) and np.array_equal(wkeep, keep)
    assert same_bits(want, full), mismatch_report(want, full)
    assert cnt == fcnt and cnt["samples"] == kc.NS * int(keep.sum())
    assert np.array_equal(bits(want[~keep]), bits(init[~keep]))
    if (~keep).sum() >= 28:
        rej = init[~keep]
        assert np.isnan(rej).any() and np.isinf(rej).any() and (np.signbit(rej) & (rej == 0)).any()
    if keep.sum() >= 100:
        lit = (want[keep] != init[keep]).any(axis=1)
        assert lit.mean() >= 0.25, lit.mean()
        control = kc.rays_control_reference(ref, SCENE, packed, n)
        clean = rr.radiance(ref, packed[SCENE], rays[keep], seeds[keep], kc.NS, 8, float(packed[SCENE].meta[45]))[0]
        differs = (bits(control[keep]) != bits(clean)).any(axis=1)
        assert differs[lit].mean() >= 0.9, differs[lit].mean()  # a replayed control entry would show


def test_rows_are_distinct(packed, ref):
    """Tiled rays under seeds base + index: the lit rows' results are pairwise distinct, so a path credited to
    another row changes bits."""
    want = kc.rays_control_reference(ref, SCENE, packed, kc.N_ALIGNED)
    lit = want[(want != 0).any(axis=1)]
    assert len(lit) >= 0.25 * kc.N_ALIGNED
    assert len(np.unique(bits(lit), axis=0)) >= 0.98 * len(lit)


def test_batched_samples(packed, ref):
    """NS_BATCHED samples (batches of 2 + 2 + 1 under wf_paths = 2 n): subset = full, as above."""
    n, mask = kc.N_RAGGED, "bernoulli50"
    rays, seeds, keep = kc.masked_rays(SCENE, packed, n, mask, kc.NS_BATCHED)
    want, cnt, _, init = kc.rays_reference(ref, SCENE, packed, n, mask, kc.NS_BATCHED)
    full, adm, fcnt, _ = rr.radiance(ref, packed[SCENE], rays, seeds, kc.NS_BATCHED, 8, float(packed[SCENE].meta[45]), False,
                                     init)
    assert np.array_equal(adm, keep) and same_bits(want, full) and cnt == fcnt
    assert np.array_equal(keep, kc.keep_rows(mask, n))


def test_the_large_case_appends_to_ragged_region_counts(packed, ref):
    """40,000 rays, one sample, Bernoulli 0.5: 625 batches over at most 512 regions — at every R <= 512 some
    region takes a second batch onto a count that is no multiple of 64."""
    rays, seeds, keep = kc.big_rays(SCENE, packed)
    assert -(-kc.BIG_N // 64) == 625 > 512
    for R in (512, 384, 256, 8):
        assert kc.census(keep, 1024, R)["ragged_regions%d" % R] > 0, R
    want, cnt, _, init = kc.big_reference(ref, SCENE, packed)
    full, adm, fcnt, _ = rr.radiance(ref, packed[SCENE], rays, seeds, 1, 8, float(packed[SCENE].meta[45]), False, init)
    assert np.array_equal(adm, keep) and same_bits(want, full) and cnt == fcnt


@pytest.mark.parametrize("n,mask", GATHER_CASES, ids=[f"{n}-{m}" for n, m in GATHER_CASES])
def test_gather_subset_reference_is_the_full_lists(packed, gref, n, mask):
    g, keep = kc.masked_points(SCENE, packed, n, mask)
    want, cnt, _, init = kc.gather_reference(gref, SCENE, packed, n, mask)
    full, adm, fcnt, _ = gr.gather(gref, packed[SCENE], g.packed, kc.NS, 0, "cosine", 8, float(packed[SCENE].meta[45]), False,
                                   init)
    assert np.array_equal(adm == kc.NS, keep) and np.array_equal(adm == 0, ~keep)
    assert same_bits(want, full), mismatch_report(want, full)
    assert cnt == fcnt and cnt["samples"] == kc.NS * int(keep.sum())
    assert np.array_equal(bits(want[~keep]), bits(init[~keep]))
    if keep.sum() >= 100:
        assert (want[keep] != init[keep]).any(axis=1).mean() >= 0.25


def test_sh9_admits_every_point(packed, gref):
    """SH9 ignores the normals: the zero normals of any mask reject nothing, so its control is its one case."""
    g, keep = kc.masked_points(SCENE, packed, kc.N_RAGGED, "alt_lanes", "sh9")
    _, adm, cnt, _ = gr.gather(gref, packed[SCENE], g.packed, kc.NS, 0, "sh9", 8, float(packed[SCENE].meta[45]))
    assert not keep.all() and (adm == kc.NS).all() and cnt["samples"] == kc.NS * kc.N_RAGGED


@pytest.mark.parametrize("name", list(kc.LENS_FOCUS))
def test_lens_shares(packed, ref, name):
    """The measured shares of the module's docstring, the conditions each lens is there for, and the subset
    reference against lens_ref.accumulate."""
    slots = kc.lens_slots(name)
    c = kc.census(slots, 256)
    assert len(slots) == 6144 == 24 * 256
    assert (c["admitted"], c["empty_waves"], c["full_waves"], c["mixed_waves"], c["empty_blocks"]) == kc.LENS_MEASURED[name], c
    for need in kc.LENS_NEEDS[name]:
        assert c[need] > 0, (need, c)
    assert round(c["admitted"] / 6144, 3) == {"dead": 0.0, "sparse": 0.032, "dense": 0.942}[name]
    for rays, _, adm in kc.lens_frames(name):
        assert np.isnan(rays[~adm][:, 4:7]).all()
    want, cnt, init, dead = kc.lens_reference(ref, SCENE, packed, name)
    full, fcnt = lr.accumulate(ref, packed[SCENE], kc.lens_meta(), kc.lens_frames(name), lr.DEPTH, init)
    assert same_bits(want, full), mismatch_report(want, full)
    assert cnt.get("samples", 0) == fcnt["samples"] == c["admitted"]
    assert np.array_equal(bits(want)[dead], bits(init)[dead])
    if name != "dense":
        assert np.isnan(init[dead]).any() and np.isinf(init[dead]).any()


def test_the_controls_see_light(packed, ref):
    """The pinhole the lens cases and the atlas run before every masked call: its paths see light, so a queue
    entry left over from it would change bits where the far lens's own paths mostly see none."""
    meta = kc.control_meta(SCENE)
    frames = [rr.camera_rays_seeds(meta, kc.CONTROL_FRAME0 + k) + (np.ones((kc.LH, kc.LW), bool),) for k in range(kc.LFRAMES)]
    acc, _ = lr.accumulate(ref, packed[SCENE], meta, frames, lr.DEPTH, np.zeros((kc.LH, kc.LW, 3), F))
    assert (acc.sum(axis=2) > 0).mean() >= 0.25


@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Glossy"])
def test_atlas(packed, ref, scene):
    """The four views' borders fall inside waves; the list has empty and mixed waves and empty blocks; the
    pinhole windows see light; subset reference = lens_ref.accumulate per view."""
    views = kc.atlas_views(scene)
    sizes = [v["window"][2] * v["window"][3] for v in views]
    assert sum(sizes) == kc.VIEWS_NPIX == 4174
    assert [b % 64 for b in np.cumsum(sizes)[:-1]] == [63, 63, 63]
    slots = kc.atlas_slots(scene)
    c = kc.census(slots, 256)
    assert len(slots) == kc.LFRAMES * kc.VIEWS_NPIX
    assert c["empty_waves"] > 0 and c["mixed_waves"] > 0 and c["empty_blocks"] > 0, c
    assert (c["empty_waves"], c["full_waves"] + c["mixed_waves"], c["empty_blocks"], c["mixed_blocks"]) == (156, 40, 34, 15), c
    assert c["admitted"] == 3 * (63 + 15) + kc.LENS_MEASURED["sparse"][0]
    for part in ((0, 1), (2,)):  # the default's two parts: each launch starts at slot 0
        cp = kc.census(kc.atlas_slots(scene, part), 256)
        assert cp["empty_waves"] > 0 and cp["mixed_waves"] > 0 and cp["empty_blocks"] > 0, (part, cp)
    inside = vr.inside_mask(views, kc.ATLAS)
    assert inside.sum() == kc.VIEWS_NPIX  # no overlap
    want, cnt, init, inside2, dead = kc.atlas_reference(ref, scene, packed)
    full = init.copy()
    for k, v in enumerate(views):
        vr.place(full, v)[...] = lr.accumulate(ref, packed[scene], v["meta"], kc.atlas_frames(scene, k), lr.DEPTH,
                                               vr.place(full, v))[0]
    assert same_bits(want, full), mismatch_report(want, full)
    assert cnt["samples"] == c["admitted"]
    assert np.array_equal(bits(want)[~inside | dead], bits(init)[~inside | dead])
    for k in (0, 3):
        tile, start = vr.place(want, views[k]), vr.place(init, views[k])
        assert (tile != start).any(axis=2).mean() >= 0.25, k
