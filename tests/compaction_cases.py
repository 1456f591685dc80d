"""Inputs and references of the generate kernels' compaction under rejection (compact_slot in
csrc/pt_wf_source.hip), shared by test_compaction_cpu.py and test_gpu_compaction.py.

A path's result does not depend on its queue slot, so the reference of every case is the oracle's radiance()
per path (radiance_ref.py, gather_ref.py, lens_ref.py, views_ref.py), bit for bit.  What this module adds:

  * rejection masks laid out in LAUNCH-SLOT space.  The 16-wave kernels (k_wf_generate_rays, _gather) give
    sample f of row i the slot p = f n + i, in blocks of 1024 slots; the 4-wave kernels (k_wf_generate_cam,
    _views) take pixels in order, frame after frame, in blocks of 256.  A wave is 64 slots = one batch j = p / 64
    of the region layout, whose region is a permutation of j mod R.  A row is rejected as a whole (a ray by
    d = 0 or a NaN component, alternating; a COSINE gather point by a zero normal), so a mask is a set of rows:
    n = 3072 keeps the pattern aligned in both samples, n = 2500 shifts it against the waves in the second.
  * distinct rows: the scene's `mixed` family (its admitted rays) and gather points tiled up to n, every row
    with its own seed base + index, so that a lost, duplicated or misattributed path changes bits.
  * an independent reference: the oracle on the ADMITTED SUBSET alone — a compacted list — scattered into the
    initial accumulator.  test_compaction_cpu.py pins it against the oracle on the full list.
  * census(): the waves, blocks and regions of each kind in launch-slot space, from the mask alone; the
    conditions every case is there for (NEEDS) are asserted by test_compaction_cpu.py.

The degenerate thin lens (tests/test_gpu_lens.py: radius 0 at (1000, 1000, 1000), the target rounding to the lens
point) at 64 x 32, 3 frames, by focus distance — measured with lens_ref.rays_seeds (test_compaction_cpu.py asserts
the counts):
    2e-5     0 admitted: 96 empty waves, 24 empty blocks
    2.5e-5   0.032 admitted: 66 empty and 30 mixed waves, 15 of 24 blocks empty
    4.5e-5   0.942 admitted: 55 full and 41 mixed waves
"""
import numpy as np

import cam_cases as cc
import gather_ref as gr
import lens_ref as lr
import radiance_ref as rr

F = np.float32
WAVE = 64
N_ALIGNED, N_RAGGED = 3072, 2500
SIZES = (N_ALIGNED, N_RAGGED)
NS = 2  # samples of a masked call: 6 and 5 blocks of 1024, 96 and 79 batches
NS_BATCHED = 5  # under wf_paths = 2 n: batches of 2 + 2 + 1 samples (a batch holds two samples of a call that has two)
REGIONS8 = 8  # {"parts": 1, "wf_trace_blocks": 1}: one trace block of 8 waves
SEED_BASE, CONTROL_BASE = 0x5EED0000, 0xC0117001
BIG_N = 40000  # one sample: 625 batches > kRegions = 512, so a region takes a second batch onto a ragged count

# mask -> what it is there for: census() keys that must be positive at both sizes, in a launch of NS samples and of one
NEEDS = {
    "none": ("full_waves", "full_blocks"),
    "all": ("empty_waves", "empty_blocks"),
    "first_row": ("empty_waves", "mixed_waves", "empty_blocks"),
    "last_row": ("empty_waves", "mixed_waves", "empty_blocks"),
    "alt_lanes": ("mixed_waves",),
    "alt_waves": ("empty_waves", "full_waves"),
    "block0": ("empty_blocks", "full_blocks"),
    "mid_block": ("empty_blocks", "full_blocks"),
    "wave0_of_block": ("empty_waves", "full_waves"),
    "wave15_of_block": ("empty_waves", "full_waves"),
    "bernoulli50": ("mixed_waves",),
    "bernoulli03": ("mixed_waves", "empty_waves"),
    "region3_out": ("empty_waves", "full_waves", "empty_regions8"),
    "region3_only": ("empty_waves", "full_waves", "empty_regions8"),
}
MASKS = list(NEEDS)
GATHER_MASKS = ["none", "all", "alt_lanes", "alt_waves", "mid_block", "bernoulli50"]


def keep_rows(name, n, ns=NS):
    """[n] bool: the rows the mask admits (ns: the samples of one launch, for the masks made of batches)."""
    i = np.arange(n)
    w = i // WAVE
    if name == "none":
        return np.ones(n, bool)
    if name == "all":
        return np.zeros(n, bool)
    if name == "first_row":
        return i == 0
    if name == "last_row":
        return i == n - 1
    if name == "alt_lanes":
        return i % 2 == 0
    if name == "alt_waves":
        return w % 2 == 0
    if name == "block0":
        return i >= 1024
    if name == "mid_block":
        return (i < 1024) | (i >= 2048)
    if name == "wave0_of_block":
        return w % 16 == 0
    if name == "wave15_of_block":
        return w % 16 == 15
    if name in ("bernoulli50", "bernoulli03"):
        q = 0.5 if name == "bernoulli50" else 0.03
        return np.random.default_rng([20261021, n, int(q * 100)]).random(n) < q
    if name in ("region3_out", "region3_only"):
        # a row whose slot falls into a batch j = 3 (mod 8) in any sample (n = 3072: the same rows in both)
        hit = np.zeros(n, bool)
        for f in range(ns):
            hit |= ((f * n + i) // WAVE) % REGIONS8 == 3
        return ~hit if name == "region3_out" else hit
    raise KeyError(name)


def census(slot_keep, block, regions=REGIONS8):
    """Waves, blocks and regions by kind for the admitted launch slots [P] bool of one launch (the last wave and
    block may be partial: full means every slot they have)."""
    P = len(slot_keep)
    out = {k: 0 for k in ("empty_waves", "full_waves", "mixed_waves", "empty_blocks", "full_blocks", "mixed_blocks")}
    for size, kind in ((WAVE, "waves"), (block, "blocks")):
        for a in range(0, P, size):
            k = int(slot_keep[a:a + size].sum())
            out[("empty_" if k == 0 else "full_" if k == len(slot_keep[a:a + size]) else "mixed_") + kind] += 1
    per_region = np.zeros(regions, np.int64)
    ragged = 0  # batches appended to a region whose count is no multiple of 64 (any append order)
    nbat = (P + WAVE - 1) // WAVE
    kept = [int(slot_keep[j * WAVE:(j + 1) * WAVE].sum()) for j in range(nbat)]
    for r in range(regions):
        mine = [k for k in kept[r::regions] if k]
        per_region[r] = sum(mine)
        ragged += len(mine) >= 2 and any(k % WAVE for k in mine)
    out["empty_regions%d" % regions] = int((per_region == 0).sum())
    out["ragged_regions%d" % regions] = int(ragged)
    out["admitted"] = int(slot_keep.sum())
    return out


def slots_of_rows(keep, ns):
    """The launch slots of a ray or gather call of ns samples in one batch: p = f n + i."""
    return np.tile(np.asarray(keep, bool), ns)


# ---------------------------------------------------------------------------------------------
# ray lists
# ---------------------------------------------------------------------------------------------
_BASE, _REF = {}, {}


def base_rays(scene, packed, n):
    """[n, 8]: the admitted rays of the scene's `mixed` family, tiled."""
    if (scene, n) not in _BASE:
        fam = rr.family(scene, packed, "mixed")
        good = fam.rays[rr.admitted(fam.rays)]
        assert len(good) >= 300
        _BASE[(scene, n)] = np.ascontiguousarray(good[np.arange(n) % len(good)])
    return _BASE[(scene, n)]


def seeds_of(n, base=SEED_BASE):
    return ((base + np.arange(n, dtype=np.uint64)) & 0xFFFFFFFF).astype(np.uint32)


def reject(rays, keep):
    """A copy of rays with the rows outside keep made unadmittable: d = 0 in the even rows, a NaN component in the odd."""
    rays = rays.copy()
    rej = np.flatnonzero(~keep)
    rays[rej[rej % 2 == 0], 4:7] = 0
    rays[rej[rej % 2 == 1], 5] = np.nan
    return rays


def masked_rays(scene, packed, n, mask, ns=NS):
    """(rays [n, 8] with the rejected rows made unadmittable, seeds, keep)."""
    keep = keep_rows(mask, n)  # a launch holds NS samples whatever the call's count (NS_BATCHED: 2 + 2 + 1)
    return reject(base_rays(scene, packed, n), keep), seeds_of(n), keep


def control_rays(scene, packed, n):
    """The unmasked call of the same shape with other seeds: whatever it leaves in the queues carries its values."""
    return base_rays(scene, packed, n), seeds_of(n, CONTROL_BASE)


def initial_rows(n, w, keep):
    """A non-zero accumulator [n, w]; some rejected rows hold -0, NaN and +-inf: bits an added zero would not keep."""
    init = np.random.default_rng(rr.SEED + 2).uniform(-2.0, 4.0, (n, w)).astype(F)
    rej = np.flatnonzero(~np.asarray(keep, bool))
    special = np.array([-0.0, np.nan, np.inf, -np.inf], F)
    for k, i in enumerate(rej[::7]):
        init[i] = np.roll(special, k)[np.arange(w) % 4]
    return init


def scatter(init, idx, sub):
    want = init.copy()
    want[idx] = sub
    return want


def rays_reference(lib, scene, packed, n, mask, ns=NS):
    """(want [n, 3], counters, keep, init) of the masked call onto initial_rows: the oracle on the admitted subset
    alone, scattered.  Memoised; callers leave it unchanged."""
    key = ("rays", scene, n, mask, ns)
    if key not in _REF:
        rays, seeds, keep = masked_rays(scene, packed, n, mask, ns)
        init = initial_rows(n, 3, keep)
        idx = np.flatnonzero(keep)
        sub, adm, cnt, _ = rr.radiance(lib, packed[scene], rays[idx], seeds[idx], ns, 8, float(packed[scene].meta[45]), False,
                                       init[idx])
        assert adm.all()
        _REF[key] = (scatter(init, idx, sub), cnt, keep, init)
    return _REF[key]


def rays_control_reference(lib, scene, packed, n, ns=NS):
    """want [n, 3] from zeros of the control call."""
    key = ("rays_control", scene, n, ns)
    if key not in _REF:
        rays, seeds = control_rays(scene, packed, n)
        _REF[key] = rr.radiance(lib, packed[scene], rays, seeds, ns, 8, float(packed[scene].meta[45]))[0]
    return _REF[key]


def big_rays(scene, packed):
    """BIG_N rays, Bernoulli 0.5 rejected, one sample."""
    keep = np.random.default_rng([20261021, BIG_N]).random(BIG_N) < 0.5
    return reject(base_rays(scene, packed, BIG_N), keep), seeds_of(BIG_N), keep


def big_reference(lib, scene, packed):
    key = ("big", scene)
    if key not in _REF:
        rays, seeds, keep = big_rays(scene, packed)
        init = initial_rows(BIG_N, 3, keep)
        idx = np.flatnonzero(keep)
        sub, _, cnt, _ = rr.radiance(lib, packed[scene], rays[idx], seeds[idx], 1, 8, float(packed[scene].meta[45]), False,
                                     init[idx])
        _REF[key] = (scatter(init, idx, sub), cnt, keep, init)
    return _REF[key]


# ---------------------------------------------------------------------------------------------
# gather points
# ---------------------------------------------------------------------------------------------
def masked_points(scene, packed, n, mask, mode="cosine", base=SEED_BASE, ns=NS):
    """(gather_ref.Points with a zero normal in the rejected rows, keep)."""
    g = gr.points(scene, packed, mode)
    t = np.arange(n) % gr.N
    keep = keep_rows(mask, n)  # a launch holds NS samples whatever the call's count (NS_BATCHED: 2 + 2 + 1)
    nrm = g.n[t].copy()
    nrm[~keep] = 0
    return gr.Points(g.p[t], nrm, seeds_of(n, base)), keep


def gather_reference(lib, scene, packed, n, mask, mode="cosine", ns=NS):
    """(want [n, 3 | 27], counters, keep, init): the reference on the admitted subset alone, scattered."""
    key = ("gather", scene, n, mask, mode, ns)
    if key not in _REF:
        g, keep = masked_points(scene, packed, n, mask, mode, ns=ns)
        init = initial_rows(n, gr.width(mode), keep)
        idx = np.flatnonzero(keep)
        sub, adm, cnt, _ = gr.gather(lib, packed[scene], g.packed[idx], ns, 0, mode, 8, float(packed[scene].meta[45]), False,
                                     init[idx])
        assert (adm == ns).all()
        _REF[key] = (scatter(init, idx, sub), cnt, keep, init)
    return _REF[key]


def gather_control_reference(lib, scene, packed, n, mode="cosine", ns=NS):
    key = ("gather_control", scene, n, mode, ns)
    if key not in _REF:
        g, _ = masked_points(scene, packed, n, "none", mode, CONTROL_BASE)
        _REF[key] = gr.gather(lib, packed[scene], g.packed, ns, 0, mode, 8, float(packed[scene].meta[45]))[0]
    return _REF[key]


# ---------------------------------------------------------------------------------------------
# lens renders and the view atlas
# ---------------------------------------------------------------------------------------------
LW, LH, LFRAMES = 64, 32, 3
LENS_FOCUS = {"dead": 2e-5, "sparse": 2.5e-5, "dense": 4.5e-5}
LENS_NEEDS = {"dead": ("empty_waves", "empty_blocks"), "sparse": ("empty_waves", "mixed_waves", "empty_blocks"),
              "dense": ("full_waves", "mixed_waves")}
# (admitted of 6144, empty / full / mixed waves of 96, empty blocks of 24)
LENS_MEASURED = {"dead": (0, 96, 0, 0, 24), "sparse": (196, 66, 0, 30, 15), "dense": (5789, 0, 55, 41, 0)}
_LENS = {}


def lens_meta():
    return cc.meta_from(cc.cam((1000, 1000, 1000), (0, 1, 0)), LW, LH)


def lens_cam(name):
    return ("thin_lens", 0.0, LENS_FOCUS[name])


def lens_frames(name):
    """[(rays [LH, LW, 8], seeds, admitted) per frame] of frames 0 .. 2 (memoised)."""
    if name not in _LENS:
        _LENS[name] = [lr.rays_seeds(lens_meta(), lens_cam(name), k) for k in range(LFRAMES)]
    return _LENS[name]


def lens_slots(name):
    """The launch slots of the render in one batch: pixel order, frame after frame."""
    return np.concatenate([f[2].reshape(-1) for f in lens_frames(name)])


def control_meta(scene="CornellBox"):
    """The control of a lens render or a view list: the scene's own pinhole at the lens cases' size — every
    sample has a path and the paths see light."""
    return cc.meta_of(scene, "xml", (LW, LH))


CONTROL_FRAME0 = 11


def lens_control_reference(lib, scene, packed):
    """[LH, LW, 3] from zeros: frames CONTROL_FRAME0 .. + 2 of control_meta."""
    key = ("lens_control", scene)
    if key not in _REF:
        meta = control_meta(scene)
        frames = [rr.camera_rays_seeds(meta, CONTROL_FRAME0 + k) + (np.ones((LH, LW), bool),) for k in range(LFRAMES)]
        _REF[key] = lr.accumulate(lib, packed[scene], meta, frames, lr.DEPTH, np.zeros((LH, LW, 3), F))[0]
    return _REF[key]


def image_init(h, w, dead):
    """lens_ref.initial_accum with -0, NaN and +-inf in every third pixel none of whose samples is admitted."""
    init = lr.initial_accum(h, w)
    special = np.array([-0.0, np.nan, np.inf, -np.inf], F)
    ys, xs = np.nonzero(dead)
    for k in range(0, len(ys), 3):
        init[ys[k], xs[k]] = np.roll(special, k)[:3]
    return init


def accumulate_subset(lib, packed_scene, meta, frames, depth, acc):
    """lens_ref.accumulate by the admitted samples alone: per frame, the oracle on the compacted list, scattered
    into a copy of acc [h, w, 3].  (accum, counters summed)."""
    h, w = frames[0][0].shape[:2]
    acc = np.array(acc, F, copy=True, order="C").reshape(-1, 3)
    total = {}
    for rays, seeds, adm in frames:
        idx = np.flatnonzero(adm.reshape(-1))
        if len(idx) == 0:
            continue
        sub, ok, cnt, _ = rr.radiance(lib, packed_scene, rays.reshape(-1, 8)[idx], seeds.reshape(-1)[idx], 1, depth,
                                      float(meta[45]), bool(meta[46] > 0), acc[idx])
        assert ok.all()
        acc[idx] = sub
        for key, v in cnt.items():
            total[key] = total.get(key, 0) + v
    return acc.reshape(h, w, 3), total


def lens_reference(lib, scene, packed, name):
    """(want [LH, LW, 3] onto image_init, counters, init, dead pixels)."""
    key = ("lens", scene, name)
    if key not in _REF:
        frames = lens_frames(name)
        dead = ~np.stack([f[2] for f in frames]).any(axis=0)
        init = image_init(LH, LW, dead)
        want, cnt = accumulate_subset(lib, packed[scene], lens_meta(), frames, lr.DEPTH, init)
        _REF[key] = (want, cnt, init, dead)
    return _REF[key]


# the atlas: the lens views at the left, the two pinhole windows beside them; list order pinhole, dead lens, sparse
# lens, pinhole, so that the views' borders fall at pixels 63, 2111 and 4159 of 4174 — all inside waves
ATLAS = (LW + 9, 2 * LH)
VIEWS_NPIX = 9 * 7 + 2 * LW * LH + 5 * 3
VIEW_LENSES = {1: "dead", 2: "sparse"}


def atlas_views(scene):
    pin = cc.meta_of(scene, "xml")
    lens = lens_meta()
    return [{"meta": pin, "window": (5, 4, 9, 7), "camera": None, "frame0": 1, "dst": (LW, 0)},
            {"meta": lens, "window": (0, 0, LW, LH), "camera": lens_cam("dead"), "frame0": 0, "dst": (0, 0)},
            {"meta": lens, "window": (0, 0, LW, LH), "camera": lens_cam("sparse"), "frame0": 0, "dst": (0, LH)},
            {"meta": pin, "window": (20, 13, 5, 3), "camera": None, "frame0": 2, "dst": (LW, 10)}]


def atlas_frames(scene, k):
    import views_ref as vr
    v = atlas_views(scene)[k]
    return lens_frames(VIEW_LENSES[k]) if k in VIEW_LENSES else vr.view_frames(v, LFRAMES)


def atlas_slots(scene, frames=range(LFRAMES)):
    """The launch slots of the list's `frames` in one launch: frame after frame, the views' pixels in list order
    (one part: all three frames; two parts: frames 0 and 1, and frame 2)."""
    per = [atlas_frames(scene, k) for k in range(4)]
    return np.concatenate([per[k][f][2].reshape(-1) for f in frames for k in range(4)])


def atlas_control_views(scene):
    """The same shape with every sample admitted and other seeds: the lens views as pinhole windows."""
    ctl = control_meta(scene)
    return [dict(v, meta=ctl if v["camera"] else v["meta"], camera=None, frame0=CONTROL_FRAME0 + k)
            for k, v in enumerate(atlas_views(scene))]


def atlas_reference(lib, scene, packed):
    """(want [ah, aw, 3] onto the initial atlas, counters summed, init, inside mask, dead mask)."""
    import views_ref as vr
    key = ("atlas", scene)
    if key not in _REF:
        views = atlas_views(scene)
        inside = vr.inside_mask(views, ATLAS)
        dead = np.zeros_like(inside)
        for k, v in enumerate(views):
            if k in VIEW_LENSES:
                vr.place(dead, v)[...] = ~np.stack([f[2] for f in atlas_frames(scene, k)]).any(axis=0)
        init = image_init(ATLAS[1], ATLAS[0], dead)
        want, total = init.copy(), {}
        for k, v in enumerate(views):
            onto, cnt = accumulate_subset(lib, packed[scene], v["meta"], atlas_frames(scene, k), lr.DEPTH, vr.place(want, v))
            vr.place(want, v)[...] = onto
            for key2, c in cnt.items():
                total[key2] = total.get(key2, 0) + c
        _REF[key] = (want, total, init, inside, dead)
    return _REF[key]


def atlas_control_reference(lib, scene, packed):
    """[ah, aw, 3] from zeros of atlas_control_views."""
    import views_ref as vr
    key = ("atlas_control", scene)
    if key not in _REF:
        out = np.zeros((ATLAS[1], ATLAS[0], 3), F)
        for v in atlas_control_views(scene):
            vr.place(out, v)[...] = lr.accumulate(lib, packed[scene], v["meta"], vr.view_frames(v, LFRAMES), lr.DEPTH,
                                                  vr.place(out, v))[0]
        _REF[key] = out
    return _REF[key]
