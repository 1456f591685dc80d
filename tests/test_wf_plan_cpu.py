"""The plan of a wavefront call (csrc/pt_wf_plan.h): batch size, parts and frames per batch, the fused
kernel's regions, streaming regeneration and the small clamps, driven through a stand-alone program
(scripts/wf_plan_harness.cpp, which includes the header alone) built with -fsanitize=address,undefined and
run as a child process.  Needs no GPU.

The formulas restated here were written from launch_wavefront's driver and prepare_wavefront /
ensure_wavefront as they stood before the plan header took them over; the harness must agree with them
exactly, and the plans must keep the invariants the kernels rely on.
"""
import itertools
import math
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

K_REGIONS, K_SLACK, K_MAX_PARTS, K_BF_SLOTS = 512, 4096, 4, 8
TARGET = 64 << 20
RING, RING_MAX = 128, 256
EXT, GEN, ADMIT, SHADOW = 0, 1, 2, 3


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("wf_plan") / "wf_plan_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "scripts", "wf_plan_harness.cpp"),
                    "-o", exe], check=True, capture_output=True)
    return exe


def ask(exe, commands):
    """One line of output per command, as lists of tokens (integers where they are)."""
    text = "".join(" ".join(str(int(v)) if not isinstance(v, str) else v for v in c) + "\n" for c in commands)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [[int(t) if t.lstrip("-").isdigit() else t for t in line.split()] for line in out if line]
    assert len(rows) == len(commands)
    return rows


def cdiv(a, b):
    return -(-a // b)


# ---- the formulas, restated ----

def batch_size(npix, nframes, wf_paths=None):
    """prepare_wavefront's want and the floor of its halving; ensure_wavefront's queue entries."""
    target0 = max(1, TARGET if wf_paths is None else wf_paths)
    pairs = (target0 + 2 * npix - 1) // (2 * npix) * (2 * npix)
    target = target0 if (wf_paths is not None or pairs > 0x7fffffff) else pairs
    all_ = npix * nframes
    two = 2 * npix if 2 * npix <= 0x7fffffff else npix
    all_even = all_ + npix if (nframes > 1 and nframes & 1) else all_
    want = max(min(all_, two), min(all_even, target))
    return want, min(all_, npix), want + 2 * K_SLACK * 64


def deal(dual, parts, streams, nframes, capacity, npix, qcap):
    """np, F and, per batch, (fb, Fb, [(f0, frames, paths, rad_off, entry_off, capacity, qcap)])."""
    n = max(1, min(K_MAX_PARTS, parts)) if (dual and streams) else 1
    while n > 1 and (nframes < n or capacity // n < npix):
        n //= 2
    F = n * max(1, min((nframes + n - 1) // n, capacity // n // npix))
    batches = []
    for fb in range(0, nframes, F):
        Fb = min(F, nframes - fb)
        ps, f0 = [], 0
        for h in range(n):
            if f0 >= Fb:
                break
            fh = min((Fb + n - 1) // n, Fb - f0)
            ps.append((f0, fh, fh * npix, f0 * npix * 3, h * (qcap // n), capacity // n, qcap // n))
            f0 += fh
        batches.append((fb, Fb, ps))
    return n, F, batches


def parse_deal(row):
    n, F, batches, i = row[0], row[1], [], 2
    while i < len(row):
        assert row[i] == "B"
        fb, Fb, cnt = row[i + 1:i + 4]
        i += 4
        ps = []
        for _ in range(cnt):
            assert row[i] == "P"
            ps.append(tuple(row[i + 1:i + 8]))
            i += 8
        batches.append((fb, Fb, ps))
    return n, F, batches


def regions(blocks, wpb, perm, qmin=1):
    """The driver's R and (q, qi) as they were (qmin = 1); the plan starts q at 2."""
    R = min(K_REGIONS, blocks * wpb)
    q = qi = 1
    if perm and R > 2:
        q = max(qmin, int(R * 0.6180339887498949))
        while math.gcd(q, R) != 1:
            q += 1
        while q * qi % R != 1:
            qi += 1
    return R, q, qi


def regen_plan(fgen, regen, R, max_depth, paths):
    q = cam = 0
    iters = 2 * (max_depth + 1)
    if fgen and regen > 0:
        cam = max(((p + 63) // 64 + R - 1) // R for p in paths)
        q = regen
        if q < cam:
            iters = 2 * ((cam + q - 1) // q + max_depth)
        else:
            q = 0
    kinds = []
    for it in range(iters):
        if q > 0 and it % 2 == 0 and (it // 2) * q < cam:
            kinds.append(ADMIT)
        elif fgen and it == 0:
            kinds.append(GEN)
        else:
            kinds.append(EXT if it % 2 == 0 else SHADOW)
    return q, cam, iters, kinds


# ---- batch size ----

def test_batch_size_matches_the_formula(harness):
    cases = []
    for npix, nframes in itertools.product([1, 63, 64, 65, 1000, 1 << 20, 4096 * 4096, 1 << 30, (1 << 31) - 1],
                                           [1, 2, 3, 5, 16, 256]):
        cases += [(npix, nframes, None)] + [(npix, nframes, t) for t in (-5, 0, 1, npix, 3 * npix + 1, 8 << 20, 1 << 40)]
    rows = ask(harness, [("batch", n, f, TARGET if t is None else t, t is not None) for n, f, t in cases])
    for (n, f, t), row in zip(cases, rows):
        assert tuple(row) == batch_size(n, f, t), (n, f, t)
        want, floor, _ = row
        assert floor <= want and (f < 2 or 2 * n > 0x7fffffff or want >= 2 * n)  # the halving's floor; two frames


# ---- frames -> batches -> parts ----

COVER = [(nframes, npix, cap, parts, dual, streams)
         for nframes in (1, 2, 3, 5, 16, 256) for npix in (1, 63, 64, 65, 1000, 1 << 20)
         for cap in (npix, 2 * npix, 2 * npix + 1, 64 << 20) for parts in (1, 2, 3, 4, 7)
         for dual in (False, True) for streams in (False, True)]


def test_every_frame_falls_in_one_part_of_one_batch(harness):
    rows = ask(harness, [("deal", d, p, s, f, c, n, c + 2 * K_SLACK * 64) for f, n, c, p, d, s in COVER])
    for (nframes, npix, cap, parts, dual, streams), row in zip(COVER, rows):
        case = (nframes, npix, cap, parts, dual, streams)
        got = parse_deal(row)
        assert got == deal(dual, parts, streams, nframes, cap, npix, cap + 2 * K_SLACK * 64), case
        n, F, batches = got
        assert n == 1 or (dual and streams and n <= min(parts, K_MAX_PARTS))
        assert parts != 3 or n in (1, 3)  # the halving takes 3 parts to 1
        nxt = 0
        for fb, Fb, ps in batches:
            assert fb == nxt and 1 <= Fb <= F and 1 <= len(ps) <= n, case
            rad = 0
            for h, (f0, frames, paths, rad_off, entry_off, pcap, pqcap) in enumerate(ps):
                assert fb + f0 == nxt and frames >= 1, case                     # increasing, none skipped, no part empty
                assert paths == frames * npix and paths <= pcap, case           # a part's paths fit its capacity
                assert rad_off == rad == 3 * f0 * npix, case                    # radiance contiguous in frame order
                assert entry_off == h * pqcap and (h + 1) * pqcap <= cap + 2 * K_SLACK * 64, case  # inside the arrays
                rad += 3 * paths
                nxt += frames
            assert nxt == fb + Fb and rad <= 3 * cap, case
        assert nxt == nframes, case


def test_two_and_five_samples_at_the_default_target(harness):
    """What the view-list pull request met on the GPU: a two-sample call runs as one batch whose two parts
    launch one sample each, and five samples as one batch of 3 + 2."""
    for npix in (6 * 128 * 128, 512 * 512, 1 << 20):
        (want2, _, q2), (want5, _, q5) = ask(harness, [("batch", npix, 2, TARGET, 0), ("batch", npix, 5, TARGET, 0)])
        assert (want2, want5) == (2 * npix, 6 * npix)
        two, five = (parse_deal(r) for r in ask(harness, [("deal", 1, 2, 1, 2, want2, npix, q2), ("deal", 1, 2, 1, 5, want5, npix, q5)]))
        assert two[0] == 2 and [(fb, Fb, [p[1] for p in ps]) for fb, Fb, ps in two[2]] == [(0, 2, [1, 1])]
        assert five[0] == 2 and [(fb, Fb, [p[1] for p in ps]) for fb, Fb, ps in five[2]] == [(0, 5, [3, 2])]


# ---- batch size -> queue entries -> parts -> regions ----

# test_region_layout.py's capacities as calls of four frames, and a few odd ones
SHAPES = [(1024, 4), (1 << 18, 4), (518400, 4), (2 << 20, 4), (1, 1), (63, 3), (65, 2), (1000, 5), (1 << 20, 256)]


@pytest.mark.parametrize("R", [1, 2, 3, 24, 64, K_REGIONS])
def test_regions_hold_their_share_of_a_part(harness, R):
    sizes = ask(harness, [("batch", n, f, TARGET, 0) for n, f in SHAPES])
    cases = [(n, f, want, qn, parts) for (n, f), (want, _, qn) in zip(SHAPES, sizes) for parts in (1, 2, 4)]
    plans = ask(harness, [("deal", 1, parts, 1, f, want, n, qn) for n, f, want, qn, parts in cases])
    for (n, f, want, qn, parts), row in zip(cases, plans):
        assert qn == want + 2 * K_SLACK * 64
        _, _, batches = parse_deal(row)
        part_list = [p for _, _, ps in batches for p in ps]
        got = ask(harness, [("regions", R, 1, perm, p[6]) for p in part_list for perm in (0, 1)])
        for k, (_, _, paths, _, _, _, pqcap) in enumerate(part_list):
            for r, q, qi, rstride in got[2 * k:2 * k + 2]:
                assert r == R and rstride == pqcap // R // 64 * 64
                assert cdiv(cdiv(paths, 64), R) * 64 <= rstride, (n, f, parts, paths)  # its share of the 64-path batches
                assert R * rstride <= pqcap


def test_region_count_and_permutation(harness):
    """R, q and qi are the earlier driver's at every R but those where its formula gave the identity with the
    option on and R > 2 — R = 3 alone, q = max(1, floor(3 * 0.618...)) = 1 — which no grid reaches (R is
    min(512, blocks * 8), a multiple of 8); there the plan starts q at 2."""
    cmds = [("regions", R, 1, perm, 1 << 20) for R in range(1, K_REGIONS + 1) for perm in (0, 1)]
    cmds += [("regions", b, 8, 1, 1 << 20) for b in (1, 3, 63, 64, 65, 1024)]
    departs = []
    for cmd, (R, q, qi, _) in zip(cmds, ask(harness, cmds)):
        was = regions(cmd[1], cmd[2], cmd[3])
        if cmd[3] and R > 2 and was[1:] == (1, 1):  # the earlier formula breaks the invariant below
            departs.append(R)
            assert R % 8 != 0 and cmd[2] != 8, cmd  # not a grid's R
            assert (R, q, qi) == regions(cmd[1], cmd[2], cmd[3], qmin=2), cmd
        else:
            assert (R, q, qi) == was, cmd
        assert R == min(K_REGIONS, cmd[1] * cmd[2])
        assert math.gcd(q, R) == 1 and q * qi % R == 1 % R
    assert departs == [3]


def test_permutation_is_the_identity_only_when_off_or_two_regions(harness):
    """The permutation is (1, 1) exactly when region_perm is off or R <= 2, for every R of 1..512."""
    cmds = [("regions", R, 1, perm, 1 << 20) for R in range(1, K_REGIONS + 1) for perm in (0, 1)]
    for cmd, (R, q, qi, _) in zip(cmds, ask(harness, cmds)):
        assert ((q, qi) == (1, 1)) == (not cmd[3] or R <= 2), cmd


# ---- streaming regeneration ----

def test_regeneration_admits_every_camera_batch(harness):
    cases = []
    for regen, R, depth in itertools.product([0, 1, 3, 8, 64], [1, 24, K_REGIONS], [0, 5]):
        q = max(regen, 1)
        for cam in sorted({1, max(q - 1, 1), q, q + 1, 2 * q, 2 * q + 1, 5 * q + 3}):
            P = cam * R * 64 - 17  # the fullest region holds `cam` camera batches
            cases += [(1, regen, R, depth, (P,)), (1, regen, R, depth, (P, max(P // 3, 1))), (0, regen, R, depth, (P, P))]
    rows = ask(harness, [("regen", fgen, regen, R, depth, *paths) for fgen, regen, R, depth, paths in cases])
    for (fgen, regen, R, depth, paths), row in zip(cases, rows):
        case = (fgen, regen, R, depth, paths)
        q, cam, iters, kinds = row[0], row[1], row[2], row[3:]
        assert (q, cam, iters, kinds) == regen_plan(fgen, regen, R, depth, paths), case
        assert [k == SHADOW for k in kinds] == [it % 2 == 1 for it in range(iters)], case
        if not fgen or regen == 0:
            assert (q, cam, iters) == (0, 0, 2 * (depth + 1)) and kinds[0] == (GEN if fgen else EXT), case
            continue
        assert cam == max(cdiv(cdiv(p, 64), R) for p in paths), case
        if regen >= cam:  # one launch admits them all: the plain first launch
            assert q == 0 and iters == 2 * (depth + 1) and kinds[0] == GEN and ADMIT not in kinds, case
            continue
        admits = [it for it, k in enumerate(kinds) if k == ADMIT]
        J = cdiv(cam, q)
        assert q == regen and admits == [2 * j for j in range(J)] and GEN not in kinds, case
        assert sum(min(q, cam - (it // 2) * q) for it in admits) == cam, case  # every batch, once
        assert (iters - admits[-1]) // 2 == depth + 1, case  # the last admission's paths run their depths


# ---- clamps ----

def test_clamps_and_ring(harness):
    vals = [-(1 << 31), -1, 0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 31) - 1]
    for v, (bins, sparse, slots) in zip(vals, ask(harness, [("clamps", v, v, v) for v in vals])):
        assert bins == (0 if v <= 0 else 8 if v < 64 else 64 if v < 512 else 512)
        assert sparse == max(0, min(v, 1 << 20)) and slots == min(K_BF_SLOTS, v)
    cases = list(itertools.product([-1, 0, 64, RING, RING_MAX, 512], [65535, 65536, 65537], [65536], [1, 2, 3], [2]))
    for (opt, l2, mx, ob, os_), (by_occ, ring) in zip(cases, ask(harness, [("ring", *c) for c in cases])):
        fits = l2 <= mx and (opt == RING_MAX or (opt <= 0 and ob >= os_))
        assert ring == (RING_MAX if fits else RING), (opt, l2, mx, ob, os_)
        assert by_occ == int(l2 <= mx and opt <= 0)  # only then are the occupancy numbers read
