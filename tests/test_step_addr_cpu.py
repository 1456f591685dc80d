"""step_addr32_ok (csrc/pt_step_addr.h): the host's rule for launching the fused step kernel's 32-bit
queue addressing, checked at the 4 GiB boundary in a stand-alone program (scripts/step_addr_harness.cpp,
which includes the header alone) built with -fsanitize=address,undefined.  Needs no GPU.

The rule restated here: a part may use 32-bit byte offsets iff the extent of its widest arrays fits 32
bits — `ray` at 32 B per queue entry and `rad` at 12 B per path.
"""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

RAY, RAD = 32, 12
LIMIT = 1 << 32


def expected(qcap, paths):
    return qcap * RAY < LIMIT and paths * RAD < LIMIT


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("step_addr") / "step_addr_harness")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "scripts", "step_addr_harness.cpp"),
                    "-o", exe], check=True, capture_output=True)
    return exe


def ask(exe, pairs):
    args = [str(v) for p in pairs for v in p]
    out = subprocess.run([exe, *args], check=True, capture_output=True, text=True).stdout.split("\n")
    got = [tuple(int(x) for x in line.split()) for line in out if line]
    assert [g[:2] for g in got] == [tuple(p) for p in pairs]
    return [bool(g[2]) for g in got]


# capacities whose `ray` extent is 2^32 - 32, 2^32 and 2^32 + 32 bytes (with a small part's radiance)
RAY_CASES = [(LIMIT // RAY - 1, 2880), (LIMIT // RAY, 2880), (LIMIT // RAY + 1, 2880)]
# paths whose `rad` extent is the last multiple of 12 below 2^32, and the first two past it
RAD_CASES = [(4096, LIMIT // RAD), (4096, LIMIT // RAD + 1), (4096, LIMIT // RAD + 2)]


def test_ray_term_at_the_boundary(harness):
    assert [q * RAY for q, _ in RAY_CASES] == [LIMIT - 32, LIMIT, LIMIT + 32]
    assert ask(harness, RAY_CASES) == [True, False, False]


def test_rad_term_at_the_boundary(harness):
    assert [p * RAD for _, p in RAD_CASES] == [LIMIT - 4, LIMIT + 8, LIMIT + 20]
    assert ask(harness, RAD_CASES) == [True, False, False]


def test_terms_are_independent_and_do_not_wrap(harness):
    pairs = [(0, 0), (1, 1), (LIMIT // RAY - 1, LIMIT // RAD), (LIMIT // RAY, LIMIT // RAD), (LIMIT - 1, 1), (1, LIMIT - 1),
             (LIMIT - 1, LIMIT - 1), ((1 << 64) - 1, 1), (1, (1 << 64) - 1), ((1 << 59), 1), (1, (1 << 62))]
    assert ask(harness, pairs) == [expected(q, p) for q, p in pairs]


def test_bench_and_default_batch_shapes_take_32_bits(harness):
    # the library's default batch: 64 Mi paths in two parts, each with 64 * 4096 entries of slack
    part = (64 << 20) // 2
    assert ask(harness, [(part + 64 * 4096, part), ((64 << 20) + 64 * 4096, 64 << 20)]) == [True, True]
