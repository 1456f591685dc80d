"""Kernels against the oracle on lights and materials the five scenes never use (tests/shade_scenes.py):
CornellBox with 1, 3, 5, 7 and 11 emissive triangles in one, two and four header ranges, a fifth
emissive object the packer does not list, an emitter as the first object and one the packer lists but
the shader does not take for one; material records patched to the combinations of Ns, illum, Kd and Ks
that pt_path.h branches on (Phong continuation with Lambert NEE, Ns = 40 without Ks, Ns one ulp either
side of 40 and of 500, Ns = 0, flat dielectric slabs, illum 7 with Ns > 500, zero and negative colours,
negative and non-finite exponents).  tests/test_gpu_parity.py's bit-exact claims rest on one light of two
triangles (inv_ntri = 0.5 exactly) and the scenes' four Ns values.  Bar: bit-exact, counters equal, NaN
equal to NaN, as there.  tests/test_shade_cpu.py checks on the oracle alone that the images are worth
comparing and the host tables against a restatement.

Per case one frame (salt 3) and a 3-frame render, counted and uncounted, at 40 x 32 and depth 8,
through the kernel sets KSETS; a direct-only frame and a frame with Russian roulette at 0.1 on
four_objects and phong_ns.
"""
import pytest

import pt_amd
import shade_scenes as ss
from test_gpu_parity import mismatch_report, same_bits
from test_gpu_step_narrow import oracle_frame, oracle_render

pytestmark = pytest.mark.gpu

# written as test_gpu_parity.py's KERNELS
KSETS = {
    "auto": {},
    "literal": {"PT_KERNEL": "literal"},
    "mega": {"PT_KERNEL": "mega"},
    "mega_global": {"PT_KERNEL": "mega", "PT_LDS": "0"},
    "wavefront": {"PT_KERNEL": "wavefront"},
    "wavefront_nofuse": {"PT_KERNEL": "wavefront", "PT_FUSE": "0"},
    "wavefront_nomailbox": {"PT_KERNEL": "wavefront", "PT_MAILBOX": "0"},
    "wavefront_global": {"PT_KERNEL": "wavefront", "PT_LDS": "0"},
}


@pytest.fixture(scope="module")
def cases(packed, tmp_path_factory):
    base = tmp_path_factory.mktemp("shade")
    return ss.all_cases({v: ss.pack_light(v, base) for v in ss.LIGHT_VARIANTS}, packed["CornellBox-Sphere"])


def check_renders(p, key):
    meta = p.meta_for(ss.W, ss.H)
    ref = oracle_frame(p, key, meta, ss.SALT, ss.DEPTH)
    racc, rc = oracle_render(p, key, meta, 3, ss.DEPTH)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        gpu = s.frame(meta, ss.SALT, ss.DEPTH)
        acc, gc = s.render(meta, 0, 3, 1, ss.DEPTH, pt_amd.MODE_AUTO, counters=True)
        plain = s.render(meta, 0, 3, 1, ss.DEPTH, pt_amd.MODE_AUTO)
    assert same_bits(gpu, ref), f"{key} frame: " + mismatch_report(gpu, ref)
    assert same_bits(acc, racc), f"{key} counted render: " + mismatch_report(acc, racc)
    assert same_bits(plain, racc), f"{key} render: " + mismatch_report(plain, racc)
    assert gc == rc, (gc, rc)


@pytest.mark.parametrize("kset", list(KSETS))
@pytest.mark.parametrize("case", ss.CASES)
def test_shade_renders_bitexact(cases, ptopts, case, kset):
    for k, v in KSETS[kset].items():
        ptopts.set(k, v)
    check_renders(cases[case], "shade-" + case)


@pytest.mark.parametrize("kset", list(KSETS))
@pytest.mark.parametrize("mode", ["direct_only", "rr0.1"])
@pytest.mark.parametrize("case", ["four_objects", "phong_ns"])
def test_shade_direct_only_and_short_paths(cases, ptopts, case, mode, kset):
    for k, v in KSETS[kset].items():
        ptopts.set(k, v)
    p = cases[case]
    meta = p.meta_for(ss.W, ss.H, direct_only=True) if mode == "direct_only" else p.meta_for(ss.W, ss.H, rr=0.1)
    key = f"shade-{case}-{mode}"
    ref = oracle_frame(p, key, meta, ss.SALT, ss.DEPTH)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        gpu = s.frame(meta, ss.SALT, ss.DEPTH)
    assert same_bits(gpu, ref), f"{key} frame: " + mismatch_report(gpu, ref)
