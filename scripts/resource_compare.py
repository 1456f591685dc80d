"""Compare the kernels' resource blocks of two trees: scripts/resource_compare.py PARENT_ASM_DIR NEW_ASM_DIR

Each directory holds pt_kernels.s, pt_wavefront.s, pt_leafpass.s, pt_query.s and pt_features.s, made from a tree's csrc/ by
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize --cuda-device-only -S X.hip -o DIR/X.s
(csrc/Makefile's flags; no GPU needed).  Per kernel instance the .amdhsa block (next free VGPR and SGPR,
accum_offset, private segment = scratch, group segment = static LDS) and the compiler's NumVgprs, NumAgprs,
ScratchSize and Occupancy are compared; kernels only the new tree has are listed."""
import re
import subprocess
import sys
KEYS = ["next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size"]
def parse(path):
    out = {}
    txt = open(path).read()
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        d = {}
        for k in KEYS:
            mm = re.search(r"\.amdhsa_" + k + r" (\S+)", m.group(2))
            d[k] = mm.group(1) if mm else "-"
        out[m.group(1)] = d
    for m in re.finditer(r"^(\S+):\s*; @\1\n.*?; NumVgprs: (\d+)\n; NumAgprs: (\d+)\n.*?; ScratchSize: (\d+)\n.*?; Occupancy: (\d+)", txt, re.S | re.M):
        if m.group(1) in out:
            out[m.group(1)].update(vgpr=m.group(2), agpr=m.group(3), scratch=m.group(4), occupancy=m.group(5))
    return out
def dem(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines()))
lines = []
same = diff = 0
newk = []
for f in ["pt_kernels", "pt_wavefront", "pt_leafpass", "pt_query", "pt_features"]:
    a, b = parse(f"{sys.argv[1]}/{f}.s"), parse(f"{sys.argv[2]}/{f}.s")
    names = dem(sorted(set(a) | set(b)))
    for k in sorted(b):
        if k in a:
            if a[k] == b[k]: same += 1
            else:
                diff += 1
                lines.append(f"CHANGED {f}.hip {names[k]}\n  parent {a[k]}\n  new    {b[k]}")
        else:
            newk.append((f, names[k], b[k]))
    for k in sorted(set(a) - set(b)):
        diff += 1
        lines.append(f"MISSING in new: {f}.hip {names[k]}")
print(f"existing kernel instances compared: {same + diff}; identical resource blocks: {same}; changed or missing: {diff}")
for l in lines: print(l)
print("\nnew kernels (vgpr, agpr, sgpr = next_free_sgpr, scratch bytes, static LDS bytes, occupancy waves/SIMD):")
for f, n, d in newk:
    print(f"  {f}.hip  {n}\n      vgpr {d.get('vgpr')}  agpr {d.get('agpr')}  sgpr {d['next_free_sgpr']}  scratch {d.get('scratch')}  lds {d['group_segment_fixed_size']}  occupancy {d.get('occupancy')}")
