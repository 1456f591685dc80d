"""Compare the kernels of two trees: scripts/resource_compare.py PARENT_ASM_DIR NEW_ASM_DIR

Each directory holds one X.s per kernel unit X.hip of a tree's csrc/ (every *.s found is read), made by
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize --cuda-device-only -S X.hip -o DIR/X.s
(csrc/Makefile's flags; no GPU needed).  Instances are keyed by kernel name, so a kernel that moved to another
unit is compared with itself.  Two comparisons per instance:
  the resource block: the .amdhsa block (next free VGPR and SGPR, accum_offset, private segment = scratch,
    group segment = static LDS) and the compiler's NumVgprs, NumAgprs, ScratchSize and Occupancy;
  the instruction text: the kernel's body between its label and its .Lfunc_end label, with comments and
    .loc / .file / .cfi / .p2align lines dropped and the local labels (.LBB, .Ltmp, .LJTI) renumbered in order
    of appearance, compared as strings.
Kernels only one tree has are listed.  Exit status 1 when anything differs or is missing."""
import glob
import os
import re
import subprocess
import sys
KEYS = ["next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size"]
LOCAL = re.compile(r"\.L(?:BB|tmp|JTI)[0-9_]+")
def body_text(body):
    lines, names = [], {}
    for l in body.split("\n"):
        l = l.split(";")[0].strip()
        if not l or re.match(r"\.(loc|file|cfi_\w+|p2align)\b", l):
            continue
        lines.append(LOCAL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), l))
    return "\n".join(lines)
def parse(path):
    out = {}
    txt = open(path).read()
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        d = {}
        for k in KEYS:
            mm = re.search(r"\.amdhsa_" + k + r" (\S+)", m.group(2))
            d[k] = mm.group(1) if mm else "-"
        out[m.group(1)] = d
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:\n.*?; NumVgprs: (\d+)\n; NumAgprs: (\d+)\n.*?; ScratchSize: (\d+)\n.*?; Occupancy: (\d+)", txt, re.S | re.M):
        if m.group(1) in out:
            out[m.group(1)].update(vgpr=m.group(3), agpr=m.group(4), scratch=m.group(5), occupancy=m.group(6), text=body_text(m.group(2)))
    return out
def parse_dir(d):
    out, unit = {}, {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        for k, v in parse(path).items():
            if k in out:
                sys.exit(f"{k} is defined in {unit[k]}.hip and in {os.path.basename(path)[:-2]}.hip")
            out[k], unit[k] = v, os.path.basename(path)[:-2]
    return out, unit
def dem(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines()))
(a, ua), (b, ub) = parse_dir(sys.argv[1]), parse_dir(sys.argv[2])
names = dem(sorted(set(a) | set(b)))
res = lambda d: {k: v for k, v in d.items() if k != "text"}
lines, moved = [], 0
same = diff = tsame = tdiff = 0
for k in sorted(set(a) & set(b)):
    moved += ua[k] != ub[k]
    if res(a[k]) == res(b[k]): same += 1
    else:
        diff += 1
        lines.append(f"CHANGED resources {ub[k]}.hip {names[k]}\n  parent {res(a[k])}\n  new    {res(b[k])}")
    if "text" in a[k] and a[k].get("text") == b[k].get("text"): tsame += 1
    else:
        tdiff += 1
        lines.append(f"CHANGED instruction text {ub[k]}.hip {names[k]}")
missing = sorted(set(a) - set(b))
for k in missing: lines.append(f"MISSING in new: {ua[k]}.hip {names[k]}")
newk = sorted(set(b) - set(a))
print(f"kernel instances: parent {len(a)}, new {len(b)}; in both {same + diff} ({moved} in another unit); missing in new {len(missing)}; only in new {len(newk)}")
print(f"identical resource blocks: {same}; changed: {diff}")
print(f"identical instruction text: {tsame}; changed: {tdiff}")
for l in lines: print(l)
if newk:
    print("\nnew kernels (vgpr, agpr, sgpr = next_free_sgpr, scratch bytes, static LDS bytes, occupancy waves/SIMD):")
for k in newk:
    d = b[k]
    print(f"  {ub[k]}.hip  {names[k]}\n      vgpr {d.get('vgpr')}  agpr {d.get('agpr')}  sgpr {d['next_free_sgpr']}  scratch {d.get('scratch')}  lds {d['group_segment_fixed_size']}  occupancy {d.get('occupancy')}")
sys.exit(1 if diff or tdiff or missing else 0)
