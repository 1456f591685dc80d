#!/usr/bin/env python3
"""Static table of the fused step kernel's instances in a hipcc -S listing of pt_wf_bf.hip (with
-Rpass-analysis=kernel-resource-usage remarks in a second file): per k_wf_step_bf instance the VALU
count, lane moves (v_readlane / v_writelane), 64-bit address VALU, 32-bit literal moves, division
pieces, registers, scratch and occupancy; then, for the instances named by --loop (default: the two
the bench runs), the same counts inside the batch loop alone.

The batch loop is the last loop of the kernel that the listing marks "Loop Header: Depth=1" (the loop
over the region's batches; the one before it stages the scene): every block whose comment names that
header ("in Loop: Header=BBn" or "Parent Loop BBn"), from the first such block to the end of the last.

usage: step_isa_table.py file.s remarks.txt [--loop true,true,true,false,4 ...]
"""
import collections
import re
import sys

args = sys.argv[1:]
loops = []
while "--loop" in args:
    i = args.index("--loop")
    loops.append("<%s>" % args[i + 1])
    del args[i:i + 2]
loops = loops or ["<true,true,true,false,4>", "<false,true,true,false,4>"]
s = open(args[0]).read()
rem = open(args[1]).read() if len(args) > 1 else ""
ADDR64 = ("v_lshl_add_u64", "v_lshlrev_b64", "v_add_co_u32", "v_addc_co_u32")
OP = re.compile(r"^\s+([vsd]s?_\w+|global_\w+|buffer_\w+|flat_\w+|scratch_\w+)")


def batch_loop(body):
    lines = body.split("\n")
    hdr = [re.match(r"\.LBB(\d+_\d+):", l).group(1) for l in lines if re.match(r"\.LBB\d+_\d+:.*This Loop Header: Depth=1", l)]
    if not hdr:
        return []
    h = hdr[-1]
    mine = [i for i, l in enumerate(lines)
            if f"Header=BB{h} " in l or f"Parent Loop BB{h} " in l or l.startswith(f".LBB{h}:")]
    end = mine[-1] + 1
    while end < len(lines) and not lines[end].startswith(".LBB"):
        end += 1
    return lines[mine[0]:end]


res = {}
for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size", rem, re.S):
    res[m.group(1)] = dict(re.findall(r"remark:\s+([^:\n]+): (\S+)", m.group(2)))
print("instance                          VALU  rdlane wrlane addr64 litmov div_scale  VGPRs SGPRs scratch occupancy")
inloop = []
for m in re.finditer(r"^(_ZN2pt12k_wf_step_bf\S*):", s, re.M):
    a = m.end()
    body = s[a:s.index(".Lfunc_end", a)]
    ops = collections.Counter(x.group(1) for x in map(OP.match, body.split("\n")) if x)
    valu = sum(v for k, v in ops.items() if k.startswith("v_"))
    lit = len(re.findall(r"^\s+v_mov_b32(?:_e32)? v\d+, 0x[0-9a-f]+", body, re.M))
    g = re.search(r"k_wf_step_bfILb(\d)ELb(\d)ELb(\d)ELb(\d)ELi(\d+)E", m.group(1)).groups()
    name = "<%s,%s>" % (",".join("true" if x == "1" else "false" for x in g[:4]), g[4])
    r = res.get(m.group(1), {})
    print(f"{name:32s} {valu:5d} {ops['v_readlane_b32']:6d} {ops['v_writelane_b32']:6d} "
          f"{sum(ops[k] for k in ADDR64):6d} {lit:6d} "
          f"{ops['v_div_scale_f32']:9d}  {r.get('VGPRs', '?'):>5} {r.get('TotalSGPRs', '?'):>5} "
          f"{r.get('ScratchSize [bytes/lane]', '?'):>7} {r.get('Occupancy [waves/SIMD]', '?'):>9}")
    if name in loops:
        lo = collections.Counter(x.group(1) for x in map(OP.match, batch_loop(body)) if x)
        inloop.append(f"{name:32s} in the batch loop: VALU {sum(v for k, v in lo.items() if k.startswith('v_')):4d}  "
                      f"v_readlane {lo['v_readlane_b32']:2d}  v_writelane {lo['v_writelane_b32']:2d}  "
                      f"addr64 {sum(lo[k] for k in ADDR64):2d}  s_load {sum(v for k, v in lo.items() if k.startswith('s_load')):2d}  "
                      f"scratch ops {sum(v for k, v in lo.items() if k.startswith('scratch_'))}")
print()
print("\n".join(inloop))
