#!/usr/bin/env python3
"""Instruction statistics of the loops of one kernel in a gfx950 .s file: VGPRs, scratch, and per inner loop the
instruction count, VALU count and the commonest mnemonics.   usage: isa_loop_stats.py <file.s> <substring of the kernel symbol>
A loop that holds other loops (the two-iteration marching loops hold their polls) is counted from the compiler's block annotations:
every block marked "in Loop: Header=<label> Depth=1", the child loops' blocks left out."""
import collections
import re
import sys

lines = open(sys.argv[1]).read().splitlines()
want = sys.argv[2]
starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and want in l]
for start in starts:
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    print(lines[start][:150])
    for l in lines[end:end + 60]:
        if re.search(r"; (NumVgprs|ScratchSize|Occupancy|NumSgprs):", l):
            print("  ", l.strip())
    body = lines[start:end]
    for i, l in enumerate(body):
        if "Loop Header" not in l:
            continue
        lab = l.split(":")[0]
        back = [k for k in range(i, len(body)) if re.search(r"s_c?branch\w* " + re.escape(lab) + r"$", body[k].strip())]
        if not back:
            continue
        seg = [x.strip() for x in body[i + 1:back[-1] + 1] if x.strip() and not x.strip().startswith(";")]
        c = collections.Counter(x.split()[0] for x in seg)
        valu = sum(v for k, v in c.items() if k.startswith("v_"))
        print(f"  loop {lab}: {len(seg)} instructions, {valu} VALU")
        if len(seg) > 300:
            print("    " + ", ".join(f"{k} {v}" for k, v in c.most_common(24)))
    # outer loops: blocks are not laid out between the header and one back edge, so go by the annotations
    for i, l in enumerate(body):
        if "=>This Loop Header: Depth=1" not in l:
            continue
        lab = l.split(":")[0]
        mark = "Header=" + lab.lstrip(".L") + " Depth=1"
        seg, keep = [], False
        for k, x in enumerate(body):
            t = x.strip()
            if re.match(r"^(\.LBB\w+:|; %bb\.\d+:)", t):
                keep = (k == i) or mark in t
                continue
            if keep and t and not t.startswith(";") and not t.startswith("."):
                seg.append(t)
        c = collections.Counter(x.split()[0] for x in seg)
        valu = sum(v for k, v in c.items() if k.startswith("v_"))
        print(f"  outer loop {lab}: {len(seg)} instructions, {valu} VALU, without its child loops")
        print("    " + ", ".join(f"{k} {v}" for k, v in c.most_common(24)))
