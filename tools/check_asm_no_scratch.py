#!/usr/bin/env python3
"""Fail when a kernel of an AMDGPU assembly listing keeps anything in scratch (private) memory.

Reads the kernel descriptors hipcc writes with -S: every `.amdhsa_kernel NAME` block must say
`.amdhsa_private_segment_fixed_size 0` and must not ask for a dynamic stack.  Spills and runtime-indexed
local arrays both show up there."""
import re
import sys


def main(path):
    text = open(path).read()
    kernels = re.findall(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S)
    if not kernels:
        print(f"{path}: no kernel descriptors found", file=sys.stderr)
        return 1
    bad = []
    for name, body in kernels:
        m = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body)
        size = int(m.group(1)) if m else -1
        dyn = re.search(r"\.amdhsa_uses_dynamic_stack\s+(\d+)", body)
        if size != 0 or (dyn and int(dyn.group(1)) != 0):
            bad.append(f"{name}: private segment {size} bytes, dynamic stack {dyn.group(1) if dyn else '?'}")
    for b in bad:
        print(f"{path}: {b}", file=sys.stderr)
    print(f"{path}: {len(kernels)} kernels, {len(bad)} with scratch")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
