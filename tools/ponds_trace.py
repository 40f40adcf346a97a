#!/usr/bin/env python3
"""A small fixed pond workload for a kernel trace: which kernels a label call launches, and how often.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ponds_trace.py [--lib FILE]                 one Ponds handle on a
                                            131 x 385 noise raster (density 0.41, 3 % NODATA), label_curves twice
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ponds_trace.py --devices 0,0 [--lib FILE]   a GroupPonds handle over
                                            two row blocks of the same raster, label_outlets twice

--lib: another build of the library (tools/build_alt.sh NAME REV) instead of the tree's.  Two builds that queue the same work show
the same kernel names and call counts.  Prints the pond count."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import wdpm_amd  # noqa: E402
from wdpm_amd.ponds import GroupPonds, Ponds  # noqa: E402

MISS, R, CC = -99999.0, 131, 385


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", metavar="FILE")
    ap.add_argument("--devices", metavar="a,b")
    a = ap.parse_args()
    hip = wdpm_amd.load(a.lib) if a.lib else wdpm_amd.load_hip()
    rng = np.random.default_rng(41)
    bd = np.full((R + 2, CC + 2), MISS)
    bw = np.zeros((R + 2, CC + 2))
    bd[1:-1, 1:-1] = np.where(rng.random((R, CC)) < 0.03, MISS, 500.0 + rng.random((R, CC)))
    bw[1:-1, 1:-1] = np.where(rng.random((R, CC)) < 0.41, 0.002 + 2.0 * rng.random((R, CC)), 0.0)
    if a.devices:
        from wdpm_amd.rowblock import Group
        with Group(hip, "add", R, CC, MISS, [int(d) for d in a.devices.split(",")]) as grp:
            grp.upload(bd, bw)
            with GroupPonds(grp) as p:
                n = [p.label_outlets(0.001) for _ in range(2)]
    else:
        with hip.context(module="add", nrows=R, ncols=CC, missingvalue=MISS) as ctx:
            ctx.upload(bd, bw)
            with Ponds(ctx) as p:
                n = [p.label_curves(0.001) for _ in range(2)]
    print("ponds:", n)


if __name__ == "__main__":
    main()
