#!/usr/bin/env python3
"""Did putting the curve kernels under `template <bool kRows>` (the row-block form, include/wdpm_group_pond_curves.h) touch the
whole-raster instantiations?  The `bed` and `stages` phases of `wdpm_curves_label` on this tree's library against the same phases on
another build of the library (the parent commit's: tools/build_alt.sh parent REV) and on a byte-for-byte copy of that other build,
all three loaded into ONE process, each with a context of its own holding the same raster, their calls alternating - the method of
tools/curves_beside.py with its own A/A:

    python tools/curve_phases_beside.py wet|noise N --other wdpm_amd/csrc/alt_parent_libwdpm_hip.so --copy wdpm_amd/csrc/alt_parent2_libwdpm_hip.so
                                        [--rounds 7] [--out FILE]

The rasters are those of tools/ponds_bench.py.  One untimed call each, then --rounds alternating rounds; HIP events around the phases
(WDPM_PONDS_TIMING=1).  Per phase: the medians of the three, the difference tree - other beside the difference copy - other (the
A/A spread of the other build against itself), and whether the first lies within the second.  Appends one JSON object to --out
(default profiles/r24/whole_raster_beside.json) and prints it.
"""
import argparse
import json
import os
import statistics
import sys

os.environ["WDPM_PONDS_TIMING"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import wdpm_amd  # noqa: E402
from wdpm_amd import ponds  # noqa: E402

MISS = -99999.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("job", choices=["wet", "noise"])
    ap.add_argument("n", type=int)
    ap.add_argument("--other", required=True, help="the other build of libwdpm_hip.so (it need not know the group curve calls or the spills)")
    ap.add_argument("--copy", required=True, help="a copy of --other under another file name: the A/A")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "whole_raster_beside.json"))
    a = ap.parse_args()
    tree = wdpm_amd.load_hip()
    libs = {"tree": tree, "other": wdpm_amd.load(os.path.abspath(a.other)), "copy": wdpm_amd.load(os.path.abspath(a.copy))}
    # the other build is bound without the group curve symbols and the spill symbols, which it may not have
    group_symbols, ponds.GROUP_CURVE_SYMBOLS = ponds.GROUP_CURVE_SYMBOLS, {}
    spill_symbols, ponds.SPILL_SYMBOLS = ponds.SPILL_SYMBOLS, {}
    ponds.bind(libs["other"])
    ponds.bind(libs["copy"])
    ponds.GROUP_CURVE_SYMBOLS, ponds.SPILL_SYMBOLS = group_symbols, spill_symbols
    ponds.bind(tree)
    n = a.n
    dem = tree.synth_dem(n, n)
    if a.job == "wet":
        water, iters = np.full((n, n), 0.1), 1000
    else:
        rng = np.random.default_rng(41)
        water, iters = np.where(rng.random((n, n)) < 0.41, 0.002 + 2.0 * rng.random((n, n)), 0.0), 0
        dem[rng.random((n, n)) < 0.03] = MISS
    bd = np.full((n + 2, n + 2), MISS)
    bd[1:-1, 1:-1] = dem
    bw = np.zeros((n + 2, n + 2))
    bw[1:-1, 1:-1] = water
    del dem, water
    kw = dict(module="add", nrows=n, ncols=n, missingvalue=MISS)
    names = list(ponds.CURVE_PHASES)
    got = {w: {k: [] for k in names} for w in libs}
    ctxs = {w: lib.context(**kw) for w, lib in libs.items()}
    try:
        for c in ctxs.values():
            c.upload(bd, bw)
            if iters:
                c.run_block(iters, 0.005 / 1000)
        handles = {w: ponds.Ponds(c) for w, c in ctxs.items()}
        try:
            for p in handles.values():
                p.label_curves(0.001)                          # untimed: allocates
            for _ in range(a.rounds):
                for w in ("other", "tree", "copy"):
                    ctxs[w].synchronize()
                    handles[w].label_curves(0.001)
                    for k, v in handles[w].curve_phase_ms().items():
                        got[w][k].append(v)
            same = all(handles[w].curves().tobytes() == handles["other"].curves().tobytes() for w in ("tree", "copy"))
        finally:
            for p in handles.values():
                p.close()
    finally:
        for c in ctxs.values():
            c.close()
    rec = dict(job=a.job, n=n, rounds=a.rounds, tree_build=tree.dll.wdpm_build_info().decode(), other=os.path.basename(a.other),
               copy=os.path.basename(a.copy), same_tables=bool(same), phases={})
    for k in names:
        med = {w: statistics.median(v[k]) for w, v in got.items()}
        diff, aa = med["tree"] - med["other"], med["copy"] - med["other"]
        per_round = [abs(c - o) for c, o in zip(got["copy"][k], got["other"][k])]
        rec["phases"][k] = dict(median_ms=med, tree_minus_other_ms=diff, copy_minus_other_ms=aa, aa_largest_round_difference_ms=max(per_round),
                                tree_within_aa=bool(abs(diff) <= max(abs(aa), max(per_round))), all_ms={w: v[k] for w, v in got.items()})
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
