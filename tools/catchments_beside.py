#!/usr/bin/env python3
"""Does the catchment pass slow what it sits beside?  The label, table and rim phases of `wdpm_catch_label` on this tree's library
against the same phases of `wdpm_rims_label` on another build of the library (the parent commit's: tools/build_alt.sh parent REV),
both loaded into ONE process, each with a context of its own holding the same raster, their calls alternating:

    python tools/catchments_beside.py wet|noise N --other wdpm_amd/csrc/alt_parent_libwdpm_hip.so [--pairs 7] [--out FILE]

The rasters are those of tools/ponds_bench.py.  One untimed call each, then --pairs alternating pairs; HIP events around the phases
(WDPM_PONDS_TIMING=1).  Per phase: median (min ... max) of either library, and whether this tree's median lies inside the other
library's own spread.  Appends one JSON object to --out (default profiles/r14/beside.json) and prints it.
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
    ap.add_argument("--other", required=True, help="the other build of libwdpm_hip.so (it need not know the catchment calls)")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "beside.json"))
    a = ap.parse_args()
    tree = wdpm_amd.load_hip()
    other = wdpm_amd.load(os.path.abspath(a.other))
    # the other build is bound without the catchment symbols, which it may not have
    catch_symbols, ponds.CATCH_SYMBOLS = ponds.CATCH_SYMBOLS, {}
    ponds.bind(other)
    ponds.CATCH_SYMBOLS = catch_symbols
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
    names = list(ponds.PHASES) + list(ponds.RIM_PHASES)
    got = {"tree": {k: [] for k in names}, "other": {k: [] for k in names}}
    with tree.context(**kw) as ct, other.context(**kw) as co:
        for c in (ct, co):
            c.upload(bd, bw)
            if iters:
                c.run_block(iters, 0.005 / 1000)
        with ponds.Ponds(ct) as pt, ponds.Ponds(co) as po:
            calls = (("other", co, po, po.label_rims), ("tree", ct, pt, pt.label_catchments))
            for _, _, _, call in calls:
                call(0.001)                                    # untimed: allocates
            for _ in range(a.pairs):
                for which, c, p, call in calls:
                    c.synchronize()
                    call(0.001)
                    for k, v in list(p.phase_ms().items()) + list(p.rims_phase_ms().items()):
                        got[which][k].append(v)
            same = pt.rims().tobytes() == po.rims().tobytes() and pt.table().tobytes() == po.table().tobytes()
            stats = pt.catchment_stats()
    rec = dict(job=a.job, n=n, pairs=a.pairs, tree_build=tree.dll.wdpm_build_info().decode(), other=os.path.basename(a.other),
               same_tables=bool(same), catchment_stats=stats, phases={})
    for k in names:
        t, o = got["tree"][k], got["other"][k]
        rec["phases"][k] = dict(tree_median=statistics.median(t), tree_min=min(t), tree_max=max(t), other_median=statistics.median(o),
                                other_min=min(o), other_max=max(o), tree_median_inside_other_spread=bool(min(o) <= statistics.median(t) <= max(o)),
                                tree=t, other=o)
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
