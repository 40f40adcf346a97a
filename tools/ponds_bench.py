#!/usr/bin/env python3
"""Time the pond inventory (wdpm_amd/ponds.py) on one GPU, one job per process invocation:

    python tools/ponds_bench.py wet N [--out FILE]     the bench workload: synthetic DEM, add 100 mm, 1000 iterations -
                                                       still entirely wet, ONE pond (every cell wants the same table row)
    python tools/ponds_bench.py ponds N [--out FILE]   the mostly dry raster of tests/test_settled_golden.py: 12 m on one
                                                       256 x 256 block in eight, 100 iterations - many ponds

    python tools/ponds_bench.py noise N [--out FILE]   no iterations: water on 41 % of the cells, independently (the 8-connected
                                                       percolation region: one giant pond among very many small ones), 3 % NODATA

    ... --rims        the rims of the ponds as well (include/wdpm_pond_rims.h): five more timed calls of label_rims, the two rim
                      phases beside the table phase of the SAME calls, and their ratio (default --out profiles/r12/pond_rims.json)
                      With --devices: GroupPonds.label_rims (include/wdpm_group_pond_rims.h) - per-rank rim phases, their sum over
                      the ranks, the host's merge_ms beside stitch_ms, foreign (default --out profiles/r13/pond_rims_group.json)
    ... --catchments  the catchments of the ponds as well (include/wdpm_pond_catchments.h): five timed pairs of label_rims and
                      label_catchments, interleaved - the three catchment phases beside the table phase of the SAME calls, their
                      ratios and rounds, and the label, table and rim phases of either call side by side (default --out
                      profiles/r14/pond_catchments.json)
                      With --devices: GroupPonds.label_catchments (include/wdpm_group_pond_catchments.h) - per-rank receiver, jump
                      and tally phases and their sums over the ranks, the host's resolve_ms, exits, crossings and remote, beside the
                      table phase; then the whole-raster call on the same water in the same process, the yardstick of those sums
                      (default --out profiles/r16/pond_catchments_group.json)
    ... --outlets     the outlets of the ponds as well (include/wdpm_pond_outlets.h): five more timed calls of label_outlets, the two
                      outlet phases beside the table phase of the SAME calls, their ratios, and their rates under the byte model
                      of 20 B per cell and pass (basin, dem, w) and of 4 B per cell (a row that holds no pass reads its basins
                      alone) against the yardstick (default --out profiles/r15/pond_outlets.json)
                      With --devices: GroupPonds.label_outlets (include/wdpm_group_pond_outlets.h) - per-rank passes and locate
                      phases and their sums over the ranks, the host's merge_ms, seam_outlets and split_ponds; then the whole-raster
                      call on the same water in the same process, the yardstick of those sums (default --out
                      profiles/r17/pond_outlets_group.json)
    ... --curves      the stage curves of the ponds as well (include/wdpm_pond_curves.h): five more timed calls of label_curves, the
                      bed and stages phases beside the table, passes and locate phases of the SAME calls, their ratios, and their
                      rates under the byte model of 12 B per cell and pass (int32 basin, fp64 dem) against the yardstick (default
                      --out profiles/r18/pond_curves.json)
                      With --devices: GroupPonds.label_stage_curves (include/wdpm_group_pond_curves.h) - per-rank bed and stages
                      phases and their sums over the ranks, the host's merge_ms, split_basins and remote_beds, the bytes of slot
                      rows that come down; then the whole-raster call on the same water in the same process, phases and wall
                      clock, the yardstick of those sums (default --out profiles/r24/pond_curves_group.json)
    ... --spills      the spills of the ponds as well (include/wdpm_pond_spills.h): five more timed calls of label_spills, the rings,
                      chains and sums phases beside the table, passes, locate, bed and stages phases of the SAME calls, their
                      ratios to the table phase, the counts, and the bytes of the unit's working arrays (whole rasters only;
                      default --out profiles/r26/pond_spills.json)
    ... --routing     a runoff depth sent down the spill graph as well (include/wdpm_pond_routing.h): per depth of --runoff-mm one
                      untimed label_routing and five timed ones - the order, sweep and finish phases beside the table phase and the
                      rings, chains and sums phases of the SAME calls - then five timed route() calls, wall clock and phases: what
                      another depth costs once the ponds are ordered (whole rasters only; default --out profiles/r28/pond_routing.json)
    ... --iterations K   instead of the job's own number of iterations before the inventory
    ... --lib FILE       another build of the library (tools/build_alt.sh NAME REV) instead of the tree's: the same job on the parent

Per job: one untimed label call, then five timed ones (wall clock around the call, which ends with the stream idle; HIP events
around every kernel with WDPM_PONDS_TIMING=1), medians; one steady iteration launch of the same context as the unit; the bytes
each phase has to move, against what tools/hbm_yardstick.hip streams on the same box (--yardstick FILE, the output of
tools/_build/hbm_yardstick); scipy.ndimage.label on the downloaded raster where scipy is there.  Appends one JSON object per job to
--out (default profiles/r10/ponds.json; with --devices profiles/r11/ponds_group.json) and prints it.  Run each job under a time limit of its own.

    python tools/ponds_bench.py wet N --devices 0,0 [--out FILE]    the same jobs over row blocks (wdpm_amd.ponds.GroupPonds), one
                                                                    per device named (a device may repeat): per-rank phase times,
                                                                    the host's stitch_ms and the wall clock of the whole call
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

os.environ["WDPM_PONDS_TIMING"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import wdpm_amd  # noqa: E402
from wdpm_amd.ponds import (CATCH_PHASES, CURVE_PHASES, OUTLET_PHASES, PHASES, RIM_PHASES, ROUTE_PHASES, SPILL_PHASES, GroupPonds,  # noqa: E402
                            Ponds)

MISS = -99999.0


def bytes_model(rows, ncp, wet_cells, n):
    """what each phase must move at least, in bytes"""
    cells, segs = rows * ncp, rows * ((ncp + 63) // 64)
    return {
        "mask": 16 * cells + 8 * segs,                       # water + DEM in, masks out (run-start parents on top)
        "merge": 4 * 8 * segs + 4 * segs,                    # own mask and three neighbours, union counts out
        "flatten": 8 * segs + 12 * segs,                     # masks in, root masks and counts out
        "scan": 3 * 4 * segs + 4 * segs,                     # counts and union counts in, counts in, offsets out
        "table": 8 * wet_cells + 4 * cells + 8 * segs + 48 * n,   # wet water in, labels out, masks in, table
        "finish": 16 * n,
    }


def rims_bytes_model(rows, ncp, wet_cells, rim_lanes, n):
    """what the two rim phases must move at least: dem and w of pond cells and of their dry neighbours, the labels of the pond
    cells (a wet lane's label is read, a dry lane's is 0 by its mask), masks; the locate pass the dry neighbours again"""
    segs = rows * ((ncp + 63) // 64)
    return {"rims": 16 * (wet_cells + rim_lanes) + 4 * wet_cells + 3 * 8 * segs + 48 * n,
            "locate": 16 * rim_lanes + 3 * 8 * segs + 48 * n}


def rims_job(ctx, p, rec, n):
    """after the label calls: one untimed label_rims (allocates the rim table), five timed ones"""
    p.label_rims(0.001)
    wall, phases, table_ms = [], {k: [] for k in RIM_PHASES}, []
    for _ in range(5):
        ctx.synchronize()
        t0 = time.perf_counter()
        p.label_rims(0.001)
        wall.append((time.perf_counter() - t0) * 1e3)
        for k, v in p.rims_phase_ms().items():
            phases[k].append(v)
        table_ms.append(p.phase_ms()["table"])
    rims = p.rims()
    med = {k: statistics.median(v) for k, v in phases.items()}
    rec["rims"] = dict(label_rims_wall_ms=statistics.median(wall), label_rims_wall_ms_all=wall, phase_ms=med, phase_ms_all=phases,
                       table_ms_same_calls=statistics.median(table_ms),
                       rims_plus_locate_over_table=(med["rims"] + med["locate"]) / statistics.median(table_ms),
                       rim_memberships=int(rims["rim_cells"].sum()), wall_memberships=int(rims["wall_cells"].sum()),
                       longest_shoreline=int(rims["rim_cells"].max()) if len(rims) else 0,
                       ponds_without_rim=int((rims["rim_cells"] == 0).sum()),
                       spilling=int((rims["rim_level"] - rims["surface_max"] <= 0).sum()), guard_bad=p.guard_bad())
    # every membership is a lane at most, and at least a quarter of one: bytes from the upper bound of lanes
    model = rims_bytes_model(n + 2, n + 2, rec["wet_cells"], rec["rims"]["rim_memberships"] + rec["rims"]["wall_memberships"], len(rims))
    rec["rims"]["bytes_model_upper"] = model
    rec["rims"]["gbps_upper"] = {k: model[k] / (med[k] * 1e6) if med[k] > 0 else None for k in RIM_PHASES}


def catchments_bytes_model(rows, ncp, caught):
    """the algorithmic traffic of the catchment phases: receivers dem 8, w 8, label 4, link 4 per cell (rows of pond cells alone
    read neither dem nor w: the model is an upper bound there); a jump round at least one link per cell; the tally a link in and a
    basin out per cell, and dem and w of the slope cells that drain to a pond"""
    cells = rows * ncp
    return {"receivers": 24 * cells, "jump_per_round": 4 * cells, "tally": 8 * cells + 16 * caught}


def catchments_job(ctx, p, rec, n):
    """after the label calls: one untimed label_catchments (allocates links and table), then five pairs of label_rims and
    label_catchments, interleaved: what the new pass costs, and whether the phases it sits beside notice it"""
    p.label_catchments(0.001)
    shared = list(PHASES) + list(RIM_PHASES)
    wall = {"rims": [], "catchments": []}
    beside = {"rims": {k: [] for k in shared}, "catchments": {k: [] for k in shared}}
    phases, rounds = {k: [] for k in CATCH_PHASES}, []
    for _ in range(5):
        for which, call in (("rims", p.label_rims), ("catchments", p.label_catchments)):
            ctx.synchronize()
            t0 = time.perf_counter()
            call(0.001)
            wall[which].append((time.perf_counter() - t0) * 1e3)
            for k, v in list(p.phase_ms().items()) + list(p.rims_phase_ms().items()):
                beside[which][k].append(v)
        for k, v in p.catchment_phase_ms().items():
            phases[k].append(v)
        rounds.append(p.catchment_stats()["rounds"])
    catch, stats = p.catchments(), p.catchment_stats()
    med = {k: statistics.median(v) for k, v in phases.items()}
    table_ms = statistics.median(beside["catchments"]["table"])
    model = catchments_bytes_model(n + 2, n + 2, int(catch["catch_cells"].sum()))
    c = rec["catchments"] = dict(
        wall_ms={k: statistics.median(v) for k, v in wall.items()}, wall_ms_all=wall, phase_ms=med, phase_ms_all=phases,
        table_ms_same_calls=table_ms, over_table={k: med[k] / table_ms for k in CATCH_PHASES}, rounds=rounds, stats=stats,
        beside_ms={w: {k: statistics.median(v) for k, v in ph.items()} for w, ph in beside.items()}, beside_ms_all=beside,
        caught_cells=int(catch["catch_cells"].sum()), inflow_cells=int(catch["inflow_cells"].sum()),
        largest_catchment=int(catch["catch_cells"].max()) if len(catch) else 0, bytes_model=model, guard_bad=p.guard_bad())
    c["gbps"] = {"receivers": model["receivers"] / (med["receivers"] * 1e6), "tally": model["tally"] / (med["tally"] * 1e6),
                 "jump": model["jump_per_round"] * rounds[-1] / (med["jump"] * 1e6)}
    if rec.get("hbm_yardstick_gbps"):
        c["of_yardstick"] = {k: v / rec["hbm_yardstick_gbps"] for k, v in c["gbps"].items()}


def outlets_job(ctx, p, rec, n):
    """after the label calls: one untimed label_outlets (allocates the basin raster and every table), five timed ones"""
    p.label_outlets(0.001)
    wall, phases, table_ms = [], {k: [] for k in OUTLET_PHASES}, []
    for _ in range(5):
        ctx.synchronize()
        t0 = time.perf_counter()
        p.label_outlets(0.001)
        wall.append((time.perf_counter() - t0) * 1e3)
        for k, v in p.outlet_phase_ms().items():
            phases[k].append(v)
        table_ms.append(p.phase_ms()["table"])
    table, stats = p.outlets(), p.outlet_stats()
    med = {k: statistics.median(v) for k, v in phases.items()}
    tms = statistics.median(table_ms)
    cells = (n + 2) * (n + 2)
    o = rec["outlets"] = dict(
        label_outlets_wall_ms=statistics.median(wall), label_outlets_wall_ms_all=wall, phase_ms=med, phase_ms_all=phases,
        table_ms_same_calls=tms, over_table={k: med[k] / tms for k in OUTLET_PHASES}, stats=stats,
        fill_cells=int(table["fill_cells"].sum()), largest_divide=int(table["divide_cells"].max()) if len(table) else 0,
        bytes_model={"per_pass_20B": 20 * cells, "per_pass_4B": 4 * cells}, guard_bad=p.guard_bad())
    o["gbps"] = {k: {"20B": 20 * cells / (med[k] * 1e6), "4B": 4 * cells / (med[k] * 1e6)} if med[k] > 0 else None for k in OUTLET_PHASES}
    if rec.get("hbm_yardstick_gbps"):
        o["of_yardstick"] = {k: {m: r / rec["hbm_yardstick_gbps"] for m, r in v.items()} if v else None for k, v in o["gbps"].items()}


def curves_job(ctx, p, rec, n):
    """after the label calls: one untimed label_curves (allocates the curve table and everything below it), five timed ones"""
    p.label_curves(0.001)
    beside_names = ("table", "passes", "locate")
    wall, phases, beside = [], {k: [] for k in CURVE_PHASES}, {k: [] for k in beside_names}
    for _ in range(5):
        ctx.synchronize()
        t0 = time.perf_counter()
        p.label_curves(0.001)
        wall.append((time.perf_counter() - t0) * 1e3)
        for k, v in p.curve_phase_ms().items():
            phases[k].append(v)
        beside["table"].append(p.phase_ms()["table"])
        for k, v in p.outlet_phase_ms().items():
            beside[k].append(v)
    table, stats = p.curves(), p.curve_stats()
    med = {k: statistics.median(v) for k, v in phases.items()}
    bmed = {k: statistics.median(v) for k, v in beside.items()}
    cells = (n + 2) * (n + 2)
    c = rec["curves"] = dict(
        label_curves_wall_ms=statistics.median(wall), label_curves_wall_ms_all=wall, phase_ms=med, phase_ms_all=phases,
        beside_ms_same_calls=bmed, beside_ms_all=beside,
        over={b: {k: med[k] / bmed[b] if bmed[b] > 0 else None for k in CURVE_PHASES} for b in beside_names}, stats=stats,
        basin_cells_with_a_curve=int(stats["stage_cells"]), largest_stage_count=int(table["cells"][:, -1].max()) if len(table) else 0,
        table_bytes=int(table.nbytes), bytes_model={"per_pass_12B": 12 * cells}, guard_bad=p.guard_bad())
    c["gbps_12B"] = {k: 12 * cells / (med[k] * 1e6) if med[k] > 0 else None for k in CURVE_PHASES}
    if rec.get("hbm_yardstick_gbps"):
        c["of_yardstick"] = {k: v / rec["hbm_yardstick_gbps"] if v else None for k, v in c["gbps_12B"].items()}


def spills_job(ctx, p, rec, n):
    """after the label calls: one untimed label_spills (allocates the spill table, its working arrays and everything below it), five
    timed ones"""
    p.label_spills(0.001, 0.0)
    beside_names = ("table", "passes", "locate", "bed", "stages")
    wall, phases, beside = [], {k: [] for k in SPILL_PHASES}, {k: [] for k in beside_names}
    for _ in range(5):
        ctx.synchronize()
        t0 = time.perf_counter()
        p.label_spills(0.001, 0.0)
        wall.append((time.perf_counter() - t0) * 1e3)
        for k, v in p.spill_phase_ms().items():
            phases[k].append(v)
        beside["table"].append(p.phase_ms()["table"])
        for k, v in list(p.outlet_phase_ms().items()) + list(p.curve_phase_ms().items()):
            beside[k].append(v)
    table, stats = p.spills(), p.spill_stats()
    med = {k: statistics.median(v) for k, v in phases.items()}
    bmed = {k: statistics.median(v) for k, v in beside.items()}
    npond = len(table)
    rec["spills"] = dict(
        label_spills_wall_ms=statistics.median(wall), label_spills_wall_ms_all=wall, phase_ms=med, phase_ms_all=phases,
        spill_pass_ms=sum(med.values()), beside_ms_same_calls=bmed, beside_ms_all=beside,
        over_table={k: med[k] / bmed["table"] if bmed["table"] > 0 else None for k in SPILL_PHASES},
        spill_pass_over_table=sum(med.values()) / bmed["table"] if bmed["table"] > 0 else None, stats=stats,
        most_direct_feeders=int(np.bincount(table["next"][table["next"] > 0]).max()) if (table["next"] > 0).any() else 0,
        largest_up_ponds=int(table["up_ponds"].max()) if npond else 0, largest_live_ponds=int(table["live_ponds"].max()) if npond else 0,
        table_bytes=int(table.nbytes), working_bytes=npond * (15 * 4 + 14 * 8), guard_bad=p.guard_bad())


def routing_job(ctx, p, rec, runoffs_mm):
    """after the label calls, per runoff depth: one untimed label_routing (allocates), five timed ones, five timed reruns"""
    rec["routing"] = []
    for mm in runoffs_mm:
        r = mm / 1000.0
        p.label_routing(0.001, r, 0.0)
        wall, phases = [], {k: [] for k in ROUTE_PHASES}
        beside = {k: [] for k in ("table",) + SPILL_PHASES}
        for _ in range(5):
            ctx.synchronize()
            t0 = time.perf_counter()
            p.label_routing(0.001, r, 0.0)
            wall.append((time.perf_counter() - t0) * 1e3)
            for k, v in p.routing_phase_ms().items():
                phases[k].append(v)
            beside["table"].append(p.phase_ms()["table"])
            for k, v in p.spill_phase_ms().items():
                beside[k].append(v)
        rerun_wall, rerun = [], {k: [] for k in ROUTE_PHASES}
        for _ in range(5):
            ctx.synchronize()
            t0 = time.perf_counter()
            p.route(r)
            rerun_wall.append((time.perf_counter() - t0) * 1e3)
            for k, v in p.routing_phase_ms().items():
                rerun[k].append(v)
        table, stats = p.routing(), p.routing_stats()
        med = {k: statistics.median(v) for k, v in phases.items()}
        bmed = {k: statistics.median(v) for k, v in beside.items()}
        npond = len(table)
        rec["routing"].append(dict(
            runoff_mm=mm, label_routing_wall_ms=statistics.median(wall), label_routing_wall_ms_all=wall, phase_ms=med, phase_ms_all=phases,
            routing_pass_ms=sum(med.values()), beside_ms_same_calls=bmed, beside_ms_all=beside,
            routing_pass_over_table=sum(med.values()) / bmed["table"] if bmed["table"] > 0 else None,
            routing_pass_over_spill_pass=sum(med.values()) / sum(bmed[k] for k in SPILL_PHASES) if sum(bmed[k] for k in SPILL_PHASES) > 0 else None,
            rerun_wall_ms=statistics.median(rerun_wall), rerun_wall_ms_all=rerun_wall,
            rerun_phase_ms={k: statistics.median(v) for k, v in rerun.items()}, stats=stats,
            largest_reach_ponds=int(table["reach_ponds"].max()) if npond else 0, largest_reach_cells=int(table["reach_cells"].max()) if npond else 0,
            largest_level=int(np.bincount(table["level"]).max()) if npond else 0, table_bytes=int(table.nbytes),
            working_bytes=npond * (3 * 4 + 5 * 8) + 8 * (stats["levels"] + 1), guard_bad=p.guard_bad()))


def yardstick_gbps(path):
    """the best rate tools/hbm_yardstick.hip reached on this box (its lines end in `<ms> ms  <rate> GB/s`)"""
    rates = [float(m.group(1)) for m in re.finditer(r"([0-9.]+) GB/s\s*$", open(path).read(), flags=re.M)]
    if not rates:
        raise SystemExit(f"{path}: no `GB/s` line of tools/_build/hbm_yardstick")
    return max(rates)


def group_job(hip, a, bd, bw, iters, rec):
    """the job over row blocks: one untimed label call, five timed ones"""
    from wdpm_amd.rowblock import Group
    n = a.n
    devices = [int(d) for d in a.devices.split(",")]
    rec["devices"] = devices
    with Group(hip, "add", n, n, MISS, devices) as grp:
        grp.upload(bd, bw)
        grp.run_block(iters, 0.005 / 1000)
        with GroupPonds(grp) as p:
            npond = p.label(0.001)                             # untimed: allocates
            wall, stitch = [], []
            phases = [{k: [] for k in PHASES} for _ in devices]
            for _ in range(5):
                t0 = time.perf_counter()
                p.label(0.001)
                wall.append((time.perf_counter() - t0) * 1e3)
                stitch.append(p.stats()["stitch_ms"])
                for i in range(len(devices)):
                    for k, v in p.phase_ms(i).items():
                        phases[i][k].append(v)
            rec.update(ponds=npond, stats=p.stats(), rank_stats=[p.rank_stats(i) for i in range(len(devices))],
                       label_wall_ms=statistics.median(wall), label_wall_ms_all=wall, stitch_ms=statistics.median(stitch),
                       rank_phase_ms=[{k: statistics.median(v) for k, v in ph.items()} for ph in phases], guard_bad=p.guard_bad())
            rec["rank_kernels_ms"] = [sum(ph.values()) for ph in rec["rank_phase_ms"]]
            rec["wet_cells"] = int(p.table()["cells"].sum())
            if a.rims:
                group_rims_job(p, rec, len(devices))
            if a.catchments:
                group_catchments_job(p, rec, len(devices))
            if a.outlets:
                group_outlets_job(p, rec, len(devices))
            if a.curves:
                group_curves_job(p, rec, len(devices))
    if a.curves:                                               # the yardstick: the whole-raster call on the same water, same process
        with hip.context(module="add", nrows=n, ncols=n, missingvalue=MISS) as ctx:
            ctx.upload(bd, bw)
            if iters > 0:
                ctx.run_block(iters, 0.005 / 1000)
            with Ponds(ctx) as p:
                p.label_curves(0.001)
                phases, wall = {k: [] for k in CURVE_PHASES}, []
                for _ in range(5):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    p.label_curves(0.001)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    for k, v in p.curve_phase_ms().items():
                        phases[k].append(v)
                whole = {k: statistics.median(v) for k, v in phases.items()}
                c = rec["curves"]
                c.update(whole_raster_phase_ms=whole, whole_raster_phase_ms_all=phases, whole_raster_stats=p.curve_stats(),
                         whole_raster_wall_ms=statistics.median(wall), whole_raster_wall_ms_all=wall)
                c["sum_over_ranks_over_whole_raster"] = {k: c["phase_sum_over_ranks_ms"][k] / whole[k] if whole[k] > 0 else None for k in CURVE_PHASES}
                c["wall_over_whole_raster_wall"] = c["label_stage_curves_wall_ms"] / c["whole_raster_wall_ms"]
                print(f"whole raster: bed {whole['bed']:.3f} ms  stages {whole['stages']:.3f} ms  wall {c['whole_raster_wall_ms']:.3f} ms", file=sys.stderr)
    if a.outlets:                                              # the yardstick: the whole-raster call on the same water, same process
        with hip.context(module="add", nrows=n, ncols=n, missingvalue=MISS) as ctx:
            ctx.upload(bd, bw)
            if iters > 0:
                ctx.run_block(iters, 0.005 / 1000)
            with Ponds(ctx) as p:
                p.label_outlets(0.001)
                phases = {k: [] for k in OUTLET_PHASES}
                for _ in range(5):
                    p.label_outlets(0.001)
                    for k, v in p.outlet_phase_ms().items():
                        phases[k].append(v)
                whole = {k: statistics.median(v) for k, v in phases.items()}
                o = rec["outlets"]
                o.update(whole_raster_phase_ms=whole, whole_raster_phase_ms_all=phases, whole_raster_stats=p.outlet_stats())
                o["sum_over_ranks_over_whole_raster"] = {k: o["phase_sum_over_ranks_ms"][k] / whole[k] if whole[k] > 0 else None for k in OUTLET_PHASES}
    if a.catchments:                                           # the yardstick: the whole-raster call on the same water, same process
        with hip.context(module="add", nrows=n, ncols=n, missingvalue=MISS) as ctx:
            ctx.upload(bd, bw)
            if iters > 0:
                ctx.run_block(iters, 0.005 / 1000)
            with Ponds(ctx) as p:
                p.label_catchments(0.001)
                phases = {k: [] for k in CATCH_PHASES}
                for _ in range(5):
                    p.label_catchments(0.001)
                    for k, v in p.catchment_phase_ms().items():
                        phases[k].append(v)
                whole = {k: statistics.median(v) for k, v in phases.items()}
                c = rec["catchments"]
                c.update(whole_raster_phase_ms=whole, whole_raster_phase_ms_all=phases, whole_raster_stats=p.catchment_stats())
                c["sum_over_ranks_over_whole_raster"] = {k: c["phase_sum_over_ranks_ms"][k] / whole[k] if whole[k] > 0 else None for k in CATCH_PHASES}
                c["all_phases_sum_over_ranks_over_whole_raster"] = sum(c["phase_sum_over_ranks_ms"].values()) / sum(whole.values())


def group_rims_job(p, rec, nranks):
    """after the label calls: one untimed label_rims (allocates every rank's rim rows and slots), five timed ones"""
    p.label_rims(0.001)
    wall, merge, stitch = [], [], []
    phases = [{k: [] for k in RIM_PHASES} for _ in range(nranks)]
    table_ms = [[] for _ in range(nranks)]
    for _ in range(5):
        t0 = time.perf_counter()
        p.label_rims(0.001)
        wall.append((time.perf_counter() - t0) * 1e3)
        merge.append(p.rims_stats()["merge_ms"])
        stitch.append(p.stats()["stitch_ms"])
        for i in range(nranks):
            for k, v in p.rims_phase_ms(i).items():
                phases[i][k].append(v)
            table_ms[i].append(p.phase_ms(i)["table"])
    rims, rstats = p.rims(), p.rims_stats()
    sums = [sum(phases[i][k][j] for i in range(nranks) for k in RIM_PHASES) for j in range(5)]     # per call, over ranks
    rec["rims"] = dict(label_rims_wall_ms=statistics.median(wall), label_rims_wall_ms_all=wall,
                       rank_phase_ms=[{k: statistics.median(v) for k, v in ph.items()} for ph in phases], rank_phase_ms_all=phases,
                       rims_plus_locate_sum_over_ranks_ms=statistics.median(sums), rims_plus_locate_sum_over_ranks_ms_all=sums,
                       rank_table_ms_same_calls=[statistics.median(v) for v in table_ms],
                       merge_ms=statistics.median(merge), merge_ms_all=merge, stitch_ms_same_calls=statistics.median(stitch),
                       foreign=rstats["foreign"], slots=rstats["slots"],
                       rim_memberships=int(rims["rim_cells"].sum()), wall_memberships=int(rims["wall_cells"].sum()),
                       longest_shoreline=int(rims["rim_cells"].max()) if len(rims) else 0,
                       ponds_without_rim=int((rims["rim_cells"] == 0).sum()),
                       spilling=int((rims["rim_level"] - rims["surface_max"] <= 0).sum()), guard_bad=p.guard_bad())


def group_catchments_job(p, rec, nranks):
    """after the label calls: one untimed label_catchments (allocates every rank's links, keys and rows), five timed ones"""
    p.label_catchments(0.001)
    wall, resolve = [], []
    phases = [{k: [] for k in CATCH_PHASES} for _ in range(nranks)]
    table_ms = [[] for _ in range(nranks)]
    for _ in range(5):
        t0 = time.perf_counter()
        p.label_catchments(0.001)
        wall.append((time.perf_counter() - t0) * 1e3)
        resolve.append(p.catchment_stats()["resolve_ms"])
        for i in range(nranks):
            for k, v in p.catchment_phase_ms(i).items():
                phases[i][k].append(v)
            table_ms[i].append(p.phase_ms(i)["table"])
    catch, stats = p.catchments(), p.catchment_stats()
    sums = {k: statistics.median([sum(phases[i][k][j] for i in range(nranks)) for j in range(5)]) for k in CATCH_PHASES}   # per call, over ranks
    rec["catchments"] = dict(label_catchments_wall_ms=statistics.median(wall), label_catchments_wall_ms_all=wall,
                             rank_phase_ms=[{k: statistics.median(v) for k, v in ph.items()} for ph in phases], rank_phase_ms_all=phases,
                             phase_sum_over_ranks_ms=sums, rank_table_ms_same_calls=[statistics.median(v) for v in table_ms],
                             resolve_ms=statistics.median(resolve), resolve_ms_all=resolve, stats=stats, exits=stats["exits"],
                             crossings=stats["crossings"], remote=stats["remote"], caught_cells=int(catch["catch_cells"].sum()),
                             inflow_cells=int(catch["inflow_cells"].sum()), guard_bad=p.guard_bad())


def group_outlets_job(p, rec, nranks):
    """after the label calls: one untimed label_outlets (allocates every rank's slots, keys and rows), five timed ones"""
    p.label_outlets(0.001)
    wall, merge = [], []
    phases = [{k: [] for k in OUTLET_PHASES} for _ in range(nranks)]
    table_ms = [[] for _ in range(nranks)]
    for _ in range(5):
        t0 = time.perf_counter()
        p.label_outlets(0.001)
        wall.append((time.perf_counter() - t0) * 1e3)
        merge.append(p.outlet_stats()["merge_ms"])
        for i in range(nranks):
            for k, v in p.outlet_phase_ms(i).items():
                phases[i][k].append(v)
            table_ms[i].append(p.phase_ms(i)["table"])
    table, stats = p.outlets(), p.outlet_stats()
    sums = {k: statistics.median([sum(phases[i][k][j] for i in range(nranks)) for j in range(5)]) for k in OUTLET_PHASES}   # per call, over ranks
    rec["outlets"] = dict(label_outlets_wall_ms=statistics.median(wall), label_outlets_wall_ms_all=wall,
                          rank_phase_ms=[{k: statistics.median(v) for k, v in ph.items()} for ph in phases], rank_phase_ms_all=phases,
                          phase_sum_over_ranks_ms=sums, rank_table_ms_same_calls=[statistics.median(v) for v in table_ms],
                          merge_ms=statistics.median(merge), merge_ms_all=merge, stats=stats, seam_outlets=stats["seam_outlets"],
                          split_ponds=stats["split_ponds"], fill_cells=int(table["fill_cells"].sum()),
                          largest_divide=int(table["divide_cells"].max()) if len(table) else 0, guard_bad=p.guard_bad())
    for i in range(nranks):
        print(f"rank {i}: passes {rec['outlets']['rank_phase_ms'][i]['passes']:.3f} ms  locate {rec['outlets']['rank_phase_ms'][i]['locate']:.3f} ms",
              file=sys.stderr)
    print(f"merge_ms {rec['outlets']['merge_ms']:.3f}", file=sys.stderr)


def group_curves_job(p, rec, nranks):
    """after the label calls: one untimed label_stage_curves (allocates every rank's slot rows and keys), five timed ones"""
    p.label_stage_curves(0.001)
    wall, merge = [], []
    phases = [{k: [] for k in CURVE_PHASES} for _ in range(nranks)]
    table_ms = [[] for _ in range(nranks)]
    for _ in range(5):
        t0 = time.perf_counter()
        p.label_stage_curves(0.001)
        wall.append((time.perf_counter() - t0) * 1e3)
        merge.append(p.stage_curve_stats()["merge_ms"])
        for i in range(nranks):
            for k, v in p.stage_curve_phase_ms(i).items():
                phases[i][k].append(v)
            table_ms[i].append(p.phase_ms(i)["table"])
    table, stats = p.stage_curves(), p.stage_curve_stats()
    slots = p.catchment_stats()["remote"] + p.rims_stats()["slots"]
    sums = {k: statistics.median([sum(phases[i][k][j] for i in range(nranks)) for j in range(5)]) for k in CURVE_PHASES}   # per call, over ranks
    c = rec["curves"] = dict(label_stage_curves_wall_ms=statistics.median(wall), label_stage_curves_wall_ms_all=wall,
                             rank_phase_ms=[{k: statistics.median(v) for k, v in ph.items()} for ph in phases], rank_phase_ms_all=phases,
                             phase_sum_over_ranks_ms=sums, rank_table_ms_same_calls=[statistics.median(v) for v in table_ms],
                             merge_ms=statistics.median(merge), merge_ms_all=merge, stats=stats, split_basins=stats["split_basins"],
                             remote_beds=stats["remote_beds"], slots=slots, slot_row_bytes_down=272 * slots, bed_key_bytes_each_way=8 * slots,
                             table_bytes=int(table.nbytes), guard_bad=p.guard_bad())
    for i in range(nranks):
        print(f"rank {i}: bed {c['rank_phase_ms'][i]['bed']:.3f} ms  stages {c['rank_phase_ms'][i]['stages']:.3f} ms", file=sys.stderr)
    print(f"merge_ms {c['merge_ms']:.3f}  wall {c['label_stage_curves_wall_ms']:.3f} ms  slots {slots}", file=sys.stderr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("job", choices=["wet", "ponds", "noise"])
    ap.add_argument("n", type=int)
    ap.add_argument("--out", help="default: profiles/r10/ponds.json, with --devices profiles/r11/ponds_group.json")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--yardstick", metavar="FILE",
                    help="output of tools/_build/hbm_yardstick from the same box: its best streaming rate goes into the record")
    ap.add_argument("--devices", metavar="a,b,...", help="label over row blocks, one per device named (wdpm_amd.ponds.GroupPonds)")
    ap.add_argument("--rims", action="store_true", help="time label_rims as well: the rim and locate phases beside the table phase")
    ap.add_argument("--catchments", action="store_true",
                    help="time label_catchments as well, interleaved with label_rims: the receiver, jump and tally phases")
    ap.add_argument("--outlets", action="store_true", help="time label_outlets as well: the passes and locate phases beside the table phase")
    ap.add_argument("--curves", action="store_true",
                    help="time label_curves (with --devices: label_stage_curves) as well: the bed and stages phases beside table, passes and locate")
    ap.add_argument("--spills", action="store_true",
                    help="time label_spills as well: the rings, chains and sums phases beside table, passes, locate, bed and stages")
    ap.add_argument("--routing", action="store_true",
                    help="time label_routing and route() as well: the order, sweep and finish phases beside table, rings, chains and sums")
    ap.add_argument("--runoff-mm", default="1,10,100", metavar="a,b,...", help="the runoff depths of --routing, in millimetres")
    ap.add_argument("--iterations", type=int, help="iterations before the inventory, instead of the job's own")
    ap.add_argument("--lib", metavar="FILE", help="time this build of the library (tools/build_alt.sh) instead of the tree's own")
    a = ap.parse_args()
    if a.spills and a.devices:
        ap.error("--spills: spills are taken on a whole raster only")
    if a.routing and a.devices:
        ap.error("--routing: routing is taken on a whole raster only")
    if not a.out:
        a.out = os.path.join(ROOT, "profiles", *(("r24", "pond_curves_group.json") if a.devices and a.curves else
                                                  ("r17", "pond_outlets_group.json") if a.devices and a.outlets else
                                                  ("r16", "pond_catchments_group.json") if a.devices and a.catchments else
                                                  ("r13", "pond_rims_group.json") if a.devices and a.rims else
                                                  ("r11", "ponds_group.json") if a.devices else
                                                  ("r28", "pond_routing.json") if a.routing else
                                                  ("r26", "pond_spills.json") if a.spills else
                                                  ("r18", "pond_curves.json") if a.curves else
                                                  ("r15", "pond_outlets.json") if a.outlets else
                                                  ("r14", "pond_catchments.json") if a.catchments else
                                                  ("r12", "pond_rims.json") if a.rims else ("r10", "ponds.json")))
    hip = wdpm_amd.load(a.lib) if a.lib else wdpm_amd.load_hip()
    n = a.n
    dem = hip.synth_dem(n, n)
    if a.job == "wet":
        water, iters = np.full((n, n), 0.1), 1000
    elif a.job == "noise":
        rng = np.random.default_rng(41)
        water, iters = np.where(rng.random((n, n)) < 0.41, 0.002 + 2.0 * rng.random((n, n)), 0.0), 0
        dem[rng.random((n, n)) < 0.03] = MISS
    else:
        bi, bj = np.mgrid[0:n, 0:n] // 256
        water, iters = np.where((3 * bi + 5 * bj) % 8 == 0, 12.0, 0.0), 100
    if a.iterations is not None:
        iters = a.iterations
    bd = np.full((n + 2, n + 2), MISS)
    bd[1:-1, 1:-1] = dem
    bw = np.zeros((n + 2, n + 2))
    bw[1:-1, 1:-1] = water
    del dem, water
    rec = dict(job=a.job, n=n, iterations=iters, build=hip.dll.wdpm_build_info().decode())
    if a.yardstick:
        rec["hbm_yardstick_gbps"] = yardstick_gbps(a.yardstick)
    if a.devices:
        group_job(hip, a, bd, bw, iters, rec)
        line = json.dumps(rec)
        print(line)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        return
    with hip.context(module="add", nrows=n, ncols=n, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        rec["iteration_launch_ms"] = None
        if iters > 0:
            ctx.run_block(iters, 0.005 / 1000)
            ctx.timing_reset()
            ctx.run_block(20, 0.005 / 1000)
            launches, ms = ctx.timing_steady()
            rec["iteration_launch_ms"] = ms / max(launches, 1)
        with Ponds(ctx) as p:
            npond = p.label(0.001)                             # untimed: allocates
            wall, phases = [], {k: [] for k in PHASES}
            for _ in range(5):
                ctx.synchronize()
                t0 = time.perf_counter()
                p.label(0.001)
                wall.append((time.perf_counter() - t0) * 1e3)
                for k, v in p.phase_ms().items():
                    phases[k].append(v)
            table, stats = p.table(), p.stats()
            rec.update(ponds=npond, stats=stats, label_wall_ms=statistics.median(wall), label_wall_ms_all=wall,
                       phase_ms={k: statistics.median(v) for k, v in phases.items()}, guard_bad=p.guard_bad())
            rec["kernels_ms"] = sum(rec["phase_ms"].values())
            rec["in_iteration_launches"] = rec["kernels_ms"] / rec["iteration_launch_ms"] if rec["iteration_launch_ms"] else None
            wet = int(table["cells"].sum())
            rec["wet_cells"], rec["largest_pond_cells"] = wet, int(table["cells"].max()) if npond else 0
            model = bytes_model(n + 2, n + 2, wet, npond)
            rec["bytes_model"] = model
            rec["bytes_per_cell"] = sum(model.values()) / ((n + 2) * (n + 2))
            rec["gbps"] = {k: model[k] / (rec["phase_ms"][k] * 1e6) if rec["phase_ms"][k] > 0 else None for k in PHASES}
            if rec.get("hbm_yardstick_gbps"):
                rec["of_yardstick"] = {k: v / rec["hbm_yardstick_gbps"] if v else None for k, v in rec["gbps"].items()}
            if a.rims:
                rims_job(ctx, p, rec, n)
            if a.catchments:
                catchments_job(ctx, p, rec, n)
            if a.outlets:
                outlets_job(ctx, p, rec, n)
            if a.curves:
                curves_job(ctx, p, rec, n)
            if a.spills:
                spills_job(ctx, p, rec, n)
            if a.routing:
                routing_job(ctx, p, rec, [float(v) for v in a.runoff_mm.split(",")])
        if not a.no_scipy:
            try:
                import scipy.ndimage as ndi
                t0 = time.perf_counter()
                w = ctx.download_water()
                rec["download_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                _, nref = ndi.label((bd > MISS) & (w > 0.001), structure=np.ones((3, 3), dtype=int))
                rec["scipy_label_ms"] = (time.perf_counter() - t0) * 1e3
                rec["scipy_ponds"] = int(nref)
            except ImportError:
                rec["scipy_label_ms"] = None
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
