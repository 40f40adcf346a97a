"""Host model of the pond routing (include/wdpm_pond_routing.h) in plain Python - the yardstick of tests/test_pond_routing.py.

The ponds are taken in decreasing hops, one after another; each hands its overflow to the next pond, a sum of Python integers; and
reach_* comes from explicit walks upstream from every pond, through the feeders that overflow.  No histogram, no levels, no plan,
nothing concurrent.  tests/test_pond_routing_model.py holds it against hand-written answers and against brute_force() below, which
repeats out = f(in) over all ponds until nothing changes.

    table, stats = routing(spill_table, values, fill_q, runoff_q)
    table, stats, spill_table, spill_stats, tables = routing_of_water(bd, miss, water, min_depth, headroom_tol, runoff_m)

`values` is cells + catch_cells per pond and `fill_q` the outlet table's column.  Of the statistics, wide_levels and launches belong
to the device's plan and are not modelled: plan_of() counts them from the level sizes for the bounds a test has set.
"""
import math

import numpy as np

from pond_spills_model import spills_of_water

ROUTE_DTYPE = np.dtype([("own_q", "<u8"), ("in_q", "<u8"), ("kept_q", "<u8"), ("out_q", "<u8"), ("reach_ponds", "<i8"), ("reach_cells", "<i8"),
                        ("overflows", "<i4"), ("full", "<i4"), ("level", "<i4"), ("reserved", "<i4")])
STATS = ("ponds", "runoff_q", "levels", "overflowing", "full", "own_q", "kept_q", "out_land_q", "out_ring_q")   # those modelled
PLAN_STATS = ("wide_levels", "launches")
BLOCK = 256
RUN_LEVELS = 65536


def runoff_q_of(runoff_m):
    """rint(runoff_m * 2^24), or -1 where the call refuses: not finite, negative, 2^32 quanta and more"""
    m = float(runoff_m)
    if not (m >= 0.0) or math.isinf(m):
        return -1
    q = round(m * 2.0 ** 24)                                  # the product is exact; round() of a float rounds halves to even, as rint
    return q if q < 2 ** 32 else -1


def routing(spill_table, values, fill_q, runoff_q):
    n = len(spill_table)
    nxt = [int(v) for v in spill_table["next"]]
    hops = [int(v) for v in spill_table["hops"]]
    values = [int(v) for v in values]
    fq = [int(v) for v in fill_q]
    own = [runoff_q * v for v in values]
    inq, out = [0] * n, [0] * n
    feeders = [[] for _ in range(n)]
    for k in sorted(range(n), key=lambda k: -hops[k]):        # a pond has everything from above before its turn
        if nxt[k] != -1:
            out[k] = max(0, own[k] + inq[k] - fq[k])
        if nxt[k] > 0:
            inq[nxt[k] - 1] += out[k]
            feeders[nxt[k] - 1].append(k)
    table = np.zeros(n, dtype=ROUTE_DTYPE)
    for k in range(n):
        ponds, cells, stack = 0, 0, [k]                       # k and whatever reaches it through ponds that overflow
        while stack:
            u = stack.pop()
            ponds += 1
            cells += values[u]
            stack.extend(f for f in feeders[u] if out[f] > 0)
        assert own[k] + inq[k] < 2 ** 64
        table[k] = (own[k], inq[k], own[k] + inq[k] - out[k], out[k], ponds, cells, int(out[k] > 0),
                    int(nxt[k] != -1 and own[k] + inq[k] >= fq[k]), hops[k], 0)
    stats = {"ponds": n, "runoff_q": runoff_q, "levels": max(hops) + 1 if n else 0, "overflowing": sum(o > 0 for o in out),
             "full": int(table["full"].sum()), "own_q": sum(own), "kept_q": sum(int(v) for v in table["kept_q"]),
             "out_land_q": sum(out[k] for k in range(n) if nxt[k] == 0), "out_ring_q": sum(out[k] for k in range(n) if nxt[k] == -2)}
    return table, stats


def brute_force(nxt, values, fill_q, runoff_q):
    """out = f(in) over ALL ponds at once, again and again until nothing changes (a forest of depth d settles in d + 1 passes); the
    reach sums by walking every pond's whole chain downstream.  Returns lists: own, in, kept, out, reach_ponds, reach_cells."""
    n = len(nxt)
    own = [runoff_q * v for v in values]
    out = [0] * n
    for _ in range(n + 2):
        inq = [0] * n
        for u in range(n):
            if nxt[u] > 0:
                inq[nxt[u] - 1] += out[u]
        new = [0 if nxt[k] == -1 else max(0, own[k] + inq[k] - fill_q[k]) for k in range(n)]
        if new == out:
            break
        out = new
    else:
        raise AssertionError("the overflow did not settle: the graph is no forest")
    reach_p, reach_c = [0] * n, [0] * n
    for u in range(n):
        k = u
        while True:                                           # u counts for k while every pond from u up to, not including, k overflows
            reach_p[k] += 1
            reach_c[k] += values[u]
            if out[k] == 0 or nxt[k] <= 0:
                break
            k = nxt[k] - 1
    return own, inq, [own[k] + inq[k] - out[k] for k in range(n)], out, reach_p, reach_c


def routing_of_water(bd, miss, water, min_depth, headroom_tol, runoff_m):
    """the routing table of a padded DEM and its water, through the models of the older units"""
    spill_table, spill_stats, tables = spills_of_water(bd, miss, water, min_depth, headroom_tol)
    table, stats = routing_of_tables(spill_table, tables, runoff_q_of(runoff_m))
    return table, stats, spill_table, spill_stats, tables


def routing_of_tables(spill_table, tables, runoff_q):
    values = (np.asarray(tables["ponds"]["cells"], dtype=np.int64) + np.asarray(tables["catchments"]["catch_cells"], dtype=np.int64)).tolist()
    return routing(spill_table, values, [int(q) for q in tables["outlets"]["fill_q"].tolist()], runoff_q)


def level_sizes(spill_table):
    """how many ponds have hops == l, for l = 0 .. max_hops"""
    return np.bincount(np.asarray(spill_table["hops"], dtype=np.int64)).tolist() if len(spill_table) else []


def plan_of(sizes, narrow=BLOCK, run_levels=RUN_LEVELS):
    """the sweep's launches as include/wdpm_pond_routing.h words them, from the deepest level down: ('wide', level) for a level of
    more than `narrow` ponds, ('run', top level, levels) for consecutive smaller ones, at most run_levels to a run"""
    launches = []
    for l in range(len(sizes) - 1, -1, -1):
        if sizes[l] > narrow:
            launches.append(("wide", l))
        elif launches and launches[-1][0] == "run" and launches[-1][2] < run_levels:
            launches[-1] = ("run", launches[-1][1], launches[-1][2] + 1)
        else:
            launches.append(("run", l, 1))
    return launches


def assert_invariants(table, stats, spill_table, values, fill_q):
    """what holds of every routing table"""
    n = len(table)
    values = np.asarray(values, dtype=np.int64)
    fq = np.asarray(fill_q, dtype=np.uint64)
    nxt = spill_table["next"]
    ints = lambda name: [int(v) for v in table[name].tolist()]                          # noqa: E731
    own, inq, kept, out = ints("own_q"), ints("in_q"), ints("kept_q"), ints("out_q")
    assert sum(own) == sum(kept) + stats["out_land_q"] + stats["out_ring_q"] == stats["own_q"] and sum(kept) == stats["kept_q"]
    assert all(o + i == k + t for o, i, k, t in zip(own, inq, kept, out))
    assert own == [stats["runoff_q"] * int(v) for v in values.tolist()]
    over = table["overflows"] != 0
    assert (over == (table["out_q"] > 0)).all() and (table["full"][over] == 1).all() and (table["kept_q"][over] == fq[over]).all()
    assert (table["out_q"][nxt == -1] == 0).all() and (table["full"][nxt == -1] == 0).all()
    assert (table["level"] == spill_table["hops"]).all() and (table["reserved"] == 0).all()
    assert (table["reach_ponds"] >= 1).all() and (table["reach_cells"] >= values).all()
    assert (table["reach_ponds"] <= spill_table["up_ponds"]).all() and (table["reach_cells"] <= spill_table["up_cells"]).all()
    fed_q, fed_p, fed_c = np.zeros(n, dtype=np.uint64), np.ones(n, dtype=np.int64), values.copy()
    on = (nxt > 0) & over
    np.add.at(fed_q, nxt[on] - 1, table["out_q"][on])
    np.add.at(fed_p, nxt[on] - 1, table["reach_ponds"][on])
    np.add.at(fed_c, nxt[on] - 1, table["reach_cells"][on])
    assert (fed_q == table["in_q"]).all() and (fed_p == table["reach_ponds"]).all() and (fed_c == table["reach_cells"]).all()
    # the rule itself, pond by pond.  With the sums over the feeders above it leaves one table only: what a level holds follows from
    # the level above it
    assert out == [0 if j == -1 else max(0, o + i - f) for j, o, i, f in zip(nxt.tolist(), own, inq, [int(v) for v in fq.tolist()])]
    assert stats["overflowing"] == int(over.sum()) and stats["full"] == int(table["full"].sum()) and stats["ponds"] == n
    assert stats["out_land_q"] == sum(o for o, j in zip(out, nxt.tolist()) if j == 0)
    assert stats["out_ring_q"] == sum(o for o, j in zip(out, nxt.tolist()) if j == -2)


def assert_same_routing(table, stats, ref_table, ref_stats):
    """the whole table and the modelled counts, for equality"""
    assert table.dtype == ROUTE_DTYPE and len(table) == len(ref_table), (table.dtype, len(table), len(ref_table))
    for name in ROUTE_DTYPE.names:
        same = table[name] == ref_table[name]
        assert same.all(), f"{name}: {int((~same).sum())} ponds differ, first pond {int(np.flatnonzero(~same)[0]) + 1}: " \
                           f"{table[name][~same][0]!r} vs {ref_table[name][~same][0]!r}"
    assert {k: stats[k] for k in STATS} == ref_stats, (stats, ref_stats)
