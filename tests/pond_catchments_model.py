"""Host model of the pond catchments (include/wdpm_pond_catchments.h) in numpy - the yardstick of tests/test_pond_catchments.py.

Levels are the order-preserving integer image of a double.  Receivers come from eight shifted copies of the level raster, visited
in the order of their padded index, so the first of equals stays.  Basins come from ONE pass over the slope cells in ascending
order of their level: a receiver is strictly lower, hence already known.  Nothing here jumps pointers, and nothing knows about
segments, waves or masks.

    basin, table, stats = catchments(labels, dem, w, pond_table)

labels: the label raster (padded, int32, 0 = no pond, 1..n); dem: the device DEM, padded, +inf on NODATA and on the border
(pond_rims_model.device_dem); w: the water that was labelled; pond_table: the pond table of the same call (its boxes and cells).
"""
import numpy as np

from pond_rims_model import depth_from_key, depth_key

CATCH_DTYPE = np.dtype([("catch_cells", "<i8"), ("inflow_cells", "<i8"), ("head_level", "<f8"), ("row_min", "<i4"),
                        ("row_max", "<i4"), ("col_min", "<i4"), ("col_max", "<i4")])
STATS = ("slope_cells", "pit_cells", "unponded_cells", "rounds", "ponds")
OFFSETS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]     # ascending padded index


def levels(labels, dem, w):
    """(has a level, its key) per cell"""
    with np.errstate(invalid="ignore"):
        has = dem < np.inf
        lvl = np.where((labels > 0) | (w > 0), dem + w, dem)
    return has, depth_key(np.where(has, lvl, 0.0))


def receivers(labels, dem, w):
    """flat padded index of every cell's receiver, -1 where it has none (only slope cells are given one)"""
    rows, ncp = labels.shape
    has, key = levels(labels, dem, w)
    top = np.iinfo(np.uint64).max
    big = np.full((rows + 2, ncp + 2), top, dtype=np.uint64)
    ok = np.zeros((rows + 2, ncp + 2), dtype=bool)
    big[1:-1, 1:-1] = key
    ok[1:-1, 1:-1] = has
    best = key.copy()                                  # strictly below the cell's own ...
    rec = np.full((rows, ncp), -1, dtype=np.int64)
    cell = np.arange(rows * ncp, dtype=np.int64).reshape(rows, ncp)
    for dr, dc in OFFSETS:                             # ... and the first of equals stays
        k = big[1 + dr:1 + dr + rows, 1 + dc:1 + dc + ncp]
        lower = ok[1 + dr:1 + dr + rows, 1 + dc:1 + dc + ncp] & (k < best)
        best = np.where(lower, k, best)
        rec = np.where(lower, cell + dr * ncp + dc, rec)
    slope = has & (labels == 0)
    return np.where(slope, rec, -1), slope, has, key


def catchments(labels, dem, w, pond_table):
    labels = np.asarray(labels)
    dem = np.asarray(dem, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n = len(pond_table)
    rows, ncp = labels.shape
    rec, slope, has, key = receivers(labels, dem, w)
    basin = np.where(has, labels, -1).astype(np.int32).ravel()
    flat_rec, flat_key = rec.ravel(), key.ravel()
    todo = np.flatnonzero(slope.ravel())
    for i in todo[np.argsort(flat_key[todo], kind="stable")].tolist():        # lowest first
        j = flat_rec[i]
        basin[i] = basin[j] if j >= 0 else 0
    basin = basin.reshape(rows, ncp)

    table = np.zeros(n, dtype=CATCH_DTYPE)
    table["head_level"] = -np.inf
    for name in ("row_min", "row_max", "col_min", "col_max"):
        table[name] = pond_table[name]
    caught = slope & (basin > 0)
    rr, cc = np.nonzero(caught)
    k = basin[rr, cc].astype(np.int64) - 1
    table["catch_cells"] = np.bincount(k, minlength=n)
    to = flat_rec[np.flatnonzero(slope.ravel() & (flat_rec >= 0))]
    into = labels.ravel()[to]
    table["inflow_cells"] = np.bincount(into[into > 0].astype(np.int64) - 1, minlength=n)
    if len(k):
        head = np.zeros(n, dtype=np.uint64)
        np.maximum.at(head, k, key[rr, cc])
        some = table["catch_cells"] > 0
        table["head_level"][some] = depth_from_key(head[some])
        for name, src, op in (("row_min", rr, np.minimum), ("row_max", rr, np.maximum), ("col_min", cc, np.minimum),
                              ("col_max", cc, np.maximum)):
            v = table[name].astype(np.int64)
            op.at(v, k, src)
            table[name] = v
    stats = {"slope_cells": int(slope.sum()), "pit_cells": int((slope & (rec < 0)).sum()),
             "unponded_cells": int((slope & (basin == 0)).sum()), "ponds": n}
    # the identity of include/wdpm_pond_catchments.h
    assert int(pond_table["cells"].sum()) + int(table["catch_cells"].sum()) + stats["unponded_cells"] == int(has.sum())
    return basin, table, stats


def descent_length(labels, dem, w):
    """hops of the longest descent (a plain walk, for the tests that want a long one)"""
    rec, slope, _, key = receivers(labels, dem, w)
    flat_rec, hops = rec.ravel(), np.zeros(rec.size, dtype=np.int64)
    todo = np.flatnonzero(slope.ravel())
    for i in todo[np.argsort(key.ravel()[todo], kind="stable")].tolist():
        j = flat_rec[i]
        if j >= 0:
            hops[i] = hops[j] + 1
    return int(hops.max()) if hops.size else 0


def assert_same_catchments(basin, table, stats, ref_basin, ref_table, ref_stats):
    """the whole basin raster, the whole table and the counts: integers by value, doubles by bit pattern"""
    assert basin.dtype == np.int32 and basin.shape == ref_basin.shape
    bad = np.argwhere(basin != ref_basin)
    assert bad.size == 0, f"{len(bad)} cells in another basin, first at {bad[0].tolist()}: {basin[tuple(bad[0])]} vs {ref_basin[tuple(bad[0])]}"
    assert table.dtype == CATCH_DTYPE and len(table) == len(ref_table), (table.dtype, len(table), len(ref_table))
    for name in CATCH_DTYPE.names:
        a, b = np.ascontiguousarray(table[name]), np.ascontiguousarray(ref_table[name])
        same = a.view(np.uint64) == b.view(np.uint64) if a.dtype.kind == "f" else a == b
        assert same.all(), f"{name}: {int((~same).sum())} ponds differ, first pond {int(np.flatnonzero(~same)[0]) + 1}: {a[~same][0]!r} vs {b[~same][0]!r}"
    for name, v in ref_stats.items():
        assert stats[name] == v, (name, stats[name], v)
