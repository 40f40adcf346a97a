"""Host model of the pond outlets (include/wdpm_pond_outlets.h) in numpy - the yardstick of tests/test_pond_outlets.py.

The basin raster comes from tests/pond_catchments_model.py.  Eight shifted copies of it give EVERY ordered pair of neighbours; the
pairs of two different basins >= 0 whose first cell lies in a pond's basin are the passes; one lexicographic sort by (pond, height,
index of the first cell, direction) puts every pond's outlet first, which is the tie rule as it is written.  The fill sums are
Python integers.  Nothing here knows about segments, waves, windows or skipped rows.

    table, stats = outlets(labels, dem, w, pond_table)              # raises TooDeep where the call must fail

labels: the label raster (padded, int32, 0 = no pond, 1..n); dem: the device DEM, padded, +inf on NODATA and on the border
(pond_rims_model.device_dem); w: the water that was labelled; pond_table: the pond table of the same call.
"""
import numpy as np

from pond_catchments_model import OFFSETS, catchments, levels
from pond_rims_model import depth_from_key

OUTLET_DTYPE = np.dtype([("pour_level", "<f8"), ("from_row", "<i4"), ("from_col", "<i4"), ("to_row", "<i4"), ("to_col", "<i4"),
                         ("to_basin", "<i4"), ("reserved", "<i4"), ("divide_cells", "<i8"), ("fill_cells", "<i8"), ("fill_q", "<u8")])
STATS = ("ponds", "no_outlet", "to_land", "divide_cells")


class TooDeep(Exception):
    """a fill term of 512 m or more, or one that is not finite"""


def passes(basin, key):
    """every pass of every pond: (pond, height key, flat padded index of a, direction) as four int arrays"""
    rows, ncp = basin.shape
    big = np.full((rows + 2, ncp + 2), -1, dtype=np.int64)
    big[1:-1, 1:-1] = basin
    bigkey = np.zeros((rows + 2, ncp + 2), dtype=np.uint64)
    bigkey[1:-1, 1:-1] = key
    cell = np.arange(rows * ncp, dtype=np.int64).reshape(rows, ncp)
    out = []
    for i, (dr, dc) in enumerate(OFFSETS):
        other = big[1 + dr:1 + dr + rows, 1 + dc:1 + dc + ncp]
        okey = bigkey[1 + dr:1 + dr + rows, 1 + dc:1 + dc + ncp]
        hit = (basin > 0) & (other >= 0) & (other != basin)
        out.append((basin[hit].astype(np.int64), np.maximum(key[hit], okey[hit]), cell[hit], np.full(int(hit.sum()), i, dtype=np.int64)))
    return tuple(np.concatenate([o[j] for o in out]) for j in range(4))


def outlets(labels, dem, w, pond_table, basin=None):
    labels = np.asarray(labels)
    dem = np.asarray(dem, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n = len(pond_table)
    rows, ncp = labels.shape
    if basin is None:
        basin, _, _ = catchments(labels, dem, w, pond_table)
    _, key = levels(labels, dem, w)
    table = np.zeros(n, dtype=OUTLET_DTYPE)
    table["pour_level"] = np.inf
    for name in ("from_row", "from_col", "to_row", "to_col", "to_basin"):
        table[name] = -1
    k, height, a, direction = passes(basin, key)
    pour = np.zeros(n, dtype=np.uint64)
    found = np.zeros(n, dtype=bool)
    if len(k):
        order = np.lexsort((direction, a, height, k))         # by pond, then height, then a, then neighbour order
        first = order[np.concatenate(([True], k[order][1:] != k[order][:-1]))]
        p = k[first] - 1
        found[p] = True
        pour[p] = height[first]
        table["pour_level"][p] = depth_from_key(height[first])
        off = np.array(OFFSETS, dtype=np.int64)[direction[first]]
        table["from_row"][p] = a[first] // ncp
        table["from_col"][p] = a[first] % ncp
        table["to_row"][p] = a[first] // ncp + off[:, 0]
        table["to_col"][p] = a[first] % ncp + off[:, 1]
        table["to_basin"][p] = basin[table["to_row"][p], table["to_col"][p]]
        divide = np.unique(k * (rows * ncp) + a) // (rows * ncp)      # distinct (pond, a) as one int64 each: below 2^62
        table["divide_cells"] = np.bincount(divide - 1, minlength=n)
    # the fill: cells of the basin strictly below the outlet
    inside = basin > 0
    kk = basin[inside].astype(np.int64) - 1
    below = found[kk] & (key[inside] < pour[kk])
    kk, lvl = kk[below], depth_from_key(key[inside][below])
    with np.errstate(invalid="ignore"):
        depth = depth_from_key(pour[kk]) - lvl                # one fp64 subtraction per cell
        if not (depth < 512.0).all():
            raise TooDeep(f"{int((~(depth < 512.0)).sum())} cells lie 512 m or more (or no finite depth) below their pond's outlet")
    table["fill_cells"] = np.bincount(kk, minlength=n)
    total = [0] * n
    for i, q in zip(kk.tolist(), np.rint(depth * 2.0 ** 24).astype(np.int64).tolist()):     # rint: half to even
        total[i] += q
    assert all(t < 2 ** 64 for t in total)
    table["fill_q"] = np.array(total, dtype=np.uint64) if n else 0
    stats = {"ponds": n, "no_outlet": int((~found).sum()), "to_land": int((found & (table["to_basin"] == 0)).sum()),
             "divide_cells": int(table["divide_cells"].sum())}
    return table, stats


def assert_invariants(table, rims):
    """the two statements of include/wdpm_pond_outlets.h that hold for every call"""
    has = table["from_row"] >= 0
    assert (table["pour_level"][has] >= rims["rim_level"][has]).all()
    assert (table["to_basin"][~has] == -1).all() and np.isposinf(table["pour_level"][~has]).all()
    assert (table["divide_cells"][~has] == 0).all() and (table["fill_cells"][~has] == 0).all() and (table["fill_q"][~has] == 0).all()
    assert (table["reserved"] == 0).all()
    j = table["to_basin"]
    to_pond = has & (j > 0)
    assert (j[to_pond] != np.flatnonzero(to_pond) + 1).all()
    assert has[j[to_pond] - 1].all() and (table["pour_level"][j[to_pond] - 1] <= table["pour_level"][to_pond]).all()


def assert_same_outlets(table, stats, ref_table, ref_stats):
    """the whole table and the counts: integers by value, doubles by bit pattern"""
    assert table.dtype == OUTLET_DTYPE and len(table) == len(ref_table), (table.dtype, len(table), len(ref_table))
    for name in OUTLET_DTYPE.names:
        a, b = np.ascontiguousarray(table[name]), np.ascontiguousarray(ref_table[name])
        same = a.view(np.uint64) == b.view(np.uint64) if a.dtype.kind == "f" else a == b
        assert same.all(), f"{name}: {int((~same).sum())} ponds differ, first pond {int(np.flatnonzero(~same)[0]) + 1}: {a[~same][0]!r} vs {b[~same][0]!r}"
    for name, v in ref_stats.items():
        assert stats[name] == v, (name, stats[name], v)
