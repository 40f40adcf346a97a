"""Host model of the pond rims (include/wdpm_pond_rims.h) in vectorised numpy - the yardstick of tests/test_pond_rims.py.

Eight shifted copies of the label raster give every (cell, neighbouring label) pair; np.unique makes each pair count once; sorting
and bincount do the rest.  Nothing here knows about segments, waves or masks.  Levels and surfaces are compared through the
order-preserving 64-bit image of a double (include/wdpm_pond_rims.h: -0.0 sorts below +0.0).

    table = rims(labels, dem, w, n)

labels: the label raster (padded, int32, 0 = no pond, 1..n); dem: the device DEM, padded, +inf on NODATA and on the border;
w: the water that was labelled.
"""
import numpy as np

RIM_DTYPE = np.dtype([("surface_min", "<f8"), ("surface_max", "<f8"), ("rim_level", "<f8"), ("rim_row", "<i4"), ("rim_col", "<i4"),
                      ("rim_cells", "<i8"), ("wall_cells", "<i8")])
SIGN = np.uint64(1 << 63)


def depth_key(v):
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | SIGN)


def depth_from_key(k):
    k = np.asarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & ~SIGN, ~k).astype(np.uint64).view(np.float64)


def device_dem(bd, miss):
    """what the device holds for a padded file DEM: +inf on NODATA (and on whatever does not compare above it) and on the border"""
    with np.errstate(invalid="ignore"):
        dem = np.where(bd > miss, bd, np.inf)
    dem[0, :] = dem[-1, :] = np.inf
    dem[:, 0] = dem[:, -1] = np.inf
    return dem


def rims(labels, dem, w, n):
    labels = np.asarray(labels)
    dem = np.asarray(dem, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    rows, ncp = labels.shape
    table = np.zeros(n, dtype=RIM_DTYPE)
    table["rim_level"] = np.inf
    table["rim_row"] = table["rim_col"] = -1
    if n == 0:
        return table
    with np.errstate(invalid="ignore"):
        surface = depth_key(dem + w)
        level = depth_key(np.where(w > 0, dem + w, dem))
        wall = ~(dem < np.inf)
    # the surface spread of every pond
    pond = labels > 0
    lab = labels[pond].astype(np.int64) - 1
    smin = np.full(n, np.iinfo(np.uint64).max, dtype=np.uint64)
    smax = np.zeros(n, dtype=np.uint64)
    np.minimum.at(smin, lab, surface[pond])
    np.maximum.at(smax, lab, surface[pond])
    table["surface_min"] = depth_from_key(smin)
    table["surface_max"] = depth_from_key(smax)
    # distinct (cell, label) pairs: a cell with label 0 and a neighbour of label k, once however many such neighbours it has
    big = np.zeros((rows + 2, ncp + 2), dtype=np.int64)
    big[1:-1, 1:-1] = labels
    cell = np.arange(rows * ncp, dtype=np.int64).reshape(rows, ncp)
    pairs = []
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            if dr == 1 and dc == 1:
                continue
            other = big[dr:dr + rows, dc:dc + ncp]
            hit = (other > 0) & ~pond
            pairs.append(cell[hit] * (n + 1) + other[hit])       # one int64 per pair: cells * (n + 1) < 2^62
    pairs = np.unique(np.concatenate(pairs))
    idx, k = pairs // (n + 1), pairs % (n + 1) - 1
    is_wall = wall.ravel()[idx]
    table["wall_cells"] = np.bincount(k[is_wall], minlength=n)
    idx, k = idx[~is_wall], k[~is_wall]
    table["rim_cells"] = np.bincount(k, minlength=n)
    if len(idx):
        key = level.ravel()[idx]
        order = np.lexsort((idx, key, k))            # by pond, then level, then padded index
        first = order[np.concatenate(([True], k[order][1:] != k[order][:-1]))]
        table["rim_level"][k[first]] = depth_from_key(key[first])
        table["rim_row"][k[first]] = idx[first] // ncp
        table["rim_col"][k[first]] = idx[first] % ncp
    return table


def assert_same_rims(table, ref):
    """the whole rim table: integers by value, doubles by bit pattern"""
    assert table.dtype == RIM_DTYPE and len(table) == len(ref), (table.dtype, len(table), len(ref))
    for name in RIM_DTYPE.names:
        a, b = np.ascontiguousarray(table[name]), np.ascontiguousarray(ref[name])
        same = a.view(np.uint64) == b.view(np.uint64) if a.dtype.kind == "f" else a == b
        assert same.all(), f"{name}: {int((~same).sum())} ponds differ, first pond {int(np.flatnonzero(~same)[0]) + 1}: {a[~same][0]!r} vs {b[~same][0]!r}"
