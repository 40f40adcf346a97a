"""Host model of the pond stage curves (include/wdpm_pond_curves.h) in numpy - the yardstick of tests/test_pond_curves.py.

The basin raster comes from tests/pond_catchments_model.py and the pour levels from tests/pond_outlets_model.py.  The bed is one
np.minimum.at over the keys of the DEM; the stage heights are computed here on their own, three rounded numpy operations each (numpy
never fuses a multiplication into an addition); every stage is one masked pass over the cells of all basins; the sums are Python
integers.  Nothing here knows about segments, waves, strips, carries or skipped rows.

    table, stats = curves(basin, dem, outlet_table)                 # raises TooDeep where the call must fail

basin: the basin raster (padded, int32: k > 0 pond k or its catchment); dem: the device DEM, padded, +inf on NODATA and on the border
(pond_rims_model.device_dem); outlet_table: the outlet table of the same call (its pour_level is the top).
"""
import numpy as np

from pond_rims_model import depth_from_key, depth_key

STAGES = 16
CURVE_DTYPE = np.dtype([("bed_level", "<f8"), ("top_level", "<f8"), ("cells", "<i8", (STAGES,)), ("q", "<u8", (STAGES,))])
STATS = ("ponds", "no_curve", "flat", "stage_cells")
NO_KEY = np.uint64(2 ** 64 - 1)


class TooDeep(Exception):
    """a term of q of 512 m or more, or one that is not finite"""


def stage_levels(bed, top):
    """the seventeen heights 0..16 for arrays of beds and finite tops, shape (17, n): stage 0 the bed, stage 16 the top itself"""
    bed = np.atleast_1d(np.asarray(bed, dtype=np.float64))
    top = np.atleast_1d(np.asarray(top, dtype=np.float64))
    h = np.empty((STAGES + 1, len(bed)))
    h[0], h[STAGES] = bed, top
    with np.errstate(invalid="ignore", over="ignore"):
        span = top - bed                                      # one subtraction
        for s in range(1, STAGES):
            part = span * np.float64(s / 16.0)                # one multiplication by the exact s / 16
            h[s] = bed + part                                 # one addition
    return h


def curves(basin, dem, outlet_table):
    basin = np.asarray(basin)
    dem = np.asarray(dem, dtype=np.float64)
    n = len(outlet_table)
    table = np.zeros(n, dtype=CURVE_DTYPE)
    inside = basin > 0
    kk = basin[inside].astype(np.int64) - 1
    e = dem[inside]
    ekey = depth_key(e)
    bedkey = np.full(n, NO_KEY, dtype=np.uint64)
    np.minimum.at(bedkey, kk, ekey)
    assert (bedkey != NO_KEY).all()                           # every pond has its own cells in its basin
    table["bed_level"] = depth_from_key(bedkey) if n else 0
    table["top_level"] = outlet_table["pour_level"]
    has = np.isfinite(table["top_level"])
    h = stage_levels(table["bed_level"], np.where(has, table["top_level"], 0.0)) if n else np.zeros((STAGES + 1, 0))
    for s in range(1, STAGES + 1):
        below = has[kk] & (ekey < depth_key(h[s])[kk])
        ks = kk[below]
        with np.errstate(invalid="ignore", over="ignore"):
            depth = h[s][ks] - e[below]                       # one fp64 subtraction per cell and stage
        if not (depth < 512.0).all():
            raise TooDeep(f"stage {s}: {int((~(depth < 512.0)).sum())} cells lie 512 m or more (or no finite depth) below it")
        table["cells"][:, s - 1] = np.bincount(ks, minlength=n)
        total = [0] * n
        for i, q in zip(ks.tolist(), np.rint(depth * 2.0 ** 24).astype(np.int64).tolist()):     # rint: half to even
            total[i] += q
        assert all(t < 2 ** 64 for t in total)
        table["q"][:, s - 1] = np.array(total, dtype=np.uint64) if n else 0
    stats = {"ponds": n, "no_curve": int((~has).sum()), "flat": int((table["top_level"] == table["bed_level"]).sum()),
             "stage_cells": int(table["cells"][:, STAGES - 1].sum()) if n else 0}
    return table, stats


def assert_invariants(table, outlet_table):
    """what include/wdpm_pond_curves.h states of every call"""
    has = np.isfinite(table["top_level"])
    assert (table["top_level"].view(np.uint64) == outlet_table["pour_level"].view(np.uint64)).all()
    assert np.isposinf(table["top_level"][~has]).all() and np.isfinite(table["bed_level"]).all()
    assert (table["cells"][~has] == 0).all() and (table["q"][~has] == 0).all()
    flat = table["top_level"] == table["bed_level"]
    assert (table["cells"][flat] == 0).all() and (table["q"][flat] == 0).all()
    if has.any():
        h = stage_levels(table["bed_level"][has], table["top_level"][has])
        assert (np.diff(h, axis=0) >= 0).all() and (h <= table["top_level"][has]).all()
    assert (np.diff(table["cells"], axis=1) >= 0).all() and (table["cells"] >= 0).all()
    assert (np.diff(table["q"].astype(object), axis=1) >= 0).all()
    assert (table["cells"][:, STAGES - 1] >= outlet_table["fill_cells"]).all()
    assert (table["q"][:, STAGES - 1] >= outlet_table["fill_q"]).all()


def assert_same_curves(table, stats, ref_table, ref_stats):
    """the whole table and the counts: integers by value, doubles by bit pattern"""
    assert table.dtype == CURVE_DTYPE and len(table) == len(ref_table), (table.dtype, len(table), len(ref_table))
    for name in CURVE_DTYPE.names:
        a, b = np.ascontiguousarray(table[name]), np.ascontiguousarray(ref_table[name])
        same = a.view(np.uint64) == b.view(np.uint64) if a.dtype.kind == "f" else a == b
        if same.ndim > 1:
            same = same.all(axis=1)
        assert same.all(), f"{name}: {int((~same).sum())} ponds differ, first pond {int(np.flatnonzero(~same)[0]) + 1}: {a[~same][0]!r} vs {b[~same][0]!r}"
    for name, v in ref_stats.items():
        assert stats[name] == v, (name, stats[name], v)
