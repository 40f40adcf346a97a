"""ctypes binding of include/wdpm_ponds.h, include/wdpm_group_ponds.h, include/wdpm_pond_rims.h, include/wdpm_group_pond_rims.h,
include/wdpm_pond_catchments.h, include/wdpm_pond_outlets.h, include/wdpm_group_pond_catchments.h,
include/wdpm_group_pond_outlets.h, include/wdpm_pond_curves.h, include/wdpm_group_pond_curves.h, include/wdpm_pond_spills.h and
include/wdpm_pond_routing.h: the pond inventory of a context's current water raster, of a raster spread over the row blocks of a
rowblock.Group, the rim, the catchment, the outlet and the stage curve of every pond of either, where every pond of a whole raster
spills to, and what a runoff depth sent down that graph leaves in every pond.

Product library only (the symbols are not part of the ABI of include/wdpm.h, and ``capi.SYMBOLS`` does not list them).

    with hip.context(...) as ctx, Ponds(ctx) as ponds:
        n = ponds.label(0.001)
        table = ponds.table()       # structured array, one row per pond, numbered by first cell
        labels = ponds.labels()     # int32, padded layout like the water raster
        n = ponds.label_rims(0.001) # the same inventory, and one rim row per pond
        rims = ponds.rims()         # spill level and where it lies, shoreline, walls, surface spread (RIM_DTYPE)
        freeboard = rims["rim_level"] - rims["surface_max"]
        n = ponds.label_catchments(0.001)   # all of the above, and which pond every dry cell drains to
        basins = ponds.basins()     # int32, padded: k > 0 pond k or its catchment, 0 drains to a pit, -1 no level
        catch = ponds.catchments()  # contributing cells, inflow cells, head level, bounding box (CATCH_DTYPE)
        n = ponds.label_outlets(0.001)      # all of the above, and where every basin spills
        outlets = ponds.outlets()   # pour level, the pass (from, to, into which basin), divide, flooded cells, storage left (OUTLET_DTYPE)
        headroom = outlets["pour_level"] - rims["surface_max"]
        n = ponds.label_curves(0.001)       # all of the above, and every basin's flooded cells and storage at sixteen stages
        curves = ponds.curves()     # bed level, top level (the pour level), cells[16], q[16] (CURVE_DTYPE)
        levels = stage_levels(curves["bed_level"][0], curves["top_level"][0])   # the seventeen heights of pond 1, stage 0..16
        n = ponds.label_spills(0.001, headroom_tol=0.0)   # all of the above, and every pond's spill followed downstream
        spills = ponds.spills()     # next, sink, end, hops, storage on the way, what drains through it, what is connected now (SPILL_DTYPE)
        n = ponds.label_routing(0.001, runoff_m=0.010)    # all of the above, and 10 mm of runoff sent down the spill graph
        routing = ponds.routing()   # what each pond takes, keeps and passes on, and what is connected to it afterwards (ROUTE_DTYPE)
        ponds.route(0.025)          # another depth on the same graph: nothing is labelled again

    with rowblock.Group(...) as grp, GroupPonds(grp) as ponds:     # the same calls, the same answer, every rank labelled in place
        n = ponds.label(0.001)
        n = ponds.label_rims(0.001) # every rank takes the rims of its own rows; the host merges them
        rims = ponds.rims()         # RIM_DTYPE, coordinates of the whole raster
        n = ponds.label_catchments(0.001)   # and every rank's receivers, jump rounds and tally; the host ends the descents that
        basins = ponds.basins()     # cross row blocks and adds the ranks' tables up (CATCH_DTYPE, coordinates of the whole raster)
        n = ponds.label_outlets(0.001)      # and every rank's passes; the host makes the pour levels final between the two passes
        outlets = ponds.outlets()   # OUTLET_DTYPE, coordinates of the whole raster
        n = ponds.label_stage_curves(0.001) # and every rank's bed and stage passes; the host makes the beds final between the two
        curves = ponds.stage_curves()       # CURVE_DTYPE
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import capi

VOLUME_QUANTUM = 2.0 ** -24   # metres per unit of volume_q
PHASES = ("mask", "merge", "flatten", "scan", "table", "finish")   # wdpm_ponds_phase_ms
RIM_PHASES = ("rims", "locate")                                    # wdpm_rims_phase_ms
CATCH_PHASES = ("receivers", "jump", "tally")                      # wdpm_catch_phase_ms
OUTLET_PHASES = ("passes", "locate")                               # wdpm_outlets_phase_ms
CURVE_PHASES = ("bed", "stages")                                   # wdpm_curves_phase_ms
CURVE_STAGES = 16                                                  # WDPM_CURVE_STAGES
SPILL_PHASES = ("rings", "chains", "sums")                         # wdpm_spill_phase_ms
ROUTE_PHASES = ("order", "sweep", "finish")                        # wdpm_route_phase_ms


class PondStruct(C.Structure):
    """struct wdpm_pond"""
    _fields_ = [("first_row", C.c_int32), ("first_col", C.c_int32), ("cells", C.c_int64), ("volume_q", C.c_uint64),
                ("max_depth", C.c_double), ("row_min", C.c_int32), ("row_max", C.c_int32), ("col_min", C.c_int32),
                ("col_max", C.c_int32)]


class StatsStruct(C.Structure):
    """struct wdpm_pond_stats"""
    _fields_ = [("segments", C.c_int64), ("unions", C.c_int64), ("seam_unions", C.c_int64), ("passes", C.c_int64),
                ("rows_per_wave", C.c_int64), ("ponds", C.c_int64)]


POND_DTYPE = np.dtype([("first_row", "<i4"), ("first_col", "<i4"), ("cells", "<i8"), ("volume_q", "<u8"), ("max_depth", "<f8"),
                       ("row_min", "<i4"), ("row_max", "<i4"), ("col_min", "<i4"), ("col_max", "<i4")])
assert POND_DTYPE.itemsize == C.sizeof(PondStruct) == 48

_vp = C.c_void_p
# name -> (restype, argtypes); every symbol include/wdpm_ponds.h declares
SYMBOLS = {
    "wdpm_ponds_create": (C.c_int, [C.POINTER(_vp), _vp]),
    "wdpm_ponds_destroy": (None, [_vp]),
    "wdpm_ponds_label": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_ponds_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_ponds_labels": (C.c_int, [_vp, _vp]),
    "wdpm_ponds_guard_bad": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "wdpm_ponds_stats": (C.c_int, [_vp, C.POINTER(StatsStruct)]),
    "wdpm_ponds_phase_ms": (C.c_int, [_vp, C.POINTER(C.c_double)]),
}


class RimStruct(C.Structure):
    """struct wdpm_pond_rim"""
    _fields_ = [("surface_min", C.c_double), ("surface_max", C.c_double), ("rim_level", C.c_double), ("rim_row", C.c_int32),
                ("rim_col", C.c_int32), ("rim_cells", C.c_int64), ("wall_cells", C.c_int64)]


RIM_DTYPE = np.dtype([("surface_min", "<f8"), ("surface_max", "<f8"), ("rim_level", "<f8"), ("rim_row", "<i4"), ("rim_col", "<i4"),
                      ("rim_cells", "<i8"), ("wall_cells", "<i8")])
assert RIM_DTYPE.itemsize == C.sizeof(RimStruct) == 48

# every symbol include/wdpm_pond_rims.h declares
RIM_SYMBOLS = {
    "wdpm_rims_label": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_rims_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_rims_phase_ms": (C.c_int, [_vp, C.POINTER(C.c_double)]),
}


class CatchStruct(C.Structure):
    """struct wdpm_pond_catchment"""
    _fields_ = [("catch_cells", C.c_int64), ("inflow_cells", C.c_int64), ("head_level", C.c_double), ("row_min", C.c_int32),
                ("row_max", C.c_int32), ("col_min", C.c_int32), ("col_max", C.c_int32)]


class CatchStatsStruct(C.Structure):
    """struct wdpm_pond_catchment_stats"""
    _fields_ = [("slope_cells", C.c_int64), ("pit_cells", C.c_int64), ("unponded_cells", C.c_int64), ("rounds", C.c_int64),
                ("ponds", C.c_int64)]


CATCH_DTYPE = np.dtype([("catch_cells", "<i8"), ("inflow_cells", "<i8"), ("head_level", "<f8"), ("row_min", "<i4"),
                        ("row_max", "<i4"), ("col_min", "<i4"), ("col_max", "<i4")])
assert CATCH_DTYPE.itemsize == C.sizeof(CatchStruct) == 40

# every symbol include/wdpm_pond_catchments.h declares
CATCH_SYMBOLS = {
    "wdpm_catch_label": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_catch_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_catch_basins": (C.c_int, [_vp, _vp]),
    "wdpm_catch_stats": (C.c_int, [_vp, C.POINTER(CatchStatsStruct)]),
    "wdpm_catch_phase_ms": (C.c_int, [_vp, C.POINTER(C.c_double)]),
}


class OutletStruct(C.Structure):
    """struct wdpm_pond_outlet"""
    _fields_ = [("pour_level", C.c_double), ("from_row", C.c_int32), ("from_col", C.c_int32), ("to_row", C.c_int32),
                ("to_col", C.c_int32), ("to_basin", C.c_int32), ("reserved", C.c_int32), ("divide_cells", C.c_int64),
                ("fill_cells", C.c_int64), ("fill_q", C.c_uint64)]


class OutletStatsStruct(C.Structure):
    """struct wdpm_pond_outlet_stats"""
    _fields_ = [("ponds", C.c_int64), ("no_outlet", C.c_int64), ("to_land", C.c_int64), ("divide_cells", C.c_int64)]


OUTLET_DTYPE = np.dtype([("pour_level", "<f8"), ("from_row", "<i4"), ("from_col", "<i4"), ("to_row", "<i4"), ("to_col", "<i4"),
                         ("to_basin", "<i4"), ("reserved", "<i4"), ("divide_cells", "<i8"), ("fill_cells", "<i8"), ("fill_q", "<u8")])
assert OUTLET_DTYPE.itemsize == C.sizeof(OutletStruct) == 56

# every symbol include/wdpm_pond_outlets.h declares
OUTLET_SYMBOLS = {
    "wdpm_outlets_label": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_outlets_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_outlets_stats": (C.c_int, [_vp, C.POINTER(OutletStatsStruct)]),
    "wdpm_outlets_phase_ms": (C.c_int, [_vp, C.POINTER(C.c_double)]),
}


class CurveStruct(C.Structure):
    """struct wdpm_pond_curve"""
    _fields_ = [("bed_level", C.c_double), ("top_level", C.c_double), ("cells", C.c_int64 * CURVE_STAGES),
                ("q", C.c_uint64 * CURVE_STAGES)]


class CurveStatsStruct(C.Structure):
    """struct wdpm_pond_curve_stats"""
    _fields_ = [("ponds", C.c_int64), ("no_curve", C.c_int64), ("flat", C.c_int64), ("stage_cells", C.c_int64)]


CURVE_DTYPE = np.dtype([("bed_level", "<f8"), ("top_level", "<f8"), ("cells", "<i8", (CURVE_STAGES,)), ("q", "<u8", (CURVE_STAGES,))])
assert CURVE_DTYPE.itemsize == C.sizeof(CurveStruct) == 272 and C.sizeof(CurveStatsStruct) == 32

# every symbol include/wdpm_pond_curves.h declares
CURVE_SYMBOLS = {
    "wdpm_curves_label": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_curves_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_curves_stats": (C.c_int, [_vp, C.POINTER(CurveStatsStruct)]),
    "wdpm_curves_phase_ms": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "wdpm_curves_stage_level": (C.c_double, [C.c_double, C.c_double, C.c_int]),
}


class SpillStruct(C.Structure):
    """struct wdpm_pond_spill"""
    _fields_ = [("next", C.c_int32), ("sink", C.c_int32), ("end", C.c_int32), ("hops", C.c_int32), ("rest", C.c_int32),
                ("rest_hops", C.c_int32), ("spilling", C.c_int32), ("reserved", C.c_int32), ("path_fill_q", C.c_uint64),
                ("up_ponds", C.c_int64), ("up_cells", C.c_int64), ("up_fill_q", C.c_uint64), ("live_ponds", C.c_int64),
                ("live_cells", C.c_int64)]


class SpillStatsStruct(C.Structure):
    """struct wdpm_pond_spill_stats"""
    _fields_ = [("ponds", C.c_int64), ("rings", C.c_int64), ("ring_ponds", C.c_int64), ("spilling", C.c_int64), ("ends_land", C.c_int64),
                ("ends_none", C.c_int64), ("ends_ring", C.c_int64), ("max_hops", C.c_int64), ("rounds", C.c_int64)]


SPILL_DTYPE = np.dtype([("next", "<i4"), ("sink", "<i4"), ("end", "<i4"), ("hops", "<i4"), ("rest", "<i4"), ("rest_hops", "<i4"),
                        ("spilling", "<i4"), ("reserved", "<i4"), ("path_fill_q", "<u8"), ("up_ponds", "<i8"), ("up_cells", "<i8"),
                        ("up_fill_q", "<u8"), ("live_ponds", "<i8"), ("live_cells", "<i8")])
assert SPILL_DTYPE.itemsize == C.sizeof(SpillStruct) == 80 and C.sizeof(SpillStatsStruct) == 72

# every symbol include/wdpm_pond_spills.h declares
SPILL_SYMBOLS = {
    "wdpm_spill_label": (C.c_int, [_vp, C.c_double, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_spill_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_spill_stats": (C.c_int, [_vp, C.POINTER(SpillStatsStruct)]),
    "wdpm_spill_phase_ms": (C.c_int, [_vp, C.POINTER(C.c_double)]),
}


class RouteStruct(C.Structure):
    """struct wdpm_pond_route"""
    _fields_ = [("own_q", C.c_uint64), ("in_q", C.c_uint64), ("kept_q", C.c_uint64), ("out_q", C.c_uint64), ("reach_ponds", C.c_int64),
                ("reach_cells", C.c_int64), ("overflows", C.c_int32), ("full", C.c_int32), ("level", C.c_int32), ("reserved", C.c_int32)]


class RouteStatsStruct(C.Structure):
    """struct wdpm_pond_route_stats"""
    _fields_ = [("ponds", C.c_int64), ("runoff_q", C.c_int64), ("levels", C.c_int64), ("wide_levels", C.c_int64), ("launches", C.c_int64),
                ("overflowing", C.c_int64), ("full", C.c_int64), ("own_q", C.c_uint64), ("kept_q", C.c_uint64), ("out_land_q", C.c_uint64),
                ("out_ring_q", C.c_uint64)]


ROUTE_DTYPE = np.dtype([("own_q", "<u8"), ("in_q", "<u8"), ("kept_q", "<u8"), ("out_q", "<u8"), ("reach_ponds", "<i8"), ("reach_cells", "<i8"),
                        ("overflows", "<i4"), ("full", "<i4"), ("level", "<i4"), ("reserved", "<i4")])
assert ROUTE_DTYPE.itemsize == C.sizeof(RouteStruct) == 64 and C.sizeof(RouteStatsStruct) == 88

# every symbol include/wdpm_pond_routing.h declares
ROUTE_SYMBOLS = {
    "wdpm_route_label": (C.c_int, [_vp, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_route_rerun": (C.c_int, [_vp, C.c_double]),
    "wdpm_route_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_route_stats": (C.c_int, [_vp, C.POINTER(RouteStatsStruct)]),
    "wdpm_route_phase_ms": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "wdpm_route_runoff_q": (C.c_int64, [C.c_double]),
}


class GroupStatsStruct(C.Structure):
    """struct wdpm_group_pond_stats"""
    _fields_ = [("ranks", C.c_int64), ("ponds", C.c_int64), ("local_ponds", C.c_int64), ("stitch_unions", C.c_int64),
                ("merged", C.c_int64), ("stitch_ms", C.c_double)]


# every symbol include/wdpm_group_ponds.h declares
GROUP_SYMBOLS = {
    "wdpm_group_ponds_create": (C.c_int, [C.POINTER(_vp), _vp]),
    "wdpm_group_ponds_destroy": (None, [_vp]),
    "wdpm_group_ponds_label": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_group_ponds_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_group_ponds_labels": (C.c_int, [_vp, _vp]),
    "wdpm_group_ponds_guard_bad": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "wdpm_group_ponds_stats": (C.c_int, [_vp, C.POINTER(GroupStatsStruct)]),
    "wdpm_group_ponds_rank_stats": (C.c_int, [_vp, C.c_int32, C.POINTER(StatsStruct)]),
    "wdpm_group_ponds_phase_ms": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_double)]),
}


class GroupRimStatsStruct(C.Structure):
    """struct wdpm_group_rim_stats"""
    _fields_ = [("ranks", C.c_int64), ("slots", C.c_int64), ("foreign", C.c_int64), ("merge_ms", C.c_double)]


# every symbol include/wdpm_group_pond_rims.h declares
GROUP_RIM_SYMBOLS = {
    "wdpm_group_rims_label": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_group_rims_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_group_rims_stats": (C.c_int, [_vp, C.POINTER(GroupRimStatsStruct)]),
    "wdpm_group_rims_phase_ms": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_double)]),
}


class GroupCatchStatsStruct(C.Structure):
    """struct wdpm_group_catchment_stats"""
    _fields_ = [("slope_cells", C.c_int64), ("pit_cells", C.c_int64), ("unponded_cells", C.c_int64), ("rounds", C.c_int64),
                ("ponds", C.c_int64), ("ranks", C.c_int64), ("exits", C.c_int64), ("crossings", C.c_int64), ("remote", C.c_int64),
                ("resolve_ms", C.c_double)]


# every symbol include/wdpm_group_pond_catchments.h declares
GROUP_CATCH_SYMBOLS = {
    "wdpm_group_catch_label": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_group_catch_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_group_catch_basins": (C.c_int, [_vp, _vp]),
    "wdpm_group_catch_stats": (C.c_int, [_vp, C.POINTER(GroupCatchStatsStruct)]),
    "wdpm_group_catch_phase_ms": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_double)]),
}


class GroupOutletStatsStruct(C.Structure):
    """struct wdpm_group_outlet_stats"""
    _fields_ = [("ponds", C.c_int64), ("no_outlet", C.c_int64), ("to_land", C.c_int64), ("divide_cells", C.c_int64),
                ("ranks", C.c_int64), ("seam_outlets", C.c_int64), ("split_ponds", C.c_int64), ("merge_ms", C.c_double)]


# every symbol include/wdpm_group_pond_outlets.h declares
GROUP_OUTLET_SYMBOLS = {
    "wdpm_group_outlets_label": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_group_outlets_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_group_outlets_stats": (C.c_int, [_vp, C.POINTER(GroupOutletStatsStruct)]),
    "wdpm_group_outlets_phase_ms": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_double)]),
}


class GroupCurveStatsStruct(C.Structure):
    """struct wdpm_group_curve_stats"""
    _fields_ = [("ponds", C.c_int64), ("no_curve", C.c_int64), ("flat", C.c_int64), ("stage_cells", C.c_int64),
                ("ranks", C.c_int64), ("split_basins", C.c_int64), ("remote_beds", C.c_int64), ("merge_ms", C.c_double)]


# every symbol include/wdpm_group_pond_curves.h declares
GROUP_CURVE_SYMBOLS = {
    "wdpm_group_curves_label": (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int64)]),
    "wdpm_group_curves_table": (C.c_int, [_vp, _vp, C.c_int64]),
    "wdpm_group_curves_stats": (C.c_int, [_vp, C.POINTER(GroupCurveStatsStruct)]),
    "wdpm_group_curves_phase_ms": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_double)]),
}


def bind(lib: capi.Lib):
    """Set the prototypes on a loaded product library; a library without the symbols is an error (no fallback)."""
    if getattr(lib, "_ponds_bound", False):
        return lib.dll
    for name, (res, args) in list(SYMBOLS.items()) + list(GROUP_SYMBOLS.items()) + list(RIM_SYMBOLS.items()) + \
            list(GROUP_RIM_SYMBOLS.items()) + list(CATCH_SYMBOLS.items()) + list(OUTLET_SYMBOLS.items()) + list(GROUP_CATCH_SYMBOLS.items()) + \
            list(GROUP_OUTLET_SYMBOLS.items()) + list(CURVE_SYMBOLS.items()) + list(GROUP_CURVE_SYMBOLS.items()) + list(SPILL_SYMBOLS.items()) + \
            list(ROUTE_SYMBOLS.items()):
        try:
            fn = getattr(lib.dll, name)
        except AttributeError:
            raise capi.WdpmError(f"{lib.path} does not export {name}: the pond inventory needs the HIP product library") from None
        fn.restype = res
        fn.argtypes = args
    lib._ponds_bound = True
    return lib.dll


# the call a table method reads
_LABELLED_BY = {"table": "label", "rims": "label_rims", "catchments": "label_catchments", "outlets": "label_outlets"}


class _Handle:
    """What Ponds and GroupPonds share: a C handle made on an owner (a Context, a Group) and destroyed before it, and the four
    shapes of call the headers repeat."""

    def __init__(self, owner, create: str, destroy: str):
        self.lib = owner.lib
        self.dll = bind(owner.lib)
        self.shape = owner.shape
        self.n = None
        self._h = None
        self._destroy = destroy
        h = C.c_void_p()
        self.lib.check(getattr(self.dll, create)(C.byref(h), owner._h))
        self._h = h
        deps = getattr(owner, "_dependents", None)
        if deps is not None:
            deps.append(weakref.ref(self))

    def close(self):
        if self._h:
            getattr(self.dll, self._destroy)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _label(self, fn, min_depth) -> int:
        n = C.c_int64()
        self.n = None
        self.lib.check(fn(self._h, float(min_depth), C.byref(n)))
        self.n = n.value
        return n.value

    def _table(self, fn, dtype, method, capacity, labelled_by=None) -> np.ndarray:
        if self.n is None:
            raise capi.WdpmError(f"{type(self).__name__}.{method}: {labelled_by or _LABELLED_BY[method]}() has not succeeded on this handle")
        cap = self.n if capacity is None else int(capacity)
        out = np.zeros(max(cap, 0), dtype=dtype)
        self.lib.check(fn(self._h, out.ctypes.data, cap))
        return out[:self.n]

    def _stats(self, fn, struct, *lead) -> dict:
        s = struct()
        self.lib.check(fn(self._h, *lead, C.byref(s)))
        return {name: (float if ctype is C.c_double else int)(getattr(s, name)) for name, ctype in struct._fields_}

    def _phase_ms(self, fn, names, *lead) -> dict:
        ms = (C.c_double * len(names))()
        self.lib.check(fn(self._h, *lead, ms))
        return dict(zip(names, (float(v) for v in ms)))


class Ponds(_Handle):
    """The inventory handle of one whole-raster context — wraps wdpm_ponds.  The C handle must go before its context: the
    object keeps its Context alive, and a Context that is closed first closes the handles that live on it."""

    def __init__(self, ctx: capi.Context):
        self.ctx = ctx
        super().__init__(ctx, "wdpm_ponds_create", "wdpm_ponds_destroy")

    def label(self, min_depth: float) -> int:
        """Label the ponds deeper than min_depth (metres, strict) on the context's current water; returns their number."""
        return self._label(self.dll.wdpm_ponds_label, min_depth)

    def table(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (POND_DTYPE).  `capacity` is what the C call is told the buffer holds (default: exactly N)."""
        return self._table(self.dll.wdpm_ponds_table, POND_DTYPE, "table", capacity)

    def labels(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.int32)
        self.lib.check(self.dll.wdpm_ponds_labels(self._h, out.ctypes.data))
        return out

    def stats(self) -> dict:
        return self._stats(self.dll.wdpm_ponds_stats, StatsStruct)

    def phase_ms(self) -> dict:
        """milliseconds per kernel phase of the last label call (handles made with WDPM_PONDS_TIMING=1 in the environment)"""
        return self._phase_ms(self.dll.wdpm_ponds_phase_ms, PHASES)

    def guard_bad(self) -> int:
        v = C.c_int64()
        self.lib.check(self.dll.wdpm_ponds_guard_bad(self._h, C.byref(v)))
        return v.value

    def label_rims(self, min_depth: float) -> int:
        """label(min_depth), then the rim pass on the same water; table(), labels() and stats() answer as after label()."""
        return self._label(self.dll.wdpm_rims_label, min_depth)

    def rims(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (RIM_DTYPE) of the last label_rims(); fails after a plain label().  Coordinates are padded, -1 where a
        pond has no rim cell; freeboard is rim_level - surface_max."""
        return self._table(self.dll.wdpm_rims_table, RIM_DTYPE, "rims", capacity)

    def rims_phase_ms(self) -> dict:
        """milliseconds of the rim pass and of the locate pass of the last label_rims() (handles made with WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_rims_phase_ms, RIM_PHASES)

    def label_catchments(self, min_depth: float) -> int:
        """label_rims(min_depth), then the catchment pass on the same water; table(), labels(), stats() and rims() answer as
        after label_rims()."""
        return self._label(self.dll.wdpm_catch_label, min_depth)

    def catchments(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (CATCH_DTYPE) of the last label_catchments(); fails after label() or label_rims().  The box is padded
        and holds the pond and its catchment; head_level is -inf where no cell drains to the pond."""
        return self._table(self.dll.wdpm_catch_table, CATCH_DTYPE, "catchments", capacity)

    def basins(self) -> np.ndarray:
        """int32, padded like labels(): k > 0 for pond k and the cells that drain to it, 0 for cells that drain to a pit, -1 for
        cells without a level (border, NODATA)"""
        out = np.empty(self.shape, dtype=np.int32)
        self.lib.check(self.dll.wdpm_catch_basins(self._h, out.ctypes.data))
        return out

    def catchment_stats(self) -> dict:
        return self._stats(self.dll.wdpm_catch_stats, CatchStatsStruct)

    def catchment_phase_ms(self) -> dict:
        """milliseconds of the receiver pass, the jump rounds and the tally of the last label_catchments() (handles made with
        WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_catch_phase_ms, CATCH_PHASES)

    def label_outlets(self, min_depth: float) -> int:
        """label_catchments(min_depth), then the outlet pass on the same water; table(), labels(), stats(), rims(), basins() and
        catchments() answer as after label_catchments()."""
        return self._label(self.dll.wdpm_outlets_label, min_depth)

    def outlets(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (OUTLET_DTYPE) of the last label_outlets(); fails after any lesser label call.  Coordinates are padded;
        a pond whose basin meets no other has pour_level +inf, coordinates -1, to_basin -1 and zeros.  fill_q counts in
        VOLUME_QUANTUM metres, like volume_q."""
        return self._table(self.dll.wdpm_outlets_table, OUTLET_DTYPE, "outlets", capacity)

    def outlet_stats(self) -> dict:
        return self._stats(self.dll.wdpm_outlets_stats, OutletStatsStruct)

    def outlet_phase_ms(self) -> dict:
        """milliseconds of the pass over the pairs and of the locate pass of the last label_outlets() (handles made with
        WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_outlets_phase_ms, OUTLET_PHASES)

    def label_curves(self, min_depth: float) -> int:
        """label_outlets(min_depth), then the curve pass on the same water; every older query answers as after label_outlets()."""
        return self._label(self.dll.wdpm_curves_label, min_depth)

    def curves(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (CURVE_DTYPE) of the last label_curves(); fails after any lesser label call.  cells[s - 1] and q[s - 1]
        are the cells of the pond's basin whose ground lies strictly below stage s of stage_levels(bed_level, top_level) and their
        depths below it in VOLUME_QUANTUM metres; a pond without an outlet has top_level +inf and zeros."""
        return self._table(self.dll.wdpm_curves_table, CURVE_DTYPE, "curves", capacity, labelled_by="label_curves")

    def curve_stats(self) -> dict:
        return self._stats(self.dll.wdpm_curves_stats, CurveStatsStruct)

    def curve_phase_ms(self) -> dict:
        """milliseconds of the bed pass and of the stage pass of the last label_curves() (handles made with WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_curves_phase_ms, CURVE_PHASES)

    def label_spills(self, min_depth: float, headroom_tol: float = 0.0) -> int:
        """label_curves(min_depth), then the spill pass on the tables it left; every older query answers as after label_curves().
        A pond is spilling when it has an outlet and pour_level - surface_max <= headroom_tol (metres, finite, >= 0)."""
        n = C.c_int64()
        self.n = None
        self.lib.check(self.dll.wdpm_spill_label(self._h, float(min_depth), float(headroom_tol), C.byref(n)))
        self.n = n.value
        return n.value

    def spills(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (SPILL_DTYPE) of the last label_spills(); fails after any lesser label call.  next / sink / rest are
        labels (next 0: land that ends in a pit, -1: no outlet, -2: a ring of ponds closed here); path_fill_q and up_fill_q count
        in VOLUME_QUANTUM metres; up_* is what drains through the pond once everything above it is full, live_* what is
        connected to it now."""
        return self._table(self.dll.wdpm_spill_table, SPILL_DTYPE, "spills", capacity, labelled_by="label_spills")

    def spill_stats(self) -> dict:
        return self._stats(self.dll.wdpm_spill_stats, SpillStatsStruct)

    def spill_phase_ms(self) -> dict:
        """milliseconds of the ring pass, the chain pass and the sums of the last label_spills() (handles made with
        WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_spill_phase_ms, SPILL_PHASES)

    def label_routing(self, min_depth: float, runoff_m: float, headroom_tol: float = 0.0) -> int:
        """label_spills(min_depth, headroom_tol), then runoff_m metres of runoff on every basin sent down the spill graph; every
        older query, spills() included, answers as after label_spills().  runoff_m is finite, >= 0 and below 256 m."""
        n = C.c_int64()
        self.n = None
        self.lib.check(self.dll.wdpm_route_label(self._h, float(min_depth), float(headroom_tol), float(runoff_m), C.byref(n)))
        self.n = n.value
        return n.value

    def route(self, runoff_m: float) -> None:
        """another runoff depth on the graph of the last label_routing(): sweep and finish only, nothing is labelled again; fails
        after any lesser label call"""
        self.lib.check(self.dll.wdpm_route_rerun(self._h, float(runoff_m)))

    def routing(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (ROUTE_DTYPE) of the last label_routing() or route(): own_q, in_q, kept_q and out_q count in
        VOLUME_QUANTUM metres times cells; reach_* is what is connected to the pond after the event."""
        return self._table(self.dll.wdpm_route_table, ROUTE_DTYPE, "routing", capacity, labelled_by="label_routing")

    def routing_stats(self) -> dict:
        return self._stats(self.dll.wdpm_route_stats, RouteStatsStruct)

    def routing_phase_ms(self) -> dict:
        """milliseconds of the ordering by level (0 after route()), of the sweep and of the finish of the last label_routing() or
        route() (handles made with WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_route_phase_ms, ROUTE_PHASES)


def stage_levels(bed: float, top: float, lib: capi.Lib | None = None) -> np.ndarray:
    """The seventeen stage heights 0..16 of a curve row, from the library's own wdpm_curves_stage_level (`lib`: a loaded product
    library; default the one load_hip() finds).  Stage 0 is the bed, stage 16 the top; with top +inf there is no curve and
    everything past the bed is not finite."""
    dll = bind(capi.load_hip() if lib is None else lib)
    return np.array([dll.wdpm_curves_stage_level(float(bed), float(top), s) for s in range(CURVE_STAGES + 1)], dtype=np.float64)


def runoff_q(runoff_m: float, lib: capi.Lib | None = None) -> int:
    """The quanta of 2^-24 m a routing call makes of runoff_m, from the library's own wdpm_route_runoff_q; -1 where the call would
    refuse the depth."""
    dll = bind(capi.load_hip() if lib is None else lib)
    return int(dll.wdpm_route_runoff_q(float(runoff_m)))


class GroupPonds(_Handle):
    """The inventory handle of a rowblock.Group - wraps wdpm_group_ponds.  Labels the water Group.download_water returns, every
    rank's rows where they lie, and answers as Ponds does on a whole-raster context holding the same water.  The C handle must
    go before its group: the object keeps its Group alive, and a Group that is closed first closes the handles that live on it."""

    def __init__(self, group):
        self.group = group
        super().__init__(group, "wdpm_group_ponds_create", "wdpm_group_ponds_destroy")
        self.ranks = group.size

    def label(self, min_depth: float) -> int:
        """Label the ponds deeper than min_depth (metres, strict) on the group's current water; returns their number."""
        return self._label(self.dll.wdpm_group_ponds_label, min_depth)

    def table(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (POND_DTYPE), coordinates of the whole raster."""
        return self._table(self.dll.wdpm_group_ponds_table, POND_DTYPE, "table", capacity)

    def labels(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.int32)
        self.lib.check(self.dll.wdpm_group_ponds_labels(self._h, out.ctypes.data))
        return out

    def stats(self) -> dict:
        return self._stats(self.dll.wdpm_group_ponds_stats, GroupStatsStruct)

    def rank_stats(self, rank: int) -> dict:
        """what Ponds.stats says, of one rank's own labelling"""
        return self._stats(self.dll.wdpm_group_ponds_rank_stats, StatsStruct, int(rank))

    def phase_ms(self, rank: int) -> dict:
        """milliseconds per kernel phase of one rank in the last label call (handles made with WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_group_ponds_phase_ms, PHASES, int(rank))

    def guard_bad(self) -> int:
        v = C.c_int64()
        self.lib.check(self.dll.wdpm_group_ponds_guard_bad(self._h, C.byref(v)))
        return v.value

    def label_rims(self, min_depth: float) -> int:
        """label(min_depth), and every rank's rim pass on the same water; table(), labels(), stats() and rank_stats() answer as
        after label()."""
        return self._label(self.dll.wdpm_group_rims_label, min_depth)

    def rims(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (RIM_DTYPE) of the last label_rims(), coordinates of the whole raster; fails after a plain label()."""
        return self._table(self.dll.wdpm_group_rims_table, RIM_DTYPE, "rims", capacity)

    def rims_stats(self) -> dict:
        return self._stats(self.dll.wdpm_group_rims_stats, GroupRimStatsStruct)

    def rims_phase_ms(self, rank: int) -> dict:
        """milliseconds of one rank's rim pass and locate pass in the last label_rims() (handles made with WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_group_rims_phase_ms, RIM_PHASES, int(rank))

    def label_catchments(self, min_depth: float) -> int:
        """label_rims(min_depth), and every rank's catchment pass on the same water; table(), labels(), stats(), rank_stats() and
        rims() answer as after label_rims()."""
        return self._label(self.dll.wdpm_group_catch_label, min_depth)

    def catchments(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (CATCH_DTYPE) of the last label_catchments(), coordinates of the whole raster; fails after label() or
        label_rims()."""
        return self._table(self.dll.wdpm_group_catch_table, CATCH_DTYPE, "catchments", capacity)

    def basins(self) -> np.ndarray:
        """int32, padded like labels(), every rank's owned rows where they lie: k > 0 for pond k and the cells that drain to it,
        0 for cells that drain to a pit, -1 for cells without a level"""
        out = np.empty(self.shape, dtype=np.int32)
        self.lib.check(self.dll.wdpm_group_catch_basins(self._h, out.ctypes.data))
        return out

    def catchment_stats(self) -> dict:
        """the counts of Ponds.catchment_stats for the whole raster, then ranks, exits, crossings, remote and resolve_ms"""
        return self._stats(self.dll.wdpm_group_catch_stats, GroupCatchStatsStruct)

    def catchment_phase_ms(self, rank: int) -> dict:
        """milliseconds of one rank's receiver pass, jump rounds and tally in the last label_catchments() (handles made with
        WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_group_catch_phase_ms, CATCH_PHASES, int(rank))

    def label_outlets(self, min_depth: float) -> int:
        """label_catchments(min_depth), and every rank's outlet pass on the same water; every older query answers as after
        label_catchments()."""
        return self._label(self.dll.wdpm_group_outlets_label, min_depth)

    def outlets(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (OUTLET_DTYPE) of the last label_outlets(), coordinates of the whole raster; fails after any lesser
        label call."""
        return self._table(self.dll.wdpm_group_outlets_table, OUTLET_DTYPE, "outlets", capacity)

    def outlet_stats(self) -> dict:
        """the counts of Ponds.outlet_stats for the whole raster, then ranks, seam_outlets, split_ponds and merge_ms"""
        return self._stats(self.dll.wdpm_group_outlets_stats, GroupOutletStatsStruct)

    def outlet_phase_ms(self, rank: int) -> dict:
        """milliseconds of one rank's pass over the pairs and of its locate pass in the last label_outlets() (handles made with
        WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_group_outlets_phase_ms, OUTLET_PHASES, int(rank))

    def label_stage_curves(self, min_depth: float) -> int:
        """label_outlets(min_depth), and every rank's bed pass and stage pass on the same water; every older query answers as after
        label_outlets()."""
        return self._label(self.dll.wdpm_group_curves_label, min_depth)

    def stage_curves(self, capacity: int | None = None) -> np.ndarray:
        """One row per pond (CURVE_DTYPE) of the last label_stage_curves(), as Ponds.curves() gives it on a whole-raster context
        holding the same water; fails after any lesser label call."""
        return self._table(self.dll.wdpm_group_curves_table, CURVE_DTYPE, "stage_curves", capacity, labelled_by="label_stage_curves")

    def stage_curve_stats(self) -> dict:
        """the counts of Ponds.curve_stats for the whole raster, then ranks, split_basins, remote_beds and merge_ms"""
        return self._stats(self.dll.wdpm_group_curves_stats, GroupCurveStatsStruct)

    def stage_curve_phase_ms(self, rank: int) -> dict:
        """milliseconds of one rank's bed pass and of its stage pass in the last label_stage_curves() (handles made with
        WDPM_PONDS_TIMING=1)"""
        return self._phase_ms(self.dll.wdpm_group_curves_phase_ms, CURVE_PHASES, int(rank))
