"""CPU-side checks of the boundary of the pond stage curves over row blocks: include/wdpm_group_pond_curves.h,
wdpm_amd.ponds.GROUP_CURVE_SYMBOLS and the product library name the same four symbols under a prefix of their own, so that the nine
older dictionaries and the export lists the older ABI tests pin stay as they are; the stats struct is laid out as the binding says;
every entry point refuses null by name and writes nothing.

A handle needs a device, so what wdpm_group_curves_table says on a handle whose last label call was label_outlets is asked in
tests/test_group_pond_curves.py (test_handle_states); the sentence itself is pinned here, from the library's own text."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NAMES = ["wdpm_group_curves_label", "wdpm_group_curves_phase_ms", "wdpm_group_curves_stats", "wdpm_group_curves_table"]


def header():
    return open(os.path.join(ROOT, "include", "wdpm_group_pond_curves.h")).read()


def test_header_binding_and_library_agree(hip):
    from wdpm_amd import capi, ponds
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(wdpm_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(ponds.GROUP_CURVE_SYMBOLS) == NAMES
    out = subprocess.check_output(["nm", "-D", "--defined-only", hip.path], text=True)
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    assert sorted(n for n in exported if n.startswith("wdpm_group_curves")) == names
    # a dictionary of its own: the nine older ones hold none of it, and they and their exports are what they were
    older = (ponds.SYMBOLS, ponds.RIM_SYMBOLS, ponds.GROUP_SYMBOLS, ponds.GROUP_RIM_SYMBOLS, ponds.CATCH_SYMBOLS, ponds.OUTLET_SYMBOLS,
             ponds.GROUP_CATCH_SYMBOLS, ponds.GROUP_OUTLET_SYMBOLS, ponds.CURVE_SYMBOLS)
    assert not any(set(ponds.GROUP_CURVE_SYMBOLS) & set(d) for d in older + (capi.SYMBOLS,))
    assert [len(d) for d in older] == [8, 3, 9, 4, 5, 4, 5, 4, 5]
    prefixes = ("wdpm_ponds", "wdpm_rims", "wdpm_group_ponds", "wdpm_group_rims", "wdpm_catch", "wdpm_outlets", "wdpm_group_catch",
                "wdpm_group_outlets", "wdpm_curves")
    for prefix, d in zip(prefixes, older):
        assert sorted(n for n in exported if n.startswith(prefix)) == sorted(d), prefix
    assert ponds._LABELLED_BY == {"table": "label", "rims": "label_rims", "catchments": "label_catchments", "outlets": "label_outlets"}
    dll = ponds.bind(hip)
    assert all(getattr(dll, n).argtypes == args and getattr(dll, n).restype == res for n, (res, args) in ponds.GROUP_CURVE_SYMBOLS.items())
    assert '#include "wdpm_group_pond_outlets.h"' in header() and '#include "wdpm_pond_curves.h"' in header()
    for method in ("label_stage_curves", "stage_curves", "stage_curve_stats", "stage_curve_phase_ms"):
        assert callable(getattr(ponds.GroupPonds, method))
    assert not any(hasattr(ponds.GroupPonds, m) for m in ("label_curves", "curves", "curve_stats", "curve_phase_ms"))
    assert not any(hasattr(ponds.Ponds, m) for m in ("label_stage_curves", "stage_curves", "stage_curve_stats", "stage_curve_phase_ms"))


def test_struct_layout_matches_the_header():
    from wdpm_amd import ponds
    body = re.search(r"typedef struct wdpm_group_curve_stats \{(.*?)\} wdpm_group_curve_stats;", header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int64_t|double)\s+(\w+);", body)
    kinds = {"int64_t": C.c_int64, "double": C.c_double}
    assert [(n, kinds[t]) for t, n in fields] == list(ponds.GroupCurveStatsStruct._fields_)
    assert C.sizeof(ponds.GroupCurveStatsStruct) == 8 * len(fields) == 64
    assert [getattr(ponds.GroupCurveStatsStruct, n).offset for _, n in fields] == list(range(0, 64, 8))
    # the four counts of the whole-raster struct come first, in its order
    assert [n for _, n in fields][:4] == [n for n, _ in ponds.CurveStatsStruct._fields_]
    assert [(t, n) for t, n in fields][4:] == [("int64_t", "ranks"), ("int64_t", "split_basins"), ("int64_t", "remote_beds"), ("double", "merge_ms")]
    # the table row is that of the whole-raster header: this one declares no row of its own
    assert "typedef struct wdpm_pond_curve " not in header() and ponds.CURVE_DTYPE.itemsize == 272


def test_every_entry_point_refuses_null_by_name_and_writes_nothing(hip):
    from wdpm_amd import ponds
    dll = ponds.bind(hip)
    n, ms = C.c_int64(-1), (C.c_double * 2)(-1.0, -1.0)
    st = ponds.GroupCurveStatsStruct(-1, -1, -1, -1, -1, -1, -1, -1.0)
    row = (C.c_uint64 * 34)(*([7] * 34))
    calls = {
        "wdpm_group_curves_label": lambda: dll.wdpm_group_curves_label(None, 0.001, C.byref(n)),
        "wdpm_group_curves_table": lambda: dll.wdpm_group_curves_table(None, row, 1),
        "wdpm_group_curves_stats": lambda: dll.wdpm_group_curves_stats(None, C.byref(st)),
        "wdpm_group_curves_phase_ms": lambda: dll.wdpm_group_curves_phase_ms(None, 0, ms),
    }
    assert sorted(calls) == NAMES
    for name, call in calls.items():
        assert call() != 0, name
        assert name.encode() in dll.wdpm_last_error(), (name, dll.wdpm_last_error())
    assert n.value == -1 and list(ms) == [-1.0, -1.0] and list(row) == [7] * 34
    assert [getattr(st, f) for f, _ in st._fields_] == [-1] * 7 + [-1.0]


def test_the_sentence_for_a_handle_without_a_curve_table_names_the_call(hip):
    """what wdpm_group_curves_table, _stats and _phase_ms answer after a lesser label call, as the library holds it"""
    text = open(hip.path, "rb").read()
    assert b"no curve table: the last label call on this handle was not a wdpm_group_curves_label that succeeded" in text
