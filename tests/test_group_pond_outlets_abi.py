"""CPU-side checks of the boundary of the pond outlets over row blocks: include/wdpm_group_pond_outlets.h,
wdpm_amd.ponds.GROUP_OUTLET_SYMBOLS and the product library name the same four symbols under a prefix of their own, so that the seven
older dictionaries and the export lists the older ABI tests pin stay as they are; the stats struct is laid out as the binding says;
every entry point refuses null by name."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NAMES = ["wdpm_group_outlets_label", "wdpm_group_outlets_phase_ms", "wdpm_group_outlets_stats", "wdpm_group_outlets_table"]


def header():
    return open(os.path.join(ROOT, "include", "wdpm_group_pond_outlets.h")).read()


def test_header_binding_and_library_agree(hip):
    from wdpm_amd import capi, ponds
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(wdpm_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(ponds.GROUP_OUTLET_SYMBOLS) == NAMES
    out = subprocess.check_output(["nm", "-D", "--defined-only", hip.path], text=True)
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    assert sorted(n for n in exported if n.startswith("wdpm_group_outlets")) == names
    # a dictionary of its own: the seven older ones hold none of it, and they and their exports are what they were
    older = (ponds.SYMBOLS, ponds.RIM_SYMBOLS, ponds.GROUP_SYMBOLS, ponds.GROUP_RIM_SYMBOLS, ponds.CATCH_SYMBOLS, ponds.OUTLET_SYMBOLS,
             ponds.GROUP_CATCH_SYMBOLS)
    assert not any(set(ponds.GROUP_OUTLET_SYMBOLS) & set(d) for d in older + (capi.SYMBOLS,))
    assert [len(d) for d in older] == [8, 3, 9, 4, 5, 4, 5]
    prefixes = ("wdpm_ponds", "wdpm_rims", "wdpm_group_ponds", "wdpm_group_rims", "wdpm_catch", "wdpm_outlets", "wdpm_group_catch")
    for prefix, d in zip(prefixes, older):
        assert sorted(n for n in exported if n.startswith(prefix)) == sorted(d), prefix
    assert ponds._LABELLED_BY == {"table": "label", "rims": "label_rims", "catchments": "label_catchments", "outlets": "label_outlets"}
    dll = ponds.bind(hip)
    assert all(getattr(dll, n).argtypes == args for n, (_, args) in ponds.GROUP_OUTLET_SYMBOLS.items())
    assert '#include "wdpm_group_pond_catchments.h"' in header() and '#include "wdpm_pond_outlets.h"' in header()
    for method in ("label_outlets", "outlets", "outlet_stats", "outlet_phase_ms"):
        assert callable(getattr(ponds.GroupPonds, method))


def test_struct_layout_matches_the_header():
    from wdpm_amd import ponds
    body = re.search(r"typedef struct wdpm_group_outlet_stats \{(.*?)\} wdpm_group_outlet_stats;", header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int64_t|double)\s+(\w+);", body)
    kinds = {"int64_t": C.c_int64, "double": C.c_double}
    assert [(n, kinds[t]) for t, n in fields] == list(ponds.GroupOutletStatsStruct._fields_)
    assert C.sizeof(ponds.GroupOutletStatsStruct) == 8 * len(fields) == 64
    # the four counts of the whole-raster struct come first, in its order
    assert [n for _, n in fields][:4] == [n for n, _ in ponds.OutletStatsStruct._fields_]
    assert [n for _, n in fields][4:] == ["ranks", "seam_outlets", "split_ponds", "merge_ms"]


def test_every_entry_point_refuses_null_by_name(hip):
    from wdpm_amd import ponds
    dll = ponds.bind(hip)
    n, ms, st = C.c_int64(-1), (C.c_double * 2)(-1.0, -1.0), ponds.GroupOutletStatsStruct()
    calls = {
        "wdpm_group_outlets_label": lambda: dll.wdpm_group_outlets_label(None, 0.001, C.byref(n)),
        "wdpm_group_outlets_table": lambda: dll.wdpm_group_outlets_table(None, None, 0),
        "wdpm_group_outlets_stats": lambda: dll.wdpm_group_outlets_stats(None, C.byref(st)),
        "wdpm_group_outlets_phase_ms": lambda: dll.wdpm_group_outlets_phase_ms(None, 0, ms),
    }
    assert sorted(calls) == NAMES
    for name, call in calls.items():
        assert call() != 0, name
        assert name.encode() in dll.wdpm_last_error(), (name, dll.wdpm_last_error())
    assert n.value == -1 and list(ms) == [-1.0, -1.0]
