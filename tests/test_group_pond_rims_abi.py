"""CPU-side checks of the boundary of the pond rims over row blocks: include/wdpm_group_pond_rims.h, wdpm_amd.ponds.GROUP_RIM_SYMBOLS
and the product library name the same four symbols under a prefix of their own, so that the export lists the three older ABI tests
pin stay as they are; the stats struct is laid out as the binding says; every entry point refuses null by name."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NAMES = ["wdpm_group_rims_label", "wdpm_group_rims_phase_ms", "wdpm_group_rims_stats", "wdpm_group_rims_table"]


def header():
    return open(os.path.join(ROOT, "include", "wdpm_group_pond_rims.h")).read()


def test_header_binding_and_library_agree(hip):
    from wdpm_amd import capi, ponds
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(wdpm_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(ponds.GROUP_RIM_SYMBOLS) == NAMES
    out = subprocess.check_output(["nm", "-D", "--defined-only", hip.path], text=True)
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    assert sorted(n for n in exported if n.startswith("wdpm_group_rims")) == names
    # a table of its own: disjoint from the four others
    others = set(ponds.SYMBOLS) | set(ponds.GROUP_SYMBOLS) | set(ponds.RIM_SYMBOLS) | set(capi.SYMBOLS)
    assert not set(ponds.GROUP_RIM_SYMBOLS) & others
    # the three pinned prefix lists are what they were
    assert sorted(n for n in exported if n.startswith("wdpm_group_ponds")) == sorted(ponds.GROUP_SYMBOLS) and len(ponds.GROUP_SYMBOLS) == 9
    assert sorted(n for n in exported if n.startswith("wdpm_rims")) == sorted(ponds.RIM_SYMBOLS) and len(ponds.RIM_SYMBOLS) == 3
    assert sorted(n for n in exported if n.startswith("wdpm_ponds")) == sorted(ponds.SYMBOLS) and len(ponds.SYMBOLS) == 8
    assert not [n for n in names if n.startswith(("wdpm_group_ponds", "wdpm_rims", "wdpm_ponds"))]
    dll = ponds.bind(hip)
    assert all(getattr(dll, n).argtypes == args for n, (_, args) in ponds.GROUP_RIM_SYMBOLS.items())
    assert '#include "wdpm_group_ponds.h"' in header() and '#include "wdpm_pond_rims.h"' in header()


def test_struct_layout_matches_the_header():
    from wdpm_amd import ponds
    body = re.search(r"typedef struct wdpm_group_rim_stats \{(.*?)\} wdpm_group_rim_stats;", header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int64_t|double)\s+(\w+);", body)
    kinds = {"int64_t": C.c_int64, "double": C.c_double}
    assert [(n, kinds[t]) for t, n in fields] == list(ponds.GroupRimStatsStruct._fields_)
    assert C.sizeof(ponds.GroupRimStatsStruct) == 8 * len(fields)
    assert {"ranks", "foreign", "merge_ms"} <= {n for _, n in fields}


def test_every_entry_point_refuses_null_by_name(hip):
    from wdpm_amd import ponds
    dll = ponds.bind(hip)
    n, ms, st = C.c_int64(-1), (C.c_double * 2)(-1.0, -1.0), ponds.GroupRimStatsStruct()
    calls = {
        "wdpm_group_rims_label": lambda: dll.wdpm_group_rims_label(None, 0.001, C.byref(n)),
        "wdpm_group_rims_table": lambda: dll.wdpm_group_rims_table(None, None, 0),
        "wdpm_group_rims_stats": lambda: dll.wdpm_group_rims_stats(None, C.byref(st)),
        "wdpm_group_rims_phase_ms": lambda: dll.wdpm_group_rims_phase_ms(None, 0, ms),
    }
    assert sorted(calls) == NAMES
    for name, call in calls.items():
        assert call() != 0, name
        assert name.encode() in dll.wdpm_last_error(), (name, dll.wdpm_last_error())
    assert n.value == -1 and list(ms) == [-1.0, -1.0]
