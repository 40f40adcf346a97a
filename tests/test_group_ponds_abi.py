"""CPU-side checks of the boundary of the pond inventory over row blocks: include/wdpm_group_ponds.h, wdpm_amd.ponds.GROUP_SYMBOLS
and the product library name the same symbols, the struct layouts match the header, and every entry point refuses null with a
message.  Nothing runs on a GPU."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wdpm_[a-z_0-9]+)\s*\(", text)))


def test_header_binding_and_library_agree(hip):
    from wdpm_amd import capi, ponds
    names = declared("wdpm_group_ponds.h")
    assert names == sorted(ponds.GROUP_SYMBOLS)
    assert len(names) == 9 and all(n.startswith("wdpm_group_ponds_") for n in names)
    out = subprocess.check_output(["nm", "-D", "--defined-only", hip.path], text=True)
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    assert not [n for n in names if n not in exported]
    # the library exports no group-inventory symbol the header does not declare
    assert sorted(n for n in exported if n.startswith("wdpm_group_ponds")) == names
    # the tables of the two older headers know none of them
    assert not set(ponds.GROUP_SYMBOLS) & (set(ponds.SYMBOLS) | set(capi.SYMBOLS))
    assert '#include "wdpm_ponds.h"' in open(os.path.join(ROOT, "include", "wdpm_group_ponds.h")).read()


def test_struct_layout_matches_the_header():
    from wdpm_amd import ponds
    text = open(os.path.join(ROOT, "include", "wdpm_group_ponds.h")).read()
    body = re.search(r"typedef struct wdpm_group_pond_stats \{(.*?)\} wdpm_group_pond_stats;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int64_t|double)\s+(\w+);", body)
    kinds = {"int64_t": C.c_int64, "double": C.c_double}
    assert [(n, kinds[t]) for t, n in fields] == list(ponds.GroupStatsStruct._fields_)
    assert C.sizeof(ponds.GroupStatsStruct) == 8 * len(fields) == 48


def test_every_entry_point_refuses_null_with_a_message(hip):
    from wdpm_amd import ponds
    dll = ponds.bind(hip)
    h, n, v = C.c_void_p(), C.c_int64(-1), C.c_int64(-1)
    gs, rs, ms = ponds.GroupStatsStruct(), ponds.StatsStruct(), (C.c_double * len(ponds.PHASES))()
    calls = {
        "wdpm_group_ponds_create": lambda: dll.wdpm_group_ponds_create(C.byref(h), None),
        "wdpm_group_ponds_label": lambda: dll.wdpm_group_ponds_label(None, 0.001, C.byref(n)),
        "wdpm_group_ponds_table": lambda: dll.wdpm_group_ponds_table(None, None, 0),
        "wdpm_group_ponds_labels": lambda: dll.wdpm_group_ponds_labels(None, None),
        "wdpm_group_ponds_guard_bad": lambda: dll.wdpm_group_ponds_guard_bad(None, C.byref(v)),
        "wdpm_group_ponds_stats": lambda: dll.wdpm_group_ponds_stats(None, C.byref(gs)),
        "wdpm_group_ponds_rank_stats": lambda: dll.wdpm_group_ponds_rank_stats(None, 0, C.byref(rs)),
        "wdpm_group_ponds_phase_ms": lambda: dll.wdpm_group_ponds_phase_ms(None, 0, ms),
    }
    assert sorted(list(calls) + ["wdpm_group_ponds_destroy"]) == sorted(ponds.GROUP_SYMBOLS)
    for name, call in calls.items():
        assert call() != 0, name
        assert name.encode() in dll.wdpm_last_error(), (name, dll.wdpm_last_error())
    assert not h.value and n.value == -1 and v.value == -1
    assert dll.wdpm_group_ponds_create(None, None) != 0
    dll.wdpm_group_ponds_destroy(None)        # harmless
