"""CPU-side checks of the routing's boundary: include/wdpm_pond_routing.h, wdpm_amd/ponds.py and the product library name the same six
symbols under a prefix of their own, and the older dictionaries with their exports stay as they are; the structs are laid out as the
binding says; every entry point refuses a null handle by name, and the label call and the rerun a bad runoff depth; the pure rule
wdpm_route_runoff_q is the model's."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NAMES = ["wdpm_route_label", "wdpm_route_phase_ms", "wdpm_route_rerun", "wdpm_route_runoff_q", "wdpm_route_stats", "wdpm_route_table"]
ROW = [("own_q", "uint64_t", 0), ("in_q", "uint64_t", 8), ("kept_q", "uint64_t", 16), ("out_q", "uint64_t", 24), ("reach_ponds", "int64_t", 32),
       ("reach_cells", "int64_t", 40), ("overflows", "int32_t", 48), ("full", "int32_t", 52), ("level", "int32_t", 56), ("reserved", "int32_t", 60)]
STATS = [("ponds", "int64_t"), ("runoff_q", "int64_t"), ("levels", "int64_t"), ("wide_levels", "int64_t"), ("launches", "int64_t"),
         ("overflowing", "int64_t"), ("full", "int64_t"), ("own_q", "uint64_t"), ("kept_q", "uint64_t"), ("out_land_q", "uint64_t"),
         ("out_ring_q", "uint64_t")]


def header():
    return open(os.path.join(ROOT, "include", "wdpm_pond_routing.h")).read()


def test_header_binding_and_library_agree(hip):
    from wdpm_amd import ponds
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(wdpm_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(ponds.ROUTE_SYMBOLS) == NAMES
    assert '#include "wdpm_pond_spills.h"' in text
    out = subprocess.check_output(["nm", "-D", "--defined-only", hip.path], text=True)
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    assert sorted(n for n in exported if n.startswith("wdpm_route")) == names
    # the older dictionaries hold none of it, no older prefix begins the new one or is begun by it, and their exports are what they were
    others = dict(wdpm_ponds=ponds.SYMBOLS, wdpm_rims=ponds.RIM_SYMBOLS, wdpm_catch=ponds.CATCH_SYMBOLS, wdpm_outlets=ponds.OUTLET_SYMBOLS,
                  wdpm_curves=ponds.CURVE_SYMBOLS, wdpm_spill=ponds.SPILL_SYMBOLS, wdpm_group_ponds=ponds.GROUP_SYMBOLS,
                  wdpm_group_rims=ponds.GROUP_RIM_SYMBOLS, wdpm_group_catch=ponds.GROUP_CATCH_SYMBOLS,
                  wdpm_group_outlets=ponds.GROUP_OUTLET_SYMBOLS, wdpm_group_curves=ponds.GROUP_CURVE_SYMBOLS)
    assert not any(set(ponds.ROUTE_SYMBOLS) & set(d) for d in others.values())
    assert [len(d) for d in others.values()] == [8, 3, 5, 4, 5, 4, 9, 4, 5, 4, 4]
    for prefix, d in others.items():
        assert not "wdpm_route_".startswith(prefix) and not prefix.startswith("wdpm_route")
        assert sorted(n for n in exported if n.startswith(prefix)) == sorted(d)
    assert all(n.startswith("wdpm_route_") for n in names)
    dll = ponds.bind(hip)
    assert all(getattr(dll, n).argtypes == args and getattr(dll, n).restype == res for n, (res, args) in ponds.ROUTE_SYMBOLS.items())
    assert ponds.ROUTE_SYMBOLS["wdpm_route_label"][1] == [C.c_void_p, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int64)]
    assert ponds.ROUTE_SYMBOLS["wdpm_route_rerun"][1] == [C.c_void_p, C.c_double] and ponds.ROUTE_SYMBOLS["wdpm_route_runoff_q"] == (C.c_int64, [C.c_double])
    methods = ("label_routing", "route", "routing", "routing_stats", "routing_phase_ms")
    assert all(hasattr(ponds.Ponds, m) for m in methods) and not any(hasattr(ponds.GroupPonds, m) for m in methods)
    assert callable(ponds.runoff_q)
    assert ponds._LABELLED_BY == {"table": "label", "rims": "label_rims", "catchments": "label_catchments", "outlets": "label_outlets"}


def struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_struct_layouts_match_the_header():
    from wdpm_amd import ponds
    assert struct_fields("wdpm_pond_route") == [(n, t) for n, t, _ in ROW]
    names = [n for n, _, _ in ROW]
    assert [n for n, _ in ponds.RouteStruct._fields_] == list(ponds.ROUTE_DTYPE.names) == names
    assert [getattr(ponds.RouteStruct, n).offset for n in names] == [ponds.ROUTE_DTYPE.fields[n][1] for n in names] == [o for _, _, o in ROW]
    kinds = {"int32_t": "<i4", "int64_t": "<i8", "uint64_t": "<u8"}
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    assert [ponds.ROUTE_DTYPE[n].str for n in names] == [kinds[t] for _, t, _ in ROW]
    assert [t for _, t in ponds.RouteStruct._fields_] == [ctypes_of[t] for _, t, _ in ROW]
    assert ponds.ROUTE_DTYPE.itemsize == C.sizeof(ponds.RouteStruct) == 64
    assert struct_fields("wdpm_pond_route_stats") == STATS
    assert [(n, t) for n, t in ponds.RouteStatsStruct._fields_] == [(n, ctypes_of[t]) for n, t in STATS]
    assert [getattr(ponds.RouteStatsStruct, n).offset for n, _ in STATS] == list(range(0, 88, 8)) and C.sizeof(ponds.RouteStatsStruct) == 88
    assert int(re.search(r"#define WDPM_ROUTE_PHASES (\d+)", header()).group(1)) == len(ponds.ROUTE_PHASES) == 3
    assert ponds.ROUTE_PHASES == ("order", "sweep", "finish")
    from pond_routing_model import PLAN_STATS, ROUTE_DTYPE, STATS as MODEL_STATS
    assert ROUTE_DTYPE == ponds.ROUTE_DTYPE and sorted(MODEL_STATS + PLAN_STATS) == sorted(n for n, _ in STATS)


def test_null_handles_and_bad_arguments_are_refused_by_name(hip):
    from wdpm_amd import ponds
    dll = ponds.bind(hip)
    n, ms, st = C.c_int64(-1), (C.c_double * 3)(-1.0, -1.0, -1.0), ponds.RouteStatsStruct(*([-1] * 7))
    assert dll.wdpm_route_label(None, 0.001, 0.0, 0.01, C.byref(n)) != 0 and b"wdpm_route_label: null handle" in dll.wdpm_last_error()
    assert n.value == -1
    assert dll.wdpm_route_rerun(None, 0.01) != 0 and b"wdpm_route_rerun: null handle" in dll.wdpm_last_error()
    assert dll.wdpm_route_table(None, None, 0) != 0 and b"wdpm_route_table" in dll.wdpm_last_error()
    assert dll.wdpm_route_stats(None, C.byref(st)) != 0 and b"wdpm_route_stats" in dll.wdpm_last_error()
    assert st.launches == -1 and st.ponds == -1
    assert dll.wdpm_route_phase_ms(None, ms) != 0 and b"wdpm_route_phase_ms" in dll.wdpm_last_error()
    assert list(ms) == [-1.0, -1.0, -1.0]
    # the arguments are looked at before the handle is used: any non-null pointer will do for a handle here
    fake = C.create_string_buffer(8)
    for md, tol, runoff, word in ((float("nan"), 0.0, 0.01, b"min_depth"), (-1.0, 0.0, 0.01, b"min_depth"), (0.001, float("nan"), 0.01, b"headroom_tol"),
                                  (0.001, -0.001, 0.01, b"headroom_tol"), (0.001, 0.0, -0.01, b"runoff_m"), (0.001, 0.0, float("nan"), b"runoff_m"),
                                  (0.001, 0.0, 256.0, b"runoff_m"), (0.001, 0.0, float("inf"), b"runoff_m")):
        assert dll.wdpm_route_label(fake, md, tol, runoff, C.byref(n)) != 0
        assert b"wdpm_route_label" in dll.wdpm_last_error() and word in dll.wdpm_last_error(), dll.wdpm_last_error()
        assert n.value == -1
    for runoff in (-0.01, float("nan"), 256.0, float("inf")):
        assert dll.wdpm_route_rerun(fake, runoff) != 0 and b"wdpm_route_rerun: runoff_m" in dll.wdpm_last_error()


def test_the_runoff_rule_is_the_models(hip):
    from pond_routing_model import runoff_q_of
    from wdpm_amd.ponds import runoff_q
    for m in (0.0, -0.0, 0.001, 0.01, 1.0, 2.0 ** -25, 3 * 2.0 ** -25, 5 * 2.0 ** -25, 1e-12, 255.0, 256.0 - 2.0 ** -24, 256.0 - 2.0 ** -26, 256.0,
              -1e-9, float("nan"), float("inf"), -float("inf"), 1e300, 5e-324, 0.1, 123.456):
        assert runoff_q(m, hip) == runoff_q_of(m), m
    assert runoff_q(256.0, hip) == -1 and runoff_q(0.001, hip) == 16777 and runoff_q(255.0, hip) == 255 * 2 ** 24
