"""CPU-side checks of the outlets' boundary: include/wdpm_pond_outlets.h, wdpm_amd/ponds.py and the product library name the same
four symbols under a prefix of their own, and the five dictionaries of the inventory, the rims and the catchments with their
exports stay as they are; the structs are laid out as the binding says; every entry point refuses a null handle by name; and the
command line, linked against a back-end without outlets, says so."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from conftest import GOLDEN, ROOT

NAMES = ["wdpm_outlets_label", "wdpm_outlets_phase_ms", "wdpm_outlets_stats", "wdpm_outlets_table"]


def header():
    return open(os.path.join(ROOT, "include", "wdpm_pond_outlets.h")).read()


def test_header_binding_and_library_agree(hip):
    from wdpm_amd import ponds
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(wdpm_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(ponds.OUTLET_SYMBOLS) == NAMES
    assert '#include "wdpm_pond_catchments.h"' in text
    out = subprocess.check_output(["nm", "-D", "--defined-only", hip.path], text=True)
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    assert sorted(n for n in exported if n.startswith("wdpm_outlets")) == names
    # the five dictionaries the other ABI tests compare with their headers hold none of it, and their exports are what they were
    others = (ponds.SYMBOLS, ponds.RIM_SYMBOLS, ponds.GROUP_SYMBOLS, ponds.GROUP_RIM_SYMBOLS, ponds.CATCH_SYMBOLS)
    assert not any(set(ponds.OUTLET_SYMBOLS) & set(d) for d in others)
    assert [len(d) for d in others] == [8, 3, 9, 4, 5]
    for prefix, d in zip(("wdpm_ponds", "wdpm_rims", "wdpm_group_ponds", "wdpm_group_rims", "wdpm_catch"), others):
        assert sorted(n for n in exported if n.startswith(prefix)) == sorted(d)
    dll = ponds.bind(hip)
    assert all(getattr(dll, n).argtypes == args for n, (_, args) in ponds.OUTLET_SYMBOLS.items())
    assert ponds._LABELLED_BY["outlets"] == "label_outlets"


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
    kinds = {"int32_t": "<i4", "int64_t": "<i8", "uint64_t": "<u8", "double": "<f8"}
    fields = struct_fields("wdpm_pond_outlet")
    assert [(n, kinds[t]) for n, t in fields] == [(n, ponds.OUTLET_DTYPE[n].str) for n in ponds.OUTLET_DTYPE.names]
    assert [n for n, _ in ponds.OutletStruct._fields_] == list(ponds.OUTLET_DTYPE.names)
    assert [getattr(ponds.OutletStruct, n).offset for n in ponds.OUTLET_DTYPE.names] == \
        [ponds.OUTLET_DTYPE.fields[n][1] for n in ponds.OUTLET_DTYPE.names] == [0, 8, 12, 16, 20, 24, 28, 32, 40, 48]
    assert ponds.OUTLET_DTYPE.itemsize == C.sizeof(ponds.OutletStruct) == 56
    stats = struct_fields("wdpm_pond_outlet_stats")
    assert [n for n, _ in stats] == [n for n, _ in ponds.OutletStatsStruct._fields_] == ["ponds", "no_outlet", "to_land", "divide_cells"]
    assert all(t == "int64_t" for _, t in stats)
    assert [getattr(ponds.OutletStatsStruct, n).offset for n, _ in stats] == [0, 8, 16, 24] and C.sizeof(ponds.OutletStatsStruct) == 32
    assert int(re.search(r"#define WDPM_OUTLETS_PHASES (\d+)", header()).group(1)) == len(ponds.OUTLET_PHASES) == 2
    assert ponds.OUTLET_PHASES == ("passes", "locate")


def test_null_handles_are_refused_by_name(hip):
    from wdpm_amd import ponds
    dll = ponds.bind(hip)
    n, ms, st = C.c_int64(-1), (C.c_double * 2)(-1.0, -1.0), ponds.OutletStatsStruct(-1, -1, -1, -1)
    assert dll.wdpm_outlets_label(None, 0.001, C.byref(n)) != 0 and b"wdpm_outlets_label" in dll.wdpm_last_error()
    assert n.value == -1
    assert dll.wdpm_outlets_table(None, None, 0) != 0 and b"wdpm_outlets_table" in dll.wdpm_last_error()
    assert dll.wdpm_outlets_stats(None, C.byref(st)) != 0 and b"wdpm_outlets_stats" in dll.wdpm_last_error()
    assert st.divide_cells == -1
    assert dll.wdpm_outlets_phase_ms(None, ms) != 0 and b"wdpm_outlets_phase_ms" in dll.wdpm_last_error()
    assert list(ms) == [-1.0, -1.0]


def test_cli_says_so_on_a_backend_without_outlets(tmp_path):
    """as WDPM_POND_CATCHMENTS does (tests/test_pond_catchments_abi.py): no file, a message, the run's own outputs complete and
    unchanged, exit status 4"""
    sys.path.insert(0, GOLDEN)
    from make_golden import strip_timing
    exe = os.path.join(ROOT, "oracle", "_build", "WDPMCL_oracle")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "oracle"])
    y, x = np.mgrid[0:30, 0:40]
    with open(tmp_path / "dem.asc", "w") as f:
        f.write("ncols 40\nnrows 30\nxllcorner 0\nyllcorner 0\ncellsize 10\nNODATA_value -99999\n")
        np.savetxt(f, 500.0 + np.round(np.sin(x / 3.0) * np.cos(y / 4.0), 4), fmt="%.4f")
    args = [exe, "add", "dem.asc", "NULL", "out.asc", "NULL", "100", "1.0", "1.0", "0", "0", "0.005", "1000"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("WDPM_POND")}
    plain = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120, env=env)
    assert plain.returncode == 0, plain.stderr
    raster = open(tmp_path / "out.asc", "rb").read()
    for extra in (dict(WDPM_POND_OUTLETS="outlets.csv"),
                  dict(WDPM_POND_OUTLETS="outlets.csv", WDPM_POND_CATCHMENTS="catch.csv", WDPM_POND_RIMS="rims.csv", WDPM_PONDS="ponds.csv")):
        p = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120, env=dict(env, **extra))
        assert p.returncode == 4 and "pond outlets" in p.stderr and "oracle-cpu" in p.stderr, p.stderr
        assert not any(os.path.exists(tmp_path / f) for f in ("outlets.csv", "catch.csv", "rims.csv", "ponds.csv"))
        assert strip_timing(p.stdout) == strip_timing(plain.stdout) and open(tmp_path / "out.asc", "rb").read() == raster
