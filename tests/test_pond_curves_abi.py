"""CPU-side checks of the stage curves' boundary: include/wdpm_pond_curves.h, wdpm_amd/ponds.py and the product library name the
same five symbols under a prefix of their own, and the eight older dictionaries with their exports stay as they are; the structs are
laid out as the binding says; every entry point that takes a handle refuses a null one by name; wdpm_curves_stage_level gives the
end points and NaN outside 0..16; and the command line, linked against a back-end without curves, says so."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np

from conftest import GOLDEN, ROOT

NAMES = ["wdpm_curves_label", "wdpm_curves_phase_ms", "wdpm_curves_stage_level", "wdpm_curves_stats", "wdpm_curves_table"]


def header():
    return open(os.path.join(ROOT, "include", "wdpm_pond_curves.h")).read()


def test_header_binding_and_library_agree(hip):
    from wdpm_amd import ponds
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(wdpm_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(ponds.CURVE_SYMBOLS) == NAMES
    assert '#include "wdpm_pond_outlets.h"' in text
    out = subprocess.check_output(["nm", "-D", "--defined-only", hip.path], text=True)
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    assert sorted(n for n in exported if n.startswith("wdpm_curves")) == names
    # the eight older dictionaries hold none of it, and their exports are what they were
    others = (ponds.SYMBOLS, ponds.RIM_SYMBOLS, ponds.CATCH_SYMBOLS, ponds.OUTLET_SYMBOLS, ponds.GROUP_SYMBOLS, ponds.GROUP_RIM_SYMBOLS,
              ponds.GROUP_CATCH_SYMBOLS, ponds.GROUP_OUTLET_SYMBOLS)
    assert not any(set(ponds.CURVE_SYMBOLS) & set(d) for d in others)
    assert [len(d) for d in others] == [8, 3, 5, 4, 9, 4, 5, 4]
    prefixes = ("wdpm_ponds", "wdpm_rims", "wdpm_catch", "wdpm_outlets", "wdpm_group_ponds", "wdpm_group_rims", "wdpm_group_catch",
                "wdpm_group_outlets")
    for prefix, d in zip(prefixes, others):
        assert sorted(n for n in exported if n.startswith(prefix)) == sorted(d)
    dll = ponds.bind(hip)
    assert all(getattr(dll, n).argtypes == args and getattr(dll, n).restype == res for n, (res, args) in ponds.CURVE_SYMBOLS.items())
    assert ponds._LABELLED_BY == {"table": "label", "rims": "label_rims", "catchments": "label_catchments", "outlets": "label_outlets"}
    assert not any(hasattr(ponds.GroupPonds, m) for m in ("label_curves", "curves", "curve_stats", "curve_phase_ms"))


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
    stages = int(re.search(r"#define WDPM_CURVE_STAGES (\d+)", header()).group(1))
    assert stages == ponds.CURVE_STAGES == 16
    fields = struct_fields("wdpm_pond_curve")
    assert fields == [("bed_level", "double"), ("top_level", "double"), ("cells[WDPM_CURVE_STAGES]", "int64_t"), ("q[WDPM_CURVE_STAGES]", "uint64_t")]
    names = ["bed_level", "top_level", "cells", "q"]
    assert [n for n, _ in ponds.CurveStruct._fields_] == list(ponds.CURVE_DTYPE.names) == names
    assert [getattr(ponds.CurveStruct, n).offset for n in names] == [ponds.CURVE_DTYPE.fields[n][1] for n in names] == [0, 8, 16, 144]
    assert [ponds.CURVE_DTYPE[n].str for n in names[:2]] == ["<f8", "<f8"]
    assert ponds.CURVE_DTYPE["cells"].subdtype == (np.dtype("<i8"), (16,)) and ponds.CURVE_DTYPE["q"].subdtype == (np.dtype("<u8"), (16,))
    assert ponds.CURVE_DTYPE.itemsize == C.sizeof(ponds.CurveStruct) == 272
    stats = struct_fields("wdpm_pond_curve_stats")
    assert [n for n, _ in stats] == [n for n, _ in ponds.CurveStatsStruct._fields_] == ["ponds", "no_curve", "flat", "stage_cells"]
    assert all(t == "int64_t" for _, t in stats)
    assert [getattr(ponds.CurveStatsStruct, n).offset for n, _ in stats] == [0, 8, 16, 24] and C.sizeof(ponds.CurveStatsStruct) == 32
    assert int(re.search(r"#define WDPM_CURVES_PHASES (\d+)", header()).group(1)) == len(ponds.CURVE_PHASES) == 2
    assert ponds.CURVE_PHASES == ("bed", "stages")


def test_null_handles_are_refused_by_name(hip):
    from wdpm_amd import ponds
    dll = ponds.bind(hip)
    n, ms, st = C.c_int64(-1), (C.c_double * 2)(-1.0, -1.0), ponds.CurveStatsStruct(-1, -1, -1, -1)
    assert dll.wdpm_curves_label(None, 0.001, C.byref(n)) != 0 and b"wdpm_curves_label" in dll.wdpm_last_error()
    assert n.value == -1
    assert dll.wdpm_curves_table(None, None, 0) != 0 and b"wdpm_curves_table" in dll.wdpm_last_error()
    assert dll.wdpm_curves_stats(None, C.byref(st)) != 0 and b"wdpm_curves_stats" in dll.wdpm_last_error()
    assert st.stage_cells == -1
    assert dll.wdpm_curves_phase_ms(None, ms) != 0 and b"wdpm_curves_phase_ms" in dll.wdpm_last_error()
    assert list(ms) == [-1.0, -1.0]


def test_stage_level_end_points_and_range(hip):
    from wdpm_amd import ponds
    f = ponds.bind(hip).wdpm_curves_stage_level
    for bed, top in ((0.0, 16.0), (-0.0, 0.0), (497.25, 501.0625), (3.0, float("inf")), (1e300, -1e300)):
        assert math.copysign(1.0, f(bed, top, 0)) == math.copysign(1.0, bed) and f(bed, top, 0) == bed
        assert f(bed, top, 16) == top
        for s in (-1, 17, 2 ** 31 - 1, -2 ** 31):
            assert math.isnan(f(bed, top, s))
    assert [f(0.0, 16.0, s) for s in range(17)] == [float(s) for s in range(17)]
    assert f(1.0, 2.0, 1) == 1.0625 and f(1.0, 1.0 + 2.0 ** -52, 8) == 1.0 and f(1.0, 1.0 + 2.0 ** -52, 9) == 1.0 + 2.0 ** -52
    # never fused: pairs for which one rounding of bed + span * (s / 16) - what a fused multiply-add would give - is another double
    # than the three rounded operations; exact rationals tell which
    from fractions import Fraction
    rng = np.random.default_rng(16)
    told = 0
    for bed, span in zip(rng.random(400).tolist(), (rng.random(400) * 1000).tolist()):
        top = bed + span
        for s in (3, 7, 11, 13):
            d = top - bed
            fused = float(Fraction(bed) + Fraction(d) * Fraction(s, 16))
            plain = bed + d * (s / 16.0)
            assert f(bed, top, s) == plain
            told += fused != plain
    assert told > 20
    assert ponds.stage_levels(2.0, 4.0, hip).tolist() == [2.0 + s / 8.0 for s in range(17)]


def test_cli_says_so_on_a_backend_without_curves(tmp_path):
    """as WDPM_POND_OUTLETS does (tests/test_pond_outlets_abi.py): no file, a message, the run's own outputs complete and
    unchanged, exit status 4"""
    sys.path.insert(0, GOLDEN)
    from make_golden import strip_timing
    exe = os.path.join(ROOT, "oracle", "_build", "WDPMCL_oracle")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "oracle"], stdout=subprocess.DEVNULL)
    y, x = np.mgrid[0:30, 0:40]
    with open(tmp_path / "dem.asc", "w") as f:
        f.write("ncols 40\nnrows 30\nxllcorner 0\nyllcorner 0\ncellsize 10\nNODATA_value -99999\n")
        np.savetxt(f, 500.0 + np.round(np.sin(x / 3.0) * np.cos(y / 4.0), 4), fmt="%.4f")
    args = [exe, "add", "dem.asc", "NULL", "out.asc", "NULL", "100", "1.0", "1.0", "0", "0", "0.005", "1000"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("WDPM_POND")}
    plain = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120, env=env)
    assert plain.returncode == 0, plain.stderr
    raster = open(tmp_path / "out.asc", "rb").read()
    for extra in (dict(WDPM_POND_CURVES="curves.csv"),
                  dict(WDPM_POND_CURVES="curves.csv", WDPM_POND_OUTLETS="outlets.csv", WDPM_POND_CATCHMENTS="catch.csv",
                       WDPM_POND_RIMS="rims.csv", WDPM_PONDS="ponds.csv")):
        p = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120, env=dict(env, **extra))
        assert p.returncode == 4 and "pond curves" in p.stderr and "oracle-cpu" in p.stderr, p.stderr
        assert not any(os.path.exists(tmp_path / f) for f in ("curves.csv", "outlets.csv", "catch.csv", "rims.csv", "ponds.csv"))
        assert strip_timing(p.stdout) == strip_timing(plain.stdout) and open(tmp_path / "out.asc", "rb").read() == raster
