"""CPU-side checks of the spills' boundary: include/wdpm_pond_spills.h, wdpm_amd/ponds.py and the product library name the same four
symbols under a prefix of their own, and the older dictionaries with their exports stay as they are; the structs are laid out as the
binding says; every entry point refuses a null handle by name, and the label call a bad threshold or tolerance; and the command line,
linked against a back-end without spills, says so."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from conftest import GOLDEN, ROOT

NAMES = ["wdpm_spill_label", "wdpm_spill_phase_ms", "wdpm_spill_stats", "wdpm_spill_table"]
ROW = [("next", "int32_t", 0), ("sink", "int32_t", 4), ("end", "int32_t", 8), ("hops", "int32_t", 12), ("rest", "int32_t", 16),
       ("rest_hops", "int32_t", 20), ("spilling", "int32_t", 24), ("reserved", "int32_t", 28), ("path_fill_q", "uint64_t", 32),
       ("up_ponds", "int64_t", 40), ("up_cells", "int64_t", 48), ("up_fill_q", "uint64_t", 56), ("live_ponds", "int64_t", 64),
       ("live_cells", "int64_t", 72)]
STATS = ["ponds", "rings", "ring_ponds", "spilling", "ends_land", "ends_none", "ends_ring", "max_hops", "rounds"]


def header():
    return open(os.path.join(ROOT, "include", "wdpm_pond_spills.h")).read()


def test_header_binding_and_library_agree(hip):
    from wdpm_amd import ponds
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(wdpm_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(ponds.SPILL_SYMBOLS) == NAMES
    assert '#include "wdpm_pond_curves.h"' in text
    out = subprocess.check_output(["nm", "-D", "--defined-only", hip.path], text=True)
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    assert sorted(n for n in exported if n.startswith("wdpm_spill")) == names
    # the older dictionaries hold none of it, no older prefix begins the new one, and their exports are what they were
    others = dict(wdpm_ponds=ponds.SYMBOLS, wdpm_rims=ponds.RIM_SYMBOLS, wdpm_catch=ponds.CATCH_SYMBOLS, wdpm_outlets=ponds.OUTLET_SYMBOLS,
                  wdpm_curves=ponds.CURVE_SYMBOLS, wdpm_group_ponds=ponds.GROUP_SYMBOLS, wdpm_group_rims=ponds.GROUP_RIM_SYMBOLS,
                  wdpm_group_catch=ponds.GROUP_CATCH_SYMBOLS, wdpm_group_outlets=ponds.GROUP_OUTLET_SYMBOLS,
                  wdpm_group_curves=ponds.GROUP_CURVE_SYMBOLS)
    assert not any(set(ponds.SPILL_SYMBOLS) & set(d) for d in others.values())
    assert [len(d) for d in others.values()] == [8, 3, 5, 4, 5, 9, 4, 5, 4, 4]
    for prefix, d in others.items():
        assert not "wdpm_spill_".startswith(prefix)
        assert sorted(n for n in exported if n.startswith(prefix)) == sorted(d)
    dll = ponds.bind(hip)
    assert all(getattr(dll, n).argtypes == args and getattr(dll, n).restype == res for n, (res, args) in ponds.SPILL_SYMBOLS.items())
    assert ponds.SPILL_SYMBOLS["wdpm_spill_label"][1] == [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_int64)]
    assert all(hasattr(ponds.Ponds, m) for m in ("label_spills", "spills", "spill_stats", "spill_phase_ms"))
    assert not any(hasattr(ponds.GroupPonds, m) for m in ("label_spills", "spills", "spill_stats", "spill_phase_ms"))


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
    assert struct_fields("wdpm_pond_spill") == [(n, t) for n, t, _ in ROW]
    names = [n for n, _, _ in ROW]
    assert [n for n, _ in ponds.SpillStruct._fields_] == list(ponds.SPILL_DTYPE.names) == names
    assert [getattr(ponds.SpillStruct, n).offset for n in names] == [ponds.SPILL_DTYPE.fields[n][1] for n in names] == [o for _, _, o in ROW]
    kinds = {"int32_t": "<i4", "int64_t": "<i8", "uint64_t": "<u8"}
    assert [ponds.SPILL_DTYPE[n].str for n in names] == [kinds[t] for _, t, _ in ROW]
    assert ponds.SPILL_DTYPE.itemsize == C.sizeof(ponds.SpillStruct) == 80
    stats = struct_fields("wdpm_pond_spill_stats")
    assert [n for n, _ in stats] == [n for n, _ in ponds.SpillStatsStruct._fields_] == STATS and all(t == "int64_t" for _, t in stats)
    assert [getattr(ponds.SpillStatsStruct, n).offset for n in STATS] == list(range(0, 72, 8)) and C.sizeof(ponds.SpillStatsStruct) == 72
    assert int(re.search(r"#define WDPM_SPILL_PHASES (\d+)", header()).group(1)) == len(ponds.SPILL_PHASES) == 3
    assert ponds.SPILL_PHASES == ("rings", "chains", "sums")
    from pond_spills_model import SPILL_DTYPE, STATS as MODEL_STATS
    assert SPILL_DTYPE == ponds.SPILL_DTYPE and list(MODEL_STATS) == STATS


def test_null_handles_and_bad_arguments_are_refused_by_name(hip):
    from wdpm_amd import ponds
    dll = ponds.bind(hip)
    n, ms, st = C.c_int64(-1), (C.c_double * 3)(-1.0, -1.0, -1.0), ponds.SpillStatsStruct(*([-1] * 9))
    assert dll.wdpm_spill_label(None, 0.001, 0.0, C.byref(n)) != 0 and b"wdpm_spill_label: null handle" in dll.wdpm_last_error()
    assert n.value == -1
    assert dll.wdpm_spill_table(None, None, 0) != 0 and b"wdpm_spill_table" in dll.wdpm_last_error()
    assert dll.wdpm_spill_stats(None, C.byref(st)) != 0 and b"wdpm_spill_stats" in dll.wdpm_last_error()
    assert st.rounds == -1 and st.ponds == -1
    assert dll.wdpm_spill_phase_ms(None, ms) != 0 and b"wdpm_spill_phase_ms" in dll.wdpm_last_error()
    assert list(ms) == [-1.0, -1.0, -1.0]
    # the arguments are looked at before the handle is used: any non-null pointer will do for a handle here
    fake = C.create_string_buffer(8)
    for md, tol, word in ((float("nan"), 0.0, b"min_depth"), (-1.0, 0.0, b"min_depth"), (float("inf"), 0.0, b"min_depth"),
                          (0.001, float("nan"), b"headroom_tol"), (0.001, -0.001, b"headroom_tol"), (0.001, float("inf"), b"headroom_tol")):
        assert dll.wdpm_spill_label(fake, md, tol, C.byref(n)) != 0
        assert b"wdpm_spill_label" in dll.wdpm_last_error() and word in dll.wdpm_last_error(), dll.wdpm_last_error()
        assert n.value == -1


def test_cli_says_so_on_a_backend_without_spills(tmp_path):
    """as WDPM_POND_CURVES does (tests/test_pond_curves_abi.py): no file, a message, the run's own outputs complete and unchanged,
    exit status 4"""
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
    for extra in (dict(WDPM_POND_SPILLS="spills.csv"), dict(WDPM_POND_SPILLS="spills.csv", WDPM_POND_HEADROOM_MM="1"),
                  dict(WDPM_POND_SPILLS="spills.csv", WDPM_POND_CURVES="curves.csv", WDPM_PONDS="ponds.csv")):
        p = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120, env=dict(env, **extra))
        assert p.returncode == 4 and "pond spills" in p.stderr and "oracle-cpu" in p.stderr, p.stderr
        assert not any(os.path.exists(tmp_path / f) for f in ("spills.csv", "curves.csv", "ponds.csv"))
        assert strip_timing(p.stdout) == strip_timing(plain.stdout) and open(tmp_path / "out.asc", "rb").read() == raster
