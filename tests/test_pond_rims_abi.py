"""CPU-side checks of the rims' boundary: include/wdpm_pond_rims.h, wdpm_amd/ponds.py and the product library name the same three
symbols under a prefix of their own (the two inventory headers stay as they are); the struct is laid out as the binding says;
every entry point refuses a null handle by name; and the command line, linked against a back-end without rims, says so."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from conftest import GOLDEN, ROOT


def header():
    return open(os.path.join(ROOT, "include", "wdpm_pond_rims.h")).read()


def test_header_binding_and_library_agree(hip):
    from wdpm_amd import ponds
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(wdpm_[a-z_0-9]+)\s*\(", text)))
    assert names == sorted(ponds.RIM_SYMBOLS) == ["wdpm_rims_label", "wdpm_rims_phase_ms", "wdpm_rims_table"]
    assert all(n.startswith("wdpm_rims_") for n in names)
    out = subprocess.check_output(["nm", "-D", "--defined-only", hip.path], text=True)
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    assert sorted(n for n in exported if n.startswith("wdpm_rims")) == names
    # a third dictionary: the two the inventory's own ABI tests compare with their headers hold none of it
    assert not set(ponds.RIM_SYMBOLS) & (set(ponds.SYMBOLS) | set(ponds.GROUP_SYMBOLS))
    dll = ponds.bind(hip)
    assert all(getattr(dll, n).argtypes == args for n, (_, args) in ponds.RIM_SYMBOLS.items())


def test_struct_layout_matches_the_header():
    from wdpm_amd import ponds
    body = re.search(r"typedef struct wdpm_pond_rim \{(.*?)\} wdpm_pond_rim;", header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    kinds = {"int32_t": "<i4", "int64_t": "<i8", "uint64_t": "<u8", "double": "<f8"}
    assert [(n, kinds[t]) for n, t in fields] == [(n, ponds.RIM_DTYPE[n].str) for n in ponds.RIM_DTYPE.names]
    assert [n for n, _ in ponds.RimStruct._fields_] == list(ponds.RIM_DTYPE.names)
    assert [getattr(ponds.RimStruct, n).offset for n in ponds.RIM_DTYPE.names] == [ponds.RIM_DTYPE.fields[n][1] for n in ponds.RIM_DTYPE.names]
    assert ponds.RIM_DTYPE.itemsize == C.sizeof(ponds.RimStruct) == 48
    assert int(re.search(r"#define WDPM_RIMS_PHASES (\d+)", header()).group(1)) == len(ponds.RIM_PHASES)


def test_null_handles_are_refused_by_name(hip):
    from wdpm_amd import ponds
    dll = ponds.bind(hip)
    n, ms = C.c_int64(-1), (C.c_double * 2)(-1.0, -1.0)
    assert dll.wdpm_rims_label(None, 0.001, C.byref(n)) != 0 and b"wdpm_rims_label" in dll.wdpm_last_error()
    assert n.value == -1
    assert dll.wdpm_rims_table(None, None, 0) != 0 and b"wdpm_rims_table" in dll.wdpm_last_error()
    assert dll.wdpm_rims_phase_ms(None, ms) != 0 and b"wdpm_rims_phase_ms" in dll.wdpm_last_error()
    assert list(ms) == [-1.0, -1.0]


def test_cli_says_so_on_a_backend_without_rims(tmp_path):
    """as WDPM_PONDS does (tests/test_ponds_abi.py): no file, a message, the run's own outputs complete and unchanged, exit status 4"""
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
    for extra in (dict(WDPM_POND_RIMS="rims.csv"), dict(WDPM_POND_RIMS="rims.csv", WDPM_PONDS="ponds.csv")):
        p = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120, env=dict(env, **extra))
        assert p.returncode == 4 and "pond rims" in p.stderr and "oracle-cpu" in p.stderr, p.stderr
        assert not os.path.exists(tmp_path / "rims.csv") and not os.path.exists(tmp_path / "ponds.csv")
        assert strip_timing(p.stdout) == strip_timing(plain.stdout) and open(tmp_path / "out.asc", "rb").read() == raster
