"""CPU-side checks of the pond inventory's boundary: include/wdpm_ponds.h, wdpm_amd/ponds.py and the product library name the
same symbols; include/wdpm.h (the ABI the CPU restatement shares) names none of them; nothing runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wdpm_[a-z_0-9]+)\s*\(", text)))


def test_header_binding_and_library_agree(hip):
    from wdpm_amd import ponds
    names = declared("wdpm_ponds.h")
    assert names == sorted(ponds.SYMBOLS)
    assert len(names) == 8 and all(n.startswith("wdpm_ponds_") for n in names)
    out = subprocess.check_output(["nm", "-D", "--defined-only", hip.path], text=True)
    exported = set(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    assert not [n for n in names if n not in exported]
    # ... and the library exports no pond symbol the header does not declare
    assert sorted(n for n in exported if n.startswith("wdpm_ponds")) == names


def test_the_shared_abi_knows_nothing_of_ponds():
    import wdpm_amd.capi as capi
    from wdpm_amd import ponds
    assert not [n for n in declared("wdpm.h") if "pond" in n]
    assert not set(ponds.SYMBOLS) & set(capi.SYMBOLS)
    assert not [n for n in capi.SYMBOLS if "pond" in n]


def test_struct_layouts_match_the_header():
    from wdpm_amd import ponds
    text = open(os.path.join(ROOT, "include", "wdpm_ponds.h")).read()
    body = re.search(r"typedef struct wdpm_pond \{(.*?)\} wdpm_pond;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    kinds = {"int32_t": "<i4", "int64_t": "<i8", "uint64_t": "<u8", "double": "<f8"}
    assert [(n, kinds[t]) for n, t in fields] == [(n, ponds.POND_DTYPE[n].str) for n in ponds.POND_DTYPE.names]
    assert [n for n, _ in ponds.PondStruct._fields_] == list(ponds.POND_DTYPE.names)
    assert ponds.POND_DTYPE.itemsize == C.sizeof(ponds.PondStruct) == 48
    sbody = re.search(r"typedef struct wdpm_pond_stats \{(.*?)\} wdpm_pond_stats;", text, flags=re.S).group(1)
    sbody = re.sub(r"/\*.*?\*/", "", sbody, flags=re.S)
    assert re.findall(r"int64_t\s+(\w+);", sbody) == [n for n, _ in ponds.StatsStruct._fields_]


def test_label_fails_loudly_without_a_gpu(hip):
    import torch
    import wdpm_amd
    from wdpm_amd import ponds
    dll = ponds.bind(hip)
    if not torch.cuda.is_available():
        # no context can be made, so no handle can
        with pytest.raises(wdpm_amd.WdpmError):
            with hip.context(module="add", nrows=4, ncols=4, missingvalue=-1.0) as ctx:
                ponds.Ponds(ctx).label(0.001)
    # ... and every entry point refuses a null handle with a message instead of running anything
    h, n = C.c_void_p(), C.c_int64(-1)
    assert dll.wdpm_ponds_create(C.byref(h), None) != 0 and b"wdpm_ponds_create" in dll.wdpm_last_error()
    assert not h.value
    assert dll.wdpm_ponds_label(None, 0.001, C.byref(n)) != 0 and b"wdpm_ponds_label" in dll.wdpm_last_error()
    assert n.value == -1
    assert dll.wdpm_ponds_table(None, None, 0) != 0 and dll.wdpm_ponds_labels(None, None) != 0


def test_cli_says_so_on_a_backend_without_the_inventory(tmp_path):
    """The command line references the inventory weakly: linked against a library that exports include/wdpm.h alone (the oracle
    back-end of the CPU tests) it still builds and runs, WDPM_PONDS writes no file and says why, the run's own outputs are complete
    and unchanged, and the exit status tells the caller that what it asked for is missing."""
    import sys

    import numpy as np
    from conftest import GOLDEN
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
    env = {k: v for k, v in os.environ.items() if not k.startswith("WDPM_PONDS")}
    plain = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120, env=env)
    assert plain.returncode == 0, plain.stderr
    raster = open(tmp_path / "out.asc", "rb").read()
    p = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120, env=dict(env, WDPM_PONDS="ponds.csv"))
    assert p.returncode == 4 and "pond inventory" in p.stderr and "oracle-cpu" in p.stderr, p.stderr
    assert not os.path.exists(tmp_path / "ponds.csv")
    assert strip_timing(p.stdout) == strip_timing(plain.stdout) and open(tmp_path / "out.asc", "rb").read() == raster
