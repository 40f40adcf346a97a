"""TEST INFRASTRUCTURE: the command line's pond files against a canned pond back-end (tests/cli_ponds_stub.c), on the CPU.
The command line's sources, the stub and the CPU restatement are linked into one program under AddressSanitizer and UBSan, and a
fixed list of cases is run on one small raster: which files come out, byte for byte, which pond, guard and stub lines stderr
carries, in order, and the exit status.  tests/golden/make_golden.py records them from a given command-line source
(cli_pond_files.json); tests/test_cli_pond_files.py holds the tree's command line against that recording."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wdpm_amd", "csrc")
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden import strip_timing  # noqa: E402

CLI_SOURCES = [os.path.join(CSRC, "wdpmcl_main.c"), os.path.join(CSRC, "wdpmcl_ponds.c")]
UNITS = ["WDPM_PONDS", "WDPM_POND_RIMS", "WDPM_POND_CATCHMENTS", "WDPM_POND_OUTLETS", "WDPM_POND_CURVES"]
FILES = ["ponds.csv", "rims.csv", "catchments.csv", "outlets.csv", "curves.csv"]
ALL = dict(zip(UNITS, FILES))
TWO = {"WDPM_DEVICES": "0,0"}
STUB_UNITS = (5, 2, 1)
ARGS = ["add", "dem.asc", "NULL", "out.asc", "NULL", "100", "1.0", "1.0", "0", "0", "0.005", "1000"]


def cases():
    """name -> (STUB_UNITS of the executable, environment).  STUB_TRACE is on everywhere."""
    out = {}

    def add(name, env, units=5):
        assert name not in out
        out[name] = (units, dict(env))

    for n in (3, 1, 0):
        for var, path in ALL.items():
            add(f"alone-{path[:-4]}-n{n}", {var: path, "STUB_N": str(n)})
    add("all-five", ALL)
    add("outlets-with-rims", {u: ALL[u] for u in ("WDPM_POND_OUTLETS", "WDPM_POND_RIMS")})
    add("curves-with-ponds", {u: ALL[u] for u in ("WDPM_POND_CURVES", "WDPM_PONDS")})
    add("curves-with-rims", {u: ALL[u] for u in ("WDPM_POND_CURVES", "WDPM_POND_RIMS")})
    add("empty-is-unset", dict(ALL, WDPM_POND_RIMS="", WDPM_POND_OUTLETS=""))
    add("all-empty", {u: "" for u in UNITS})
    add("min-depth-50", dict(ALL, WDPM_PONDS_MIN_DEPTH_MM="50"))
    add("min-depth-50-two-blocks", dict(TWO, WDPM_PONDS="ponds.csv", WDPM_PONDS_MIN_DEPTH_MM="50"))
    add("two-blocks-ponds", dict(TWO, WDPM_PONDS="ponds.csv"))
    add("two-blocks-ponds-n1", dict(TWO, WDPM_PONDS="ponds.csv", STUB_N="1"))
    add("two-blocks-all-five", dict(TWO, **ALL))
    for var, path in list(ALL.items())[1:]:
        add(f"two-blocks-ponds-{path[:-4]}", dict(TWO, WDPM_PONDS="ponds.csv", **{var: path}))
        add(f"two-blocks-{path[:-4]}", dict(TWO, **{var: path}))
    add("fail-wdpm_ponds_create", dict(ALL, STUB_FAIL="wdpm_ponds_create"))
    for var, sym in zip(UNITS, ("ponds", "rims", "catch", "outlets", "curves")):
        add(f"fail-wdpm_{sym}_label", {var: ALL[var], "STUB_FAIL": f"wdpm_{sym}_label"})
    for sym in ("ponds_table", "rims_table", "catch_table", "catch_stats", "outlets_table", "outlets_stats", "curves_table",
                "curves_stats"):
        add(f"fail-wdpm_{sym}", dict(ALL, STUB_FAIL=f"wdpm_{sym}"))
    for sym in ("create", "label", "stats", "table"):
        add(f"fail-wdpm_group_ponds_{sym}", dict(TWO, WDPM_PONDS="ponds.csv", STUB_FAIL=f"wdpm_group_ponds_{sym}"))
    add("fail-wdpm_ponds_guard_bad", dict(ALL, WDPM_GUARD_KB="4", STUB_FAIL="wdpm_ponds_guard_bad"))
    add("fail-wdpm_group_ponds_guard_bad", dict(TWO, WDPM_PONDS="ponds.csv", WDPM_GUARD_KB="4", STUB_FAIL="wdpm_group_ponds_guard_bad"))
    for var, path in ALL.items():
        add(f"cannot-write-{path[:-4]}", dict(ALL, **{var: "no_such_directory/" + path}))
    for bad in ("0", "5"):
        add(f"guard-{bad}", dict(ALL, WDPM_GUARD_KB="4", STUB_GUARD_BAD=bad))
        add(f"guard-{bad}-two-blocks", dict(TWO, WDPM_PONDS="ponds.csv", WDPM_GUARD_KB="4", STUB_GUARD_BAD=bad))
    add("guard-without-ponds", {"WDPM_GUARD_KB": "4", "STUB_GUARD_BAD": "5"})
    add("units2-all-five", ALL, units=2)
    add("units2-curves", {"WDPM_POND_CURVES": "curves.csv"}, units=2)
    add("units2-two-blocks-all-five", dict(TWO, **ALL), units=2)
    add("units1-ponds-rims", {u: ALL[u] for u in UNITS[:2]}, units=1)
    add("units1-rims", {"WDPM_POND_RIMS": "rims.csv"}, units=1)
    return out


def build(work, units, cli_sources=None):
    """the stand-alone program of tools/asan_cli.sh with the stub beside it; returns its path"""
    exe = os.path.join(str(work), f"WDPMCL_stub{units}")
    subprocess.check_call(
        ["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
         "-ffp-contract=off", f"-DSTUB_UNITS={units}", "-I", CSRC, "-o", exe, *(cli_sources or CLI_SOURCES),
         os.path.join(HERE, "cli_ponds_stub.c"), os.path.join(CSRC, "arcascii.c"), os.path.join(ROOT, "oracle", "wdpm_oracle.c"),
         os.path.join(CSRC, "synth.c"), os.path.join(CSRC, "wdpm_rowblock.c"), "-lpthread", "-lm"])
    return exe


def write_dem(work):
    """the 30 x 40 sine DEM of tests/test_ponds_abi.py"""
    y, x = np.mgrid[0:30, 0:40]
    with open(os.path.join(str(work), "dem.asc"), "w") as f:
        f.write("ncols 40\nnrows 30\nxllcorner 0\nyllcorner 0\ncellsize 10\nNODATA_value -99999\n")
        np.savetxt(f, 500.0 + np.round(np.sin(x / 3.0) * np.cos(y / 4.0), 4), fmt="%.4f")


def run(exe, work, env, leak_check=True):
    """one job in `work` (which holds dem.asc): what is recorded, and beside it the report, the raster and stderr"""
    work = str(work)
    for name in FILES + ["out.asc"]:
        if os.path.exists(os.path.join(work, name)):
            os.remove(os.path.join(work, name))
    base = {k: v for k, v in os.environ.items() if not k.startswith(("WDPM_", "STUB_"))}
    p = subprocess.run([exe] + ARGS, cwd=work, capture_output=True, text=True, timeout=120,
                       env=dict(base, STUB_TRACE="1", ASAN_OPTIONS=f"detect_leaks={int(leak_check)}", **env))
    lines = [ln for ln in p.stderr.splitlines()
             if ln.startswith(("WDPMCL: pond", "WDPMCL: cannot write pond", "WDPMCL: error writing pond", "WDPMCL: guard", "stub:"))]
    files = {name: open(os.path.join(work, name)).read() for name in FILES if os.path.exists(os.path.join(work, name))}
    raster = open(os.path.join(work, "out.asc"), "rb").read() if os.path.exists(os.path.join(work, "out.asc")) else None
    return {"status": p.returncode, "lines": lines, "files": files}, strip_timing(p.stdout), raster, p.stderr


def record(cli_sources, work):
    """every case against the command line built from `cli_sources`.  Recorded without the leak check at exit, which answers a leak
    with an exit status of its own: a command line that ends with status 3 and its rasters still allocated is recorded as status 3.
    The test keeps the check on."""
    write_dem(work)
    exes = {u: build(work, u, cli_sources) for u in STUB_UNITS}
    return {name: run(exes[units], work, env, leak_check=False)[0] for name, (units, env) in cases().items()}
