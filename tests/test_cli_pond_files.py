"""The command line's pond files, locked on the CPU: wdpmcl_main.c and wdpmcl_ponds.c linked with a canned pond back-end
(tests/cli_ponds_stub.c) and the CPU restatement into a stand-alone program under AddressSanitizer and UBSan, run as a child
process on the cases of tests/cli_pond_cases.py.  Every case is held against tests/golden/cli_pond_files.json, recorded by
tests/golden/make_golden.py from the command line as it was before the pond files became one table of units: the exit status, the
files byte for byte, and the pond, guard and stub lines of stderr in order - which label call is made, which tables and statistics
are fetched, what is said and in which order.  The report on stdout and the output raster never depend on a pond variable."""
import json
import os

import pytest

import cli_pond_cases as cpc
from conftest import GOLDEN

CASES = cpc.cases()
RECORDED = json.load(open(os.path.join(GOLDEN, "cli_pond_files.json")))


@pytest.fixture(scope="module")
def stand(tmp_path_factory):
    """the three executables, the DEM and the run with no variable set"""
    work = tmp_path_factory.mktemp("cli_pond_files")
    cpc.write_dem(work)
    exes = {units: cpc.build(work, units) for units in cpc.STUB_UNITS}
    got, report, raster, err = cpc.run(exes[5], work, {})
    assert got == {"status": 0, "lines": [], "files": {}} and raster, err
    return work, exes, report, raster


def test_the_recording_covers_the_cases():
    assert sorted(RECORDED) == sorted(CASES)
    # every unit alone at 3, 1 and 0 ponds; all five together write what each writes alone
    for n in (3, 1, 0):
        for name in cpc.FILES:
            rec = RECORDED[f"alone-{name[:-4]}-n{n}"]
            assert rec["status"] == 0 and list(rec["files"]) == [name]
            assert rec["files"][name].count("\n") == 1 + (n if name != "curves.csv" else {0: 0, 1: 17, 3: 35}[n])
    assert RECORDED["all-five"]["files"] == {name: RECORDED[f"alone-{name[:-4]}-n3"]["files"][name] for name in cpc.FILES}
    assert "inf" in RECORDED["all-five"]["files"]["rims.csv"] and ",-1,-1," in RECORDED["all-five"]["files"]["outlets.csv"]
    assert "-inf" in RECORDED["all-five"]["files"]["catchments.csv"]
    # the quanta above 2^53: the integer column and the cubic metres differ in what they keep
    assert ",1152921504606859321," in RECORDED["all-five"]["files"]["ponds.csv"]
    assert any("min_depth=0.050000000000000003" in ln for ln in RECORDED["min-depth-50"]["lines"])
    assert any("min_depth=0.001" in ln for ln in RECORDED["all-five"]["lines"])
    assert RECORDED["two-blocks-ponds"]["lines"][-1].endswith("(2 row blocks, 7 joined across them)")
    for name, rec in RECORDED.items():
        if name.startswith("fail-"):
            assert rec["status"] == 4 and not rec["files"], name
            assert sum("failed, no file written: " + name[5:] + " failed" in ln for ln in rec["lines"]) == 1, name
        if name.startswith("cannot-write-"):
            assert rec["status"] == 4 and sorted(rec["files"]) == sorted(set(cpc.FILES) - {name[13:] + ".csv"}), name
            assert sum("cannot write" in ln for ln in rec["lines"]) == 1, name
    assert [RECORDED[f"guard-{k}"]["status"] for k in ("0", "0-two-blocks", "5", "5-two-blocks")] == [0, 0, 3, 3]
    none = [ln for ln in RECORDED["units2-all-five"]["lines"] if "has none" in ln]
    assert [ln.split(":")[1].strip() for ln in none] == ["pond catchments", "pond outlets", "pond curves"]
    assert RECORDED["units2-all-five"]["status"] == 4 and sorted(RECORDED["units2-all-five"]["files"]) == ["ponds.csv", "rims.csv"]
    assert RECORDED["units1-ponds-rims"]["status"] == 4 and list(RECORDED["units1-ponds-rims"]["files"]) == ["ponds.csv"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_matches_the_recording(stand, name):
    work, exes, report, raster = stand
    units, env = CASES[name]
    got, got_report, got_raster, err = cpc.run(exes[units], work, env)
    print(err)
    assert "ERROR" not in err and "runtime error" not in err
    assert got["status"] == RECORDED[name]["status"]
    assert got["lines"] == RECORDED[name]["lines"]
    assert got["files"] == RECORDED[name]["files"]
    if got["status"] == 3:     # overwritten guard bands end the run before its summary
        assert got_raster is None and report.startswith(got_report) and "WDPM run summary" not in got_report
    else:
        assert got_report == report and got_raster == raster
