"""WDPM_POND_CURVES on the WDPMCL command line: the CSV is the curve table the Python binding takes of the same job, value for value
(one line `stage 0` per pond and sixteen more where it has an outlet, levels from the library's own stage rule, doubles that read
back exactly, area and volume from the counts), and it agrees with the numpy model; set beside WDPM_PONDS, WDPM_POND_RIMS,
WDPM_POND_CATCHMENTS and WDPM_POND_OUTLETS it leaves those files byte for byte what they are without it; stdout and the output
raster never change; and a raster in two row blocks is refused with exit status 4 after a run whose own outputs - and whose
WDPM_PONDS file - are complete."""
import os
import re
import types

import numpy as np
import pytest

from helpers import pad
from pond_curves_model import STAGES, assert_same_curves
from test_pond_curves import reference
from pond_cli import ADD_MM, ITER, job_args, run_cli

pytestmark = pytest.mark.gpu
COLUMNS = "label,stage,level_m,cells,area_m2,q,volume_m3"
MISS = -99999.0
CELLSIZE = 10.0
JOB = job_args("dem.asc")
OTHERS = {"WDPM_PONDS": "ponds.csv", "WDPM_POND_RIMS": "rims.csv", "WDPM_POND_CATCHMENTS": "catch.csv", "WDPM_POND_OUTLETS": "outlets.csv"}


def small_dem():
    """60 x 150: hollows a dozen cells across on a tilted plane, in steps of 0.1 mm"""
    y, x = np.mgrid[0:60, 0:150]
    return np.round(500.0 + 2.0 * np.sin(x / 7.0) * np.cos(y / 6.0) + 0.004 * x, 4)


def binding_curves(hip, dem, min_depth):
    """the same job through the Python binding: set-up on the device as the CLI does it, one block, curves of the context; and the
    water they were taken of"""
    from wdpm_amd.ponds import Ponds
    from wdpm_amd.rowblock import Group
    R, Cc = dem.shape
    with Group(hip, "add", R, Cc, MISS, [0]) as grp:
        grp.upload_unpadded(dem, None, op=1, add=ADD_MM / 1000.0, rof=1.0, sub=0.0)
        grp.run_block(ITER, 0.005 / 1000)
        ctx = types.SimpleNamespace(lib=hip, _h=grp.rank_ctx(0), shape=grp.shape)
        with Ponds(ctx) as p:
            p.label_curves(min_depth)
            table, stats = p.curves(), p.curve_stats()
            assert p.guard_bad() == 0
        water = grp.download_water()
    return table, stats, water


def expected_rows(hip, table, cellsize):
    from wdpm_amd.ponds import stage_levels
    area = cellsize * cellsize
    rows = []
    for k, t in enumerate(table):
        rows.append((k + 1, 0, float(t["bed_level"]), 0, 0.0, 0, 0.0))
        if not np.isfinite(t["top_level"]):
            continue
        levels = stage_levels(t["bed_level"], t["top_level"], hip)
        for s in range(1, STAGES + 1):
            rows.append((k + 1, s, float(levels[s]), int(t["cells"][s - 1]), float(int(t["cells"][s - 1])) * area, int(t["q"][s - 1]),
                         float(int(t["q"][s - 1])) * 2.0 ** -24 * area))
    return rows


def parse_csv(path):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == COLUMNS
    kinds = (int, int, float, int, float, int, float)
    return [tuple(k(v) for k, v in zip(kinds, ln.split(","), strict=True)) for ln in lines[1:]]


@pytest.fixture(scope="module")
def job(tmp_path_factory, hip):
    """the small job; the run with none of the variables; the four other files of a run without the new variable"""
    d = tmp_path_factory.mktemp("curves_cli")
    with open(d / "dem.asc", "w") as f:
        f.write("ncols 150\nnrows 60\nxllcorner 0\nyllcorner 0\ncellsize %g\nNODATA_value %d\n" % (CELLSIZE, int(MISS)))
        np.savetxt(f, small_dem(), fmt="%.4f")
    plain = run_cli(d, JOB)
    assert run_cli(d, JOB, **OTHERS)[:2] == plain[:2]
    before = {k: open(d / v, "rb").read() for k, v in OTHERS.items()}
    for v in OTHERS.values():
        os.remove(d / v)
    return d, plain, before


def test_csv_is_the_binding_table_and_nothing_else_changes(hip, job):
    d, plain, before = job
    dem = np.loadtxt(d / "dem.asc", skiprows=6)                 # as the command line reads it
    assert dem.shape == (60, 150)
    table, stats, water = binding_curves(hip, dem, 0.001)
    want = expected_rows(hip, table, CELLSIZE)
    assert len(table) >= 3 and len(want) > len(table) and stats["stage_cells"] > 0
    # the binding's table is the model's
    bd, _ = pad(dem, np.zeros_like(dem), MISS)
    _, _, ref_table, ref_stats = reference(bd, MISS, water, 0.001)
    assert_same_curves(table, stats, ref_table, ref_stats)
    # alone
    csv = d / "curves.csv"
    out, raster, err = run_cli(d, JOB, WDPM_POND_CURVES=str(csv))
    assert (out, raster) == plain[:2] and "pond curves: %d pond" % len(table) in err
    said = re.search(r"\((\d+) without a curve, (\d+) flat, (\d+) cells below the last stage\)", err)
    assert said and tuple(map(int, said.groups())) == (stats["no_curve"], stats["flat"], stats["stage_cells"])
    assert not any(os.path.exists(d / f) for f in OTHERS.values())
    got = parse_csv(csv)
    assert got == want, next((a, b) for a, b in zip(got, want) if a != b) if len(got) == len(want) else (len(got), len(want))
    alone = open(csv, "rb").read()
    # beside the other four: one label call serves all five files
    out, raster, err = run_cli(d, JOB, WDPM_POND_CURVES=str(csv), **OTHERS)
    assert (out, raster) == plain[:2]
    for k, v in OTHERS.items():
        assert open(d / v, "rb").read() == before[k], k
        os.remove(d / v)
    assert open(csv, "rb").read() == alone
    # beside one of them
    out, raster, err = run_cli(d, JOB, WDPM_POND_CURVES=str(csv), WDPM_POND_RIMS="rims.csv")
    assert (out, raster) == plain[:2] and open(d / "rims.csv", "rb").read() == before["WDPM_POND_RIMS"]
    assert open(csv, "rb").read() == alone
    os.remove(d / "rims.csv")
    os.remove(csv)


def test_two_row_blocks_are_refused_after_a_complete_run(job):
    d, plain, before = job
    out, raster, err = run_cli(d, JOB, status=4, WDPM_DEVICES="0,0", WDPM_POND_CURVES=str(d / "curves.csv"), WDPM_PONDS="ponds.csv")
    assert (out, raster) == plain[:2]
    assert "pond curves" in err and "row blocks" in err and not os.path.exists(d / "curves.csv")
    assert open(d / "ponds.csv", "rb").read() == before["WDPM_PONDS"]
    os.remove(d / "ponds.csv")
