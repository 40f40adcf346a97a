"""WDPM_POND_SPILLS on the WDPMCL command line: the CSV is the spill table the Python binding takes of the same job, value for value
(labels and counts as they are, areas and volumes from the counts, doubles that read back exactly), and it agrees with the model;
WDPM_POND_HEADROOM_MM reaches the label call; set beside WDPM_PONDS, WDPM_POND_RIMS, WDPM_POND_CATCHMENTS, WDPM_POND_OUTLETS and
WDPM_POND_CURVES it leaves those five files byte for byte what they are without it; stdout and the output raster never change; and a
raster in two row blocks is refused with exit status 4 after a run whose own outputs - and whose WDPM_PONDS file - are complete."""
import os
import re
import types

import numpy as np
import pytest

from helpers import pad
from pond_cli import ADD_MM, ITER, job_args, run_cli
from pond_spills_model import assert_same_spills
from test_pond_curves_cli import small_dem
from test_pond_spills import reference

pytestmark = pytest.mark.gpu
COLUMNS = ("label,next_label,spilling,sink_label,end,hops,path_fill_q,path_fill_m3,up_ponds,up_cells,up_area_m2,up_fill_q,up_fill_m3,"
           "rest_label,rest_hops,live_ponds,live_cells,live_area_m2")
MISS = -99999.0
CELLSIZE = 10.0
JOB = job_args("dem.asc")
OTHERS = {"WDPM_PONDS": "ponds.csv", "WDPM_POND_RIMS": "rims.csv", "WDPM_POND_CATCHMENTS": "catch.csv", "WDPM_POND_OUTLETS": "outlets.csv",
          "WDPM_POND_CURVES": "curves.csv"}


def binding_spills(hip, dem, min_depth, tol):
    """the same job through the Python binding: set-up on the device as the CLI does it, one block, spills of the context; and the
    water they were taken of"""
    from wdpm_amd.ponds import Ponds
    from wdpm_amd.rowblock import Group
    R, Cc = dem.shape
    with Group(hip, "add", R, Cc, MISS, [0]) as grp:
        grp.upload_unpadded(dem, None, op=1, add=ADD_MM / 1000.0, rof=1.0, sub=0.0)
        grp.run_block(ITER, 0.005 / 1000)
        ctx = types.SimpleNamespace(lib=hip, _h=grp.rank_ctx(0), shape=grp.shape)
        with Ponds(ctx) as p:
            p.label_spills(min_depth, tol)
            table, stats = p.spills(), p.spill_stats()
            assert p.guard_bad() == 0
        water = grp.download_water()
    return table, stats, water


def expected_rows(table, cellsize):
    area = cellsize * cellsize
    q = lambda v: float(int(v)) * 2.0 ** -24 * area                                    # noqa: E731
    return [(k + 1, int(t["next"]), int(t["spilling"]), int(t["sink"]), int(t["end"]), int(t["hops"]), int(t["path_fill_q"]),
             q(t["path_fill_q"]), int(t["up_ponds"]), int(t["up_cells"]), float(int(t["up_cells"])) * area, int(t["up_fill_q"]),
             q(t["up_fill_q"]), int(t["rest"]), int(t["rest_hops"]), int(t["live_ponds"]), int(t["live_cells"]),
             float(int(t["live_cells"])) * area) for k, t in enumerate(table)]


def parse_csv(path):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == COLUMNS
    kinds = (int, int, int, int, int, int, int, float, int, int, float, int, float, int, int, int, int, float)
    return [tuple(k(v) for k, v in zip(kinds, ln.split(","), strict=True)) for ln in lines[1:]]


@pytest.fixture(scope="module")
def job(tmp_path_factory, hip):
    """the small job; the run with none of the variables; the five other files of a run without the new variable"""
    d = tmp_path_factory.mktemp("spills_cli")
    with open(d / "dem.asc", "w") as f:
        f.write("ncols 150\nnrows 60\nxllcorner 0\nyllcorner 0\ncellsize %g\nNODATA_value %d\n" % (CELLSIZE, int(MISS)))
        np.savetxt(f, small_dem(), fmt="%.4f")
    plain = run_cli(d, JOB)
    out, raster, err = run_cli(d, JOB, **OTHERS)
    assert (out, raster) == plain[:2]
    before = {k: open(d / v, "rb").read() for k, v in OTHERS.items()}
    for v in OTHERS.values():
        os.remove(d / v)
    return d, plain, before, err


def said(err):
    m = re.search(r"pond spills: (\d+) ponds? written to \S+ \((\d+) rings of (\d+) ponds, (\d+) spilling, chains end: (\d+) on land, "
                  r"(\d+) without an outlet, (\d+) at a ring; longest chain (\d+)\)", err)
    assert m, err
    return dict(zip(("ponds", "rings", "ring_ponds", "spilling", "ends_land", "ends_none", "ends_ring", "max_hops"), map(int, m.groups())))


def test_csv_is_the_binding_table_and_nothing_else_changes(hip, job):
    d, plain, before, err_before = job
    dem = np.loadtxt(d / "dem.asc", skiprows=6)                 # as the command line reads it
    assert dem.shape == (60, 150)
    table, stats, water = binding_spills(hip, dem, 0.001, 0.0)
    want = expected_rows(table, CELLSIZE)
    assert len(table) >= 3
    # the binding's table is the model's
    bd, _ = pad(dem, np.zeros_like(dem), MISS)
    ref_table, ref_stats, _ = reference(bd, MISS, water, 0.001, 0.0)
    assert_same_spills(table, stats, ref_table, ref_stats)
    # alone
    csv = d / "spills.csv"
    out, raster, err = run_cli(d, JOB, WDPM_POND_SPILLS=str(csv))
    assert (out, raster) == plain[:2]
    assert said(err) == {k: v for k, v in stats.items() if k != "rounds"}
    assert not any(os.path.exists(d / f) for f in OTHERS.values())
    got = parse_csv(csv)
    assert got == want, next((a, b) for a, b in zip(got, want) if a != b) if len(got) == len(want) else (len(got), len(want))
    alone = open(csv, "rb").read()
    # beside the other five: one label call serves all six files, and their stderr lines are what they were
    out, raster, err = run_cli(d, JOB, WDPM_POND_SPILLS=str(csv), **OTHERS)
    assert (out, raster) == plain[:2]
    for k, v in OTHERS.items():
        assert open(d / v, "rb").read() == before[k], k
        os.remove(d / v)
    assert open(csv, "rb").read() == alone
    written = lambda text: [ln for ln in text.splitlines() if ln.startswith("WDPMCL: pond") and "pond spills" not in ln]   # noqa: E731
    assert written(err) == written(err_before) and len(written(err)) == len(OTHERS)
    # beside one of them
    out, raster, err = run_cli(d, JOB, WDPM_POND_SPILLS=str(csv), WDPM_POND_RIMS="rims.csv")
    assert (out, raster) == plain[:2] and open(d / "rims.csv", "rb").read() == before["WDPM_POND_RIMS"]
    assert open(csv, "rb").read() == alone
    os.remove(d / "rims.csv")
    os.remove(csv)


def test_headroom_is_honoured(hip, job):
    """a tolerance of 200 mm makes more ponds spill than none: the file is the binding's table at that tolerance, and differs"""
    d, plain, before, _ = job
    dem = np.loadtxt(d / "dem.asc", skiprows=6)
    strict, strict_stats, _ = binding_spills(hip, dem, 0.001, 0.0)
    table, stats, _ = binding_spills(hip, dem, 0.001, 0.2)
    assert stats["spilling"] > strict_stats["spilling"], "the job must have a pond within 200 mm of its pour level"
    csv = d / "spills.csv"
    out, raster, err = run_cli(d, JOB, WDPM_POND_SPILLS=str(csv), WDPM_POND_HEADROOM_MM="200")
    assert (out, raster) == plain[:2] and said(err)["spilling"] == stats["spilling"]
    assert parse_csv(csv) == expected_rows(table, CELLSIZE) != expected_rows(strict, CELLSIZE)
    os.remove(csv)


def test_two_row_blocks_are_refused_after_a_complete_run(job):
    d, plain, before, _ = job
    out, raster, err = run_cli(d, JOB, status=4, WDPM_DEVICES="0,0", WDPM_POND_SPILLS=str(d / "spills.csv"), WDPM_PONDS="ponds.csv")
    assert (out, raster) == plain[:2]
    assert "pond spills" in err and "row blocks" in err and "spills are taken on a whole raster only" in err
    assert not os.path.exists(d / "spills.csv")
    assert open(d / "ponds.csv", "rb").read() == before["WDPM_PONDS"]
    os.remove(d / "ponds.csv")
