"""WDPM_POND_ROUTING on the WDPMCL command line: the CSV is the routing table the Python binding takes of the same job, value for
value, and it agrees with the model; WDPM_POND_RUNOFF_MM reaches the label call; set beside the six other pond files it leaves those
byte for byte what they are without it; stdout and the output raster never change; and a raster in two row blocks is refused with
exit status 4 after a run whose own outputs - and whose WDPM_PONDS file - are complete."""
import os
import re
import types

import numpy as np
import pytest

from helpers import pad
from pond_cli import ADD_MM, ITER, job_args, run_cli
from pond_routing_model import assert_same_routing, routing_of_tables, runoff_q_of
from test_pond_curves_cli import small_dem
from test_pond_spills import reference

pytestmark = pytest.mark.gpu
COLUMNS = "label,level,own_q,in_q,kept_q,out_q,out_m3,full,overflows,reach_ponds,reach_cells,reach_area_m2"
MISS = -99999.0
CELLSIZE = 10.0
RUNOFF_MM = 25.0
JOB = job_args("dem.asc")
OTHERS = {"WDPM_PONDS": "ponds.csv", "WDPM_POND_RIMS": "rims.csv", "WDPM_POND_CATCHMENTS": "catch.csv", "WDPM_POND_OUTLETS": "outlets.csv",
          "WDPM_POND_CURVES": "curves.csv", "WDPM_POND_SPILLS": "spills.csv"}


def binding_routing(hip, dem, min_depth, tol, runoff_m):
    """the same job through the Python binding: set-up on the device as the CLI does it, one block, routing of the context; and the
    water it was taken of"""
    from wdpm_amd.ponds import Ponds
    from wdpm_amd.rowblock import Group
    R, Cc = dem.shape
    with Group(hip, "add", R, Cc, MISS, [0]) as grp:
        grp.upload_unpadded(dem, None, op=1, add=ADD_MM / 1000.0, rof=1.0, sub=0.0)
        grp.run_block(ITER, 0.005 / 1000)
        ctx = types.SimpleNamespace(lib=hip, _h=grp.rank_ctx(0), shape=grp.shape)
        with Ponds(ctx) as p:
            p.label_routing(min_depth, runoff_m, tol)
            table, stats = p.routing(), p.routing_stats()
            assert p.guard_bad() == 0
        water = grp.download_water()
    return table, stats, water


def expected_rows(table, cellsize):
    area = cellsize * cellsize
    return [(k + 1, int(t["level"]), int(t["own_q"]), int(t["in_q"]), int(t["kept_q"]), int(t["out_q"]), float(int(t["out_q"])) * 2.0 ** -24 * area,
             int(t["full"]), int(t["overflows"]), int(t["reach_ponds"]), int(t["reach_cells"]), float(int(t["reach_cells"])) * area)
            for k, t in enumerate(table)]


def parse_csv(path):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == COLUMNS
    kinds = (int, int, int, int, int, int, float, int, int, int, int, float)
    return [tuple(k(v) for k, v in zip(kinds, ln.split(","), strict=True)) for ln in lines[1:]]


@pytest.fixture(scope="module")
def job(tmp_path_factory, hip):
    """the small job; the run with none of the variables; the six other files of a run without the new variable"""
    d = tmp_path_factory.mktemp("routing_cli")
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


def said(err, area):
    m = re.search(r"pond routing: (\d+) ponds? written to \S+ \((\S+) mm of runoff: (\d+) full, (\d+) overflowing, (\S+) m3 kept, "
                  r"(\S+) m3 left over land, (\S+) m3 at rings; (\d+) levels\)", err)
    assert m, err
    g = m.groups()
    q = lambda text: round(float(text) / area * 2.0 ** 24)                              # noqa: E731
    return dict(ponds=int(g[0]), runoff_q=round(float(g[1]) / 1000.0 * 2.0 ** 24), full=int(g[2]), overflowing=int(g[3]), kept_q=q(g[4]),
                out_land_q=q(g[5]), out_ring_q=q(g[6]), levels=int(g[7]))


def test_csv_is_the_binding_table_and_nothing_else_changes(hip, job):
    d, plain, before, err_before = job
    dem = np.loadtxt(d / "dem.asc", skiprows=6)                 # as the command line reads it
    table, stats, water = binding_routing(hip, dem, 0.001, 0.0, RUNOFF_MM / 1000.0)
    want = expected_rows(table, CELLSIZE)
    assert len(table) >= 3 and stats["overflowing"] > 0
    # the binding's table is the model's
    bd, _ = pad(dem, np.zeros_like(dem), MISS)
    ref_spills, _, tables = reference(bd, MISS, water, 0.001, 0.0)
    assert_same_routing(table, stats, *routing_of_tables(ref_spills, tables, runoff_q_of(RUNOFF_MM / 1000.0)))
    # alone
    csv = d / "routing.csv"
    out, raster, err = run_cli(d, JOB, WDPM_POND_ROUTING=str(csv), WDPM_POND_RUNOFF_MM=str(RUNOFF_MM))
    assert (out, raster) == plain[:2]
    assert said(err, CELLSIZE ** 2) == {k: stats[k] for k in ("ponds", "runoff_q", "full", "overflowing", "kept_q", "out_land_q", "out_ring_q", "levels")}
    assert not any(os.path.exists(d / f) for f in OTHERS.values())
    got = parse_csv(csv)
    assert got == want, next((a, b) for a, b in zip(got, want) if a != b) if len(got) == len(want) else (len(got), len(want))
    alone = open(csv, "rb").read()
    # beside the other six: one label call serves all seven files, and their stderr lines are what they were
    out, raster, err = run_cli(d, JOB, WDPM_POND_ROUTING=str(csv), WDPM_POND_RUNOFF_MM=str(RUNOFF_MM), **OTHERS)
    assert (out, raster) == plain[:2]
    for k, v in OTHERS.items():
        assert open(d / v, "rb").read() == before[k], k
        os.remove(d / v)
    assert open(csv, "rb").read() == alone
    written = lambda text: [ln for ln in text.splitlines() if ln.startswith("WDPMCL: pond") and "pond routing" not in ln]   # noqa: E731
    assert written(err) == written(err_before) and len(written(err)) == len(OTHERS)
    # beside one of them
    out, raster, err = run_cli(d, JOB, WDPM_POND_ROUTING=str(csv), WDPM_POND_RUNOFF_MM=str(RUNOFF_MM), WDPM_POND_SPILLS="spills.csv")
    assert (out, raster) == plain[:2] and open(d / "spills.csv", "rb").read() == before["WDPM_POND_SPILLS"]
    assert open(csv, "rb").read() == alone
    os.remove(d / "spills.csv")
    # without a depth: no runoff, nothing moves, every pond alone
    out, raster, err = run_cli(d, JOB, WDPM_POND_ROUTING=str(csv))
    rows = parse_csv(csv)
    assert (out, raster) == plain[:2] and len(rows) == len(want) and all(r[2:7] == (0, 0, 0, 0, 0.0) and r[8:10] == (0, 1) for r in rows)
    assert said(err, CELLSIZE ** 2)["runoff_q"] == 0
    os.remove(csv)


def test_two_row_blocks_are_refused_after_a_complete_run(job):
    d, plain, before, _ = job
    out, raster, err = run_cli(d, JOB, status=4, WDPM_DEVICES="0,0", WDPM_POND_ROUTING=str(d / "routing.csv"), WDPM_POND_RUNOFF_MM="25",
                               WDPM_PONDS="ponds.csv")
    assert (out, raster) == plain[:2]
    assert "pond routing" in err and "row blocks" in err and "routing is taken on a whole raster only" in err
    assert not os.path.exists(d / "routing.csv")
    assert open(d / "ponds.csv", "rb").read() == before["WDPM_PONDS"]
    os.remove(d / "ponds.csv")
