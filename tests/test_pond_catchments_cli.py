"""WDPM_POND_CATCHMENTS on the WDPMCL command line: the CSV is the catchment table the Python binding takes of the same job, value
for value (file coordinates, doubles that read back exactly, the area from the cell count); set beside WDPM_PONDS and
WDPM_POND_RIMS it leaves those files byte for byte what they are without it; stdout and the output raster never change; and a
raster in two row blocks is refused with exit status 4 after a run whose own outputs - and whose WDPM_PONDS file - are complete."""
import gzip
import os
import re
import shutil
import types

import pytest

from conftest import GOLDEN
from pond_cli import ADD_MM, ITER, job_args, read_asc, run_cli

pytestmark = pytest.mark.gpu
COLUMNS = "label,catch_cells,catch_area_m2,inflow_cells,head_level_m,row_min,row_max,col_min,col_max"
MISS = -99999.0


def binding_catchments(hip, dem, min_depth):
    """the same job through the Python binding: set-up on the device as the CLI does it, one block, catchments of the context"""
    from wdpm_amd.ponds import Ponds
    from wdpm_amd.rowblock import Group
    R, Cc = dem.shape
    with Group(hip, "add", R, Cc, MISS, [0]) as grp:
        grp.upload_unpadded(dem, None, op=1, add=ADD_MM / 1000.0, rof=1.0, sub=0.0)
        grp.run_block(ITER, 0.005 / 1000)
        ctx = types.SimpleNamespace(lib=hip, _h=grp.rank_ctx(0), shape=grp.shape)
        with Ponds(ctx) as p:
            p.label_catchments(min_depth)
            table, stats = p.catchments(), p.catchment_stats()
            assert p.guard_bad() == 0
    return table, stats


def expected_rows(table, cellsize):
    return [(k + 1, int(t["catch_cells"]), float(int(t["catch_cells"])) * (cellsize * cellsize), int(t["inflow_cells"]),
             float(t["head_level"]), int(t["row_min"]) - 1, int(t["row_max"]) - 1, int(t["col_min"]) - 1, int(t["col_max"]) - 1)
            for k, t in enumerate(table)]


def parse_csv(path):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == COLUMNS
    kinds = (int, int, float, int, float, int, int, int, int)
    return [tuple(k(v) for k, v in zip(kinds, ln.split(","), strict=True)) for ln in lines[1:]]


@pytest.fixture(scope="module")
def job(tmp_path_factory, hip):
    """basin5; the run with none of the variables; the WDPM_PONDS and WDPM_POND_RIMS files of a run without the new variable"""
    d = tmp_path_factory.mktemp("catch_cli")
    with gzip.open(os.path.join(GOLDEN, "basin5.asc.gz"), "rb") as f, open(d / "basin5.asc", "wb") as g:
        shutil.copyfileobj(f, g)
    dem_path = str(d / "basin5.asc")
    plain = run_cli(d, job_args(dem_path))
    ponds_csv, rims_csv = d / "ponds_before.csv", d / "rims_before.csv"
    assert run_cli(d, job_args(dem_path), WDPM_PONDS=str(ponds_csv), WDPM_POND_RIMS=str(rims_csv))[:2] == plain[:2]
    return d, dem_path, plain, open(ponds_csv, "rb").read(), open(rims_csv, "rb").read()


def test_csv_is_the_binding_table_and_nothing_else_changes(hip, job, tmp_path):
    d, dem_path, plain, ponds_before, rims_before = job
    dem, cellsize = read_asc(dem_path)
    table, stats = binding_catchments(hip, dem, 0.001)
    want = expected_rows(table, cellsize)
    assert len(want) >= 1 and any(r[1] > 0 for r in want)
    # alone
    csv = tmp_path / "catch.csv"
    out, raster, err = run_cli(tmp_path, job_args(dem_path), WDPM_POND_CATCHMENTS=str(csv))
    assert (out, raster) == plain[:2] and "pond catchments: %d pond" % len(want) in err
    said = re.search(r"\((\d+) slope cells, (\d+) pits, (\d+) cells drain to no pond, (\d+) rounds\)", err)
    assert said and tuple(map(int, said.groups())) == (stats["slope_cells"], stats["pit_cells"], stats["unponded_cells"], stats["rounds"])
    assert not os.path.exists(tmp_path / "ponds.csv") and not os.path.exists(tmp_path / "rims.csv")
    got = parse_csv(csv)
    assert got == want, next((a, b) for a, b in zip(got, want) if a != b) if len(got) == len(want) else (len(got), len(want))
    alone = open(csv, "rb").read()
    # beside the other two: one label call serves all three files
    out, raster, err = run_cli(tmp_path, job_args(dem_path), WDPM_POND_CATCHMENTS=str(csv), WDPM_POND_RIMS=str(tmp_path / "rims.csv"),
                               WDPM_PONDS=str(tmp_path / "ponds.csv"))
    assert (out, raster) == plain[:2]
    assert open(tmp_path / "ponds.csv", "rb").read() == ponds_before and open(tmp_path / "rims.csv", "rb").read() == rims_before
    assert open(csv, "rb").read() == alone
    # beside one of them
    os.remove(tmp_path / "rims.csv")
    out, raster, err = run_cli(tmp_path, job_args(dem_path), WDPM_POND_CATCHMENTS=str(csv), WDPM_POND_RIMS=str(tmp_path / "rims.csv"))
    assert (out, raster) == plain[:2] and open(tmp_path / "rims.csv", "rb").read() == rims_before and open(csv, "rb").read() == alone


def test_min_depth_variable(hip, job, tmp_path):
    d, dem_path, plain, _, _ = job
    dem, cellsize = read_asc(dem_path)
    csv = tmp_path / "catch.csv"
    run_cli(tmp_path, job_args(dem_path), WDPM_POND_CATCHMENTS=str(csv), WDPM_PONDS_MIN_DEPTH_MM="50")
    assert parse_csv(csv) == expected_rows(binding_catchments(hip, dem, 0.05)[0], cellsize)


def test_two_row_blocks_are_refused_after_a_complete_run(job, tmp_path):
    d, dem_path, plain, ponds_before, _ = job
    out, raster, err = run_cli(tmp_path, job_args(dem_path), status=4, WDPM_DEVICES="0,0", WDPM_POND_CATCHMENTS=str(tmp_path / "catch.csv"),
                               WDPM_PONDS=str(tmp_path / "ponds.csv"))
    assert (out, raster) == plain[:2]
    assert "pond catchments" in err and "row blocks" in err and not os.path.exists(tmp_path / "catch.csv")
    assert open(tmp_path / "ponds.csv", "rb").read() == ponds_before
