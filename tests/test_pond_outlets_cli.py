"""WDPM_POND_OUTLETS on the WDPMCL command line: the CSV is the outlet table the Python binding takes of the same job, value for
value (file coordinates, doubles that read back exactly, the headroom from the rim table's highest surface, area and volume from
the counts); set beside WDPM_PONDS, WDPM_POND_RIMS and WDPM_POND_CATCHMENTS it leaves those files byte for byte what they are
without it; stdout and the output raster never change; and a raster in two row blocks is refused with exit status 4 after a run
whose own outputs - and whose WDPM_PONDS file - are complete."""
import gzip
import os
import re
import shutil
import types

import pytest

from conftest import GOLDEN
from pond_cli import ADD_MM, ITER, job_args, read_asc, run_cli

pytestmark = pytest.mark.gpu
COLUMNS = "label,pour_level_m,headroom_m,from_row,from_col,to_row,to_col,to_label,divide_cells,fill_cells,fill_area_m2,fill_q,fill_m3"
MISS = -99999.0


def binding_outlets(hip, dem, min_depth):
    """the same job through the Python binding: set-up on the device as the CLI does it, one block, outlets of the context"""
    from wdpm_amd.ponds import Ponds
    from wdpm_amd.rowblock import Group
    R, Cc = dem.shape
    with Group(hip, "add", R, Cc, MISS, [0]) as grp:
        grp.upload_unpadded(dem, None, op=1, add=ADD_MM / 1000.0, rof=1.0, sub=0.0)
        grp.run_block(ITER, 0.005 / 1000)
        ctx = types.SimpleNamespace(lib=hip, _h=grp.rank_ctx(0), shape=grp.shape)
        with Ponds(ctx) as p:
            p.label_outlets(min_depth)
            table, rims, stats = p.outlets(), p.rims(), p.outlet_stats()
            assert p.guard_bad() == 0
    return table, rims, stats


def expected_rows(table, rims, cellsize):
    area = cellsize * cellsize
    rows = []
    for k, (t, r) in enumerate(zip(table, rims)):
        none = int(t["from_row"]) < 0
        coords = (-1, -1, -1, -1) if none else tuple(int(t[n]) - 1 for n in ("from_row", "from_col", "to_row", "to_col"))
        rows.append((k + 1, float(t["pour_level"]), float(t["pour_level"]) - float(r["surface_max"])) + coords +
                    (int(t["to_basin"]), int(t["divide_cells"]), int(t["fill_cells"]), float(int(t["fill_cells"])) * area,
                     int(t["fill_q"]), float(int(t["fill_q"])) * 2.0 ** -24 * area))
    return rows


def parse_csv(path):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == COLUMNS
    kinds = (int, float, float, int, int, int, int, int, int, int, float, int, float)
    return [tuple(k(v) for k, v in zip(kinds, ln.split(","), strict=True)) for ln in lines[1:]]


@pytest.fixture(scope="module")
def job(tmp_path_factory, hip):
    """basin5; the run with none of the variables; the three other files of a run without the new variable"""
    d = tmp_path_factory.mktemp("outlets_cli")
    with gzip.open(os.path.join(GOLDEN, "basin5.asc.gz"), "rb") as f, open(d / "basin5.asc", "wb") as g:
        shutil.copyfileobj(f, g)
    dem_path = str(d / "basin5.asc")
    plain = run_cli(d, job_args(dem_path))
    before = {"WDPM_PONDS": d / "ponds_before.csv", "WDPM_POND_RIMS": d / "rims_before.csv", "WDPM_POND_CATCHMENTS": d / "catch_before.csv"}
    assert run_cli(d, job_args(dem_path), **{k: str(v) for k, v in before.items()})[:2] == plain[:2]
    return d, dem_path, plain, {k: open(v, "rb").read() for k, v in before.items()}


def test_csv_is_the_binding_table_and_nothing_else_changes(hip, job, tmp_path):
    d, dem_path, plain, before = job
    dem, cellsize = read_asc(dem_path)
    table, rims, stats = binding_outlets(hip, dem, 0.001)
    want = expected_rows(table, rims, cellsize)
    assert len(want) >= 1 and any(r[3] >= 0 for r in want)
    # alone
    csv = tmp_path / "outlets.csv"
    out, raster, err = run_cli(tmp_path, job_args(dem_path), WDPM_POND_OUTLETS=str(csv))
    assert (out, raster) == plain[:2] and "pond outlets: %d pond" % len(want) in err
    said = re.search(r"\((\d+) without an outlet, (\d+) spill onto land that ends in a pit, (\d+) cells on the divides\)", err)
    assert said and tuple(map(int, said.groups())) == (stats["no_outlet"], stats["to_land"], stats["divide_cells"])
    assert not any(os.path.exists(tmp_path / f) for f in ("ponds.csv", "rims.csv", "catch.csv"))
    got = parse_csv(csv)
    assert got == want, next((a, b) for a, b in zip(got, want) if a != b) if len(got) == len(want) else (len(got), len(want))
    alone = open(csv, "rb").read()
    # beside the other three: one label call serves all four files
    others = {"WDPM_PONDS": tmp_path / "ponds.csv", "WDPM_POND_RIMS": tmp_path / "rims.csv", "WDPM_POND_CATCHMENTS": tmp_path / "catch.csv"}
    out, raster, err = run_cli(tmp_path, job_args(dem_path), WDPM_POND_OUTLETS=str(csv), **{k: str(v) for k, v in others.items()})
    assert (out, raster) == plain[:2]
    for k, v in others.items():
        assert open(v, "rb").read() == before[k], k
    assert open(csv, "rb").read() == alone
    # beside one of them
    os.remove(others["WDPM_POND_RIMS"])
    out, raster, err = run_cli(tmp_path, job_args(dem_path), WDPM_POND_OUTLETS=str(csv), WDPM_POND_RIMS=str(others["WDPM_POND_RIMS"]))
    assert (out, raster) == plain[:2] and open(others["WDPM_POND_RIMS"], "rb").read() == before["WDPM_POND_RIMS"]
    assert open(csv, "rb").read() == alone


def test_min_depth_variable(hip, job, tmp_path):
    d, dem_path, plain, _ = job
    dem, cellsize = read_asc(dem_path)
    csv = tmp_path / "outlets.csv"
    run_cli(tmp_path, job_args(dem_path), WDPM_POND_OUTLETS=str(csv), WDPM_PONDS_MIN_DEPTH_MM="50")
    table, rims, _ = binding_outlets(hip, dem, 0.05)
    assert parse_csv(csv) == expected_rows(table, rims, cellsize)


def test_two_row_blocks_are_refused_after_a_complete_run(job, tmp_path):
    d, dem_path, plain, before = job
    out, raster, err = run_cli(tmp_path, job_args(dem_path), status=4, WDPM_DEVICES="0,0", WDPM_POND_OUTLETS=str(tmp_path / "outlets.csv"),
                               WDPM_PONDS=str(tmp_path / "ponds.csv"))
    assert (out, raster) == plain[:2]
    assert "pond outlets" in err and "row blocks" in err and not os.path.exists(tmp_path / "outlets.csv")
    assert open(tmp_path / "ponds.csv", "rb").read() == before["WDPM_PONDS"]
