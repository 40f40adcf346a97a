"""WDPM_POND_RIMS on the WDPMCL command line: the CSV is the rim table the Python binding takes of the same job, field for field
(file coordinates, doubles that read back exactly, the freeboard taken from them); set beside WDPM_PONDS it leaves that file
byte for byte what it is alone; stdout and the output raster never change; and a raster in two row blocks is refused with exit
status 4 after a run whose own outputs - and whose WDPM_PONDS file - are complete."""
import gzip
import os
import shutil
import types

import pytest

from conftest import GOLDEN
from pond_cli import ADD_MM, ITER, job_args, read_asc, run_cli

pytestmark = pytest.mark.gpu
COLUMNS = "label,surface_min_m,surface_max_m,rim_level_m,freeboard_m,rim_row,rim_col,rim_cells,wall_cells"
MISS = -99999.0


def binding_rims(hip, dem, min_depth):
    """the same job through the Python binding: set-up on the device as the CLI does it, one block, rims of the context"""
    from wdpm_amd.ponds import Ponds
    from wdpm_amd.rowblock import Group
    R, Cc = dem.shape
    with Group(hip, "add", R, Cc, MISS, [0]) as grp:
        grp.upload_unpadded(dem, None, op=1, add=ADD_MM / 1000.0, rof=1.0, sub=0.0)
        grp.run_block(ITER, 0.005 / 1000)
        ctx = types.SimpleNamespace(lib=hip, _h=grp.rank_ctx(0), shape=grp.shape)
        with Ponds(ctx) as p:
            p.label_rims(min_depth)
            table = p.rims()
            assert p.guard_bad() == 0
    return table


def expected_rows(table):
    rows = []
    for k, t in enumerate(table):
        none = int(t["rim_row"]) < 0
        rows.append((k + 1, float(t["surface_min"]), float(t["surface_max"]), float(t["rim_level"]),
                     float(t["rim_level"]) - float(t["surface_max"]), -1 if none else int(t["rim_row"]) - 1,
                     -1 if none else int(t["rim_col"]) - 1, int(t["rim_cells"]), int(t["wall_cells"])))
    return rows


def parse_csv(path):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == COLUMNS
    kinds = (int, float, float, float, float, int, int, int, int)
    return [tuple(k(v) for k, v in zip(kinds, ln.split(","), strict=True)) for ln in lines[1:]]


@pytest.fixture(scope="module")
def job(tmp_path_factory, hip):
    """basin5, the run with neither variable, and the rim table of the binding at the default threshold"""
    d = tmp_path_factory.mktemp("rims_cli")
    with gzip.open(os.path.join(GOLDEN, "basin5.asc.gz"), "rb") as f, open(d / "basin5.asc", "wb") as g:
        shutil.copyfileobj(f, g)
    dem_path = str(d / "basin5.asc")
    plain = run_cli(d, job_args(dem_path))
    ponds_alone = d / "ponds_alone.csv"
    assert run_cli(d, job_args(dem_path), WDPM_PONDS=str(ponds_alone))[:2] == plain[:2]
    return d, dem_path, plain, open(ponds_alone, "rb").read()


def test_csv_is_the_binding_table_and_nothing_else_changes(hip, job, tmp_path):
    d, dem_path, plain, ponds_alone = job
    want = expected_rows(binding_rims(hip, read_asc(dem_path)[0], 0.001))
    assert len(want) >= 1 and any(r[7] > 0 for r in want)
    # alone
    csv = tmp_path / "rims.csv"
    out, raster, err = run_cli(tmp_path, job_args(dem_path), WDPM_POND_RIMS=str(csv))
    assert (out, raster) == plain[:2] and "pond rims: %d pond" % len(want) in err
    assert not os.path.exists(tmp_path / "ponds.csv")
    got = parse_csv(csv)
    assert got == want, next((a, b) for a, b in zip(got, want) if a != b) if len(got) == len(want) else (len(got), len(want))
    alone = open(csv, "rb").read()
    # beside WDPM_PONDS: one label call serves both files
    out, raster, err = run_cli(tmp_path, job_args(dem_path), WDPM_POND_RIMS=str(csv), WDPM_PONDS=str(tmp_path / "ponds.csv"))
    assert (out, raster) == plain[:2]
    assert open(tmp_path / "ponds.csv", "rb").read() == ponds_alone and open(csv, "rb").read() == alone


def test_min_depth_variable(hip, job, tmp_path):
    d, dem_path, plain, _ = job
    csv = tmp_path / "rims.csv"
    run_cli(tmp_path, job_args(dem_path), WDPM_POND_RIMS=str(csv), WDPM_PONDS_MIN_DEPTH_MM="50")
    assert parse_csv(csv) == expected_rows(binding_rims(hip, read_asc(dem_path)[0], 0.05))


def test_two_row_blocks_are_refused_after_a_complete_run(job, tmp_path):
    d, dem_path, plain, ponds_alone = job
    out, raster, err = run_cli(tmp_path, job_args(dem_path), status=4, WDPM_DEVICES="0,0", WDPM_POND_RIMS=str(tmp_path / "rims.csv"),
                               WDPM_PONDS=str(tmp_path / "ponds.csv"))
    assert (out, raster) == plain[:2]
    assert "pond rims" in err and "row blocks" in err and not os.path.exists(tmp_path / "rims.csv")
    assert open(tmp_path / "ponds.csv", "rb").read() == ponds_alone
