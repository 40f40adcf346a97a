"""WDPM_PONDS on the WDPMCL command line: the CSV is the inventory the Python binding takes of the same job, field for field, and
the variable changes nothing else - stdout and the output raster stay byte-identical to a run without it.  On one device (the
handle sits on the group's only context) and with WDPM_DEVICES=0,0 (two row blocks: the CLI keeps the unmasked depths and
labels them in one whole-raster context after the group is gone)."""
import gzip
import os
import re
import shutil
import types

import numpy as np
import pytest

from conftest import GOLDEN
from pond_cli import ADD_MM, ITER, job_args, read_asc, run_cli

pytestmark = pytest.mark.gpu
COLUMNS = "label,row,col,cells,area_m2,volume_q,volume_m3,max_depth_m,row_min,row_max,col_min,col_max"
MISS = -99999.0


def binding_inventory(hip, dem, min_depth):
    """the same job through the Python binding: set-up on the device as the CLI does it, one block, inventory of the context"""
    from wdpm_amd.ponds import Ponds
    from wdpm_amd.rowblock import Group
    R, Cc = dem.shape
    with Group(hip, "add", R, Cc, MISS, [0]) as grp:
        grp.upload_unpadded(dem, None, op=1, add=ADD_MM / 1000.0, rof=1.0, sub=0.0)
        grp.run_block(ITER, 0.005 / 1000)
        wet = grp.count_stats()[1]
        ctx = types.SimpleNamespace(lib=hip, _h=grp.rank_ctx(0), shape=grp.shape)
        with Ponds(ctx) as p:
            p.label(min_depth)
            table = p.table()
            assert p.guard_bad() == 0
    return table, wet


def expected_rows(table, cellsize):
    area = cellsize * cellsize
    rows = []
    for k, t in enumerate(table):
        q = int(t["volume_q"])
        rows.append((k + 1, int(t["first_row"]) - 1, int(t["first_col"]) - 1, int(t["cells"]), float(int(t["cells"])) * area, q,
                     float(q) * 2.0 ** -24 * area, float(t["max_depth"]), int(t["row_min"]) - 1, int(t["row_max"]) - 1,
                     int(t["col_min"]) - 1, int(t["col_max"]) - 1))
    return rows


def parse_csv(path):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == COLUMNS
    kinds = (int, int, int, int, float, int, float, float, int, int, int, int)
    return [tuple(k(v) for k, v in zip(kinds, ln.split(","), strict=True)) for ln in lines[1:]]


@pytest.fixture(scope="module")
def rasters(tmp_path_factory, hip):
    d = tmp_path_factory.mktemp("ponds_cli")
    with gzip.open(os.path.join(GOLDEN, "basin5.asc.gz"), "rb") as f, open(d / "basin5.asc", "wb") as g:
        shutil.copyfileobj(f, g)
    dem = hip.synth_dem(900, 77)[:600, :].copy()
    dem[100:130, 400:470] = MISS
    with open(d / "synth.asc", "w") as f:
        f.write(f"ncols 900\nnrows 600\nxllcorner 0\nyllcorner 0\ncellsize 2.5\nNODATA_value {MISS:.0f}\n")
        np.savetxt(f, dem, fmt="%.4f")
    return d


@pytest.mark.parametrize("name", ["basin5", "synth"])
def test_csv_is_the_binding_inventory_and_nothing_else_changes(hip, rasters, name, tmp_path):
    dem_path = str(rasters / f"{name}.asc")
    dem, cellsize = read_asc(dem_path)
    want, wet = binding_inventory(hip, dem, 0.001)
    want = expected_rows(want, cellsize)
    assert len(want) >= 1 and sum(r[3] for r in want) == wet          # the default threshold is the reference's wet threshold
    plain = run_cli(tmp_path, job_args(dem_path))
    assert not os.path.exists(tmp_path / "ponds.csv")
    for tag, devices in (("one", {}), ("two", {"WDPM_DEVICES": "0,0"})):
        csv = tmp_path / f"ponds_{tag}.csv"
        out, raster, err = run_cli(tmp_path, job_args(dem_path), WDPM_PONDS=str(csv), WDPM_TIMING="1", **devices)
        assert (out, raster) == plain[:2], tag
        assert ("2 devices" in err) == (tag == "two")
        assert re.search(r"^WDPMCL timing: pond inventory +[0-9.]+ s$", err, flags=re.M), err      # the phase line of WDPM_TIMING=1
        assert re.search(r"^WDPMCL: pond inventory: \d+ ponds? written to ", err, flags=re.M), err
        got = parse_csv(csv)
        assert got == want, f"{tag}: first difference {next((a, b) for a, b in zip(got, want) if a != b) if len(got) == len(want) else (len(got), len(want))}"


@pytest.mark.parametrize("mm", ["0", "50"])
def test_min_depth_variable(hip, rasters, tmp_path, mm):
    dem_path = str(rasters / "basin5.asc")
    dem, cellsize = read_asc(dem_path)
    want, _ = binding_inventory(hip, dem, float(mm) / 1000.0)
    csv = tmp_path / "ponds.csv"
    run_cli(tmp_path, job_args(dem_path), WDPM_PONDS=str(csv), WDPM_PONDS_MIN_DEPTH_MM=mm)
    assert parse_csv(csv) == expected_rows(want, cellsize)
