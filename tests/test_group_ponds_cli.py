"""WDPM_PONDS on the WDPMCL command line with several row blocks: the inventory is taken on the group, every block labelled where
it lies.  The synthetic 600 x 900 job of tests/test_ponds_cli.py with WDPM_DEVICES=0,0,0: the CSV equals the one-device CSV, stdout
and the output raster do not change, and the stderr line says how many row blocks there were and how many local ponds were joined
across them - the number the Python binding reports for the same job."""
import os
import re

import numpy as np
import pytest

from pond_cli import ADD_MM, ITER, job_args, read_asc, run_cli
from test_ponds_cli import MISS, parse_csv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synth(tmp_path_factory, hip):
    d = tmp_path_factory.mktemp("group_ponds_cli")
    dem = hip.synth_dem(900, 77)[:600, :].copy()
    dem[100:130, 400:470] = MISS
    with open(d / "synth.asc", "w") as f:
        f.write(f"ncols 900\nnrows 600\nxllcorner 0\nyllcorner 0\ncellsize 2.5\nNODATA_value {MISS:.0f}\n")
        np.savetxt(f, dem, fmt="%.4f")
    return str(d / "synth.asc")


def binding_merged(hip, dem, devices):
    """the same job through the Python binding: `merged` and N of the group inventory"""
    from wdpm_amd.ponds import GroupPonds
    from wdpm_amd.rowblock import Group
    R, Cc = dem.shape
    with Group(hip, "add", R, Cc, MISS, devices) as grp:
        grp.upload_unpadded(dem, None, op=1, add=ADD_MM / 1000.0, rof=1.0, sub=0.0)
        grp.run_block(ITER, 0.005 / 1000)
        with GroupPonds(grp) as p:
            n = p.label(0.001)
            assert p.guard_bad() == 0
            return n, p.stats()["merged"]


def test_three_row_blocks_write_the_one_device_inventory(hip, synth, tmp_path):
    dem, _ = read_asc(synth)
    plain = run_cli(tmp_path, job_args(synth))
    one, three = tmp_path / "one.csv", tmp_path / "three.csv"
    out1, raster1, err1 = run_cli(tmp_path, job_args(synth), WDPM_PONDS=str(one))
    out3, raster3, err3 = run_cli(tmp_path, job_args(synth), WDPM_PONDS=str(three), WDPM_DEVICES="0,0,0", WDPM_TIMING="1")
    assert (out1, raster1) == plain[:2] and (out3, raster3) == plain[:2]
    assert open(three, "rb").read() == open(one, "rb").read()
    rows = parse_csv(three)
    n, merged = binding_merged(hip, dem, [0, 0, 0])
    assert len(rows) == n >= 1
    m = re.search(r"^WDPMCL: pond inventory: (\d+) ponds? written to (.*) \(3 row blocks, (\d+) joined across them\)$", err3, flags=re.M)
    assert m, err3
    assert int(m.group(1)) == n and m.group(2) == str(three) and int(m.group(3)) == merged
    assert "row blocks" not in err1                                    # one device: the line as it was
    assert re.search(r"^WDPMCL timing: pond inventory +[0-9.]+ s$", err3, flags=re.M), err3
