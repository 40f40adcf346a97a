"""The pond outlets over row blocks past the strip gate (include/wdpm_group_pond_outlets.h): 300 000 x 3 on two row blocks of one GPU
with WDPM_PONDS_ROWS_PER_WAVE unset, so that each rank's view holds more than 32 768 segments and the library itself cuts strips of
several rows over the rank's owned rows.  One call, held against the numpy model and the whole-raster answer of the device
(tests/group_pond_outlets_cases.check_outlets)."""
import numpy as np
import pytest

from group_pond_outlets_cases import OutletCase
from group_ponds_cases import MISS, WET
from helpers import rough_dem

pytestmark = pytest.mark.gpu
TABLE_WAVES = 32768      # kTableWaves: the waves ponds_rows_per_wave aims at


def noise_scene(R, Cc):
    """rough ground in steps of 1/8 m, water at density 0.41 - a few millimetres, some cells 3 m - and 3 % NODATA with water on it"""
    rng = np.random.default_rng(R + Cc)
    dem = rough_dem(R, Cc, R + Cc, step=0.125)
    depth = 0.002 + rng.random((R, Cc)) * 0.02
    depth[rng.random((R, Cc)) < 0.02] = 3.0
    water = np.where(rng.random((R, Cc)) < 0.41, depth, 0.0)
    dem[rng.random((R, Cc)) < 0.03] = MISS
    return dem, water


def test_two_row_blocks_of_150000_rows(hip, monkeypatch):
    monkeypatch.delenv("WDPM_PONDS_ROWS_PER_WAVE", raising=False)
    R, Cc = 300000, 3
    dem, water = noise_scene(R, Cc)
    with OutletCase(hip, R, Cc, [0, 0]) as case:
        table, stats, _, _ = case.check(water, dem)
        assert len(table) > 10000 and stats["divide_cells"] > 0 and stats["no_outlet"] < len(table), stats
        for i in range(case.n):
            s = case.ponds.rank_stats(i)
            assert s["segments"] > TABLE_WAVES and s["rows_per_wave"] == -(-s["segments"] // TABLE_WAVES) > 1, s
